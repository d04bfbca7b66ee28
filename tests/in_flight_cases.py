"""Cases for RG_OPT_DEVICE_IN_FLIGHT: the table keeps State.requestInFlight (member/Leadership.java:31) per (group, follower) and the send step of a recorded tick
derives its per-row inputs — which handler sent, how much is in flight — from the tick's own rows. Shared by tests/test_in_flight_gpu.py (an MI355X) and
tests/devemu/emu_cases_in_flight.py (the host emulation of the kernels, small tables).

The oracle keeps no counts, so the cases carry a small MODEL of the rules of include/raftgpu.h ("the send step with device-resident in-flight counts"): counts
per (group, follower), and per row the trigger, both worked out from the ORACLE's outcome rows, round by round. What the tick must have written is then
  - for a triggered row: OracleTable.replicate(gid, heartbeat = the model's, in_flight = the model's counts after the row's decrements) — after which every
    follower with an RG_SEND_APPEND / _SNAPSHOT / _NEED_HOST send has one more in flight;
  - for any other row: the head of OracleTable.read_state(), every send {0, 0, 0, 0, RG_SEND_NONE}, no prepareReplication, no count up;
and send_head.reserved says which of the two (RG_SENT_TRIGGERED, RG_SENT_HEARTBEAT).
The fuzzed cases reuse sparse_rounds_cases.lead() and its seeds unchanged: the counts never feed back into a decision, so the decision stream — and its share of
RG_NEED_HOST rows, repaired on the host as there and capped at 2 % of the listed rows — is that of sparse_rounds_cases.rounds_tick_case. A repaired group is left out
of that tick's send / count comparison and then given the model's counts (rg_in_flight_set): the tick walked rows the host had yet to repair."""
import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import assemble_cases as A
from tests.clock import origin as clock_origin
from tests import oracle_lib
from tests import sparse_rounds_cases as X
from tests.helpers import compare_states, make_state, set_group, simple_log
from tests.sparse_tick_cases import assert_untouched, subset

SENT = (abi.SEND_APPEND, abi.SEND_SNAPSHOT, abi.SEND_NEED_HOST)
HEAD_FIELDS = ("term", "leader_commit", "epoch_index", "epoch_term", "role_epoch", "is_leader", "reserved")
SEND_FIELDS = ("prev_index", "prev_term", "last_index", "count", "kind")
MUST_SEE = ("command", "heartbeat", "untriggered", "gated_heartbeat_a_command_would_pass", "gated_command", "decrement", "clamp", "early_zeroing", "deep", "ragged")
SET_EVERY, SET_AT = 5, 2                                     # every fifth tick (k % 5 == 2: a thin list next, the full one two ticks on) both sides get random counts


class Model:
    """requestInFlight per (group, follower) and the trigger per row, from outcome rows"""

    def __init__(self, groups, cluster, self_slot):
        self.G, self.P, self.F, self.self_slot = groups, cluster, cluster - 1, self_slot
        self.counts = np.zeros((groups, self.F), dtype=np.int64)
        self.seen = dict.fromkeys(MUST_SEE, 0)

    def walk(self, gid, hdr, flags):
        """rounds 0 .. R - 1 of the rows of groups gid ([R][n] event headers and outcome flags) -> (command[n], heartbeat[n]): the handlers that sent since the row's
        last conversion. Moves the counts: zeroed by a conversion to Leader, one down per ack that reached its callback, clamped at 0."""
        hdr, flags = np.asarray(hdr, dtype=np.uint32), np.asarray(flags, dtype=np.uint32)
        R, n = hdr.shape
        c = self.counts[gid]
        command, timeout = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for r in range(R):
            h, f = hdr[r], flags[r]
            kind, slot, status = h & 0xF, (h >> 4) & 0xF, abi.flags_status(f)
            changed = (f & abi.F_ROLE_CHANGED) != 0
            command[changed] = False
            timeout[changed] = False
            won = changed & (abi.flags_role(f) == abi.LEADER)
            if r < R - 1:
                self.seen["early_zeroing"] += int(np.count_nonzero(won & (c.sum(axis=1) > 0)))
            c[won] = 0
            ack = ((kind == abi.EV_AE_ACK) | (kind == abi.EV_IS_ACK)) & ~changed & (status != abi.DROPPED_STALE_ROLE) & (status != abi.BAD_EVENT) & \
                  (slot < self.P) & (slot != self.self_slot)
            i = np.flatnonzero(ack)
            j = np.where(slot[i] < self.self_slot, slot[i], slot[i] - 1).astype(np.int64)
            cur = c[i, j]
            self.seen["decrement"] += int(np.count_nonzero(cur > 0))
            self.seen["clamp"] += int(np.count_nonzero(cur == 0))
            c[i, j] = np.maximum(cur - 1, 0)
            command |= (kind == abi.EV_CLIENT_APPEND) & (status == abi.OK) & ((f & abi.F_LOG_APPEND) != 0)
            timeout |= abi.flags_emit(f) == abi.EMIT_HEARTBEAT
        self.counts[gid] = c
        return command, timeout & ~command

    def plan(self, orc, gid, command, heartbeat, note=None):
        """what the send step must write for the rows of groups gid after their last round -> (head[n], send[n][F]); the oracle prepares and the model counts
        what is sent. note: the rows that count for `seen` (None: all)"""
        n = len(gid)
        st = orc.read_state()
        head, send = np.zeros(n, dtype=abi.SEND_HEAD_DT), np.zeros((n, self.F), dtype=abi.SEND_DT)
        head["term"], head["leader_commit"] = st.current_term[gid], st.commit_index[gid]
        head["epoch_index"], head["epoch_term"], head["role_epoch"] = st.epoch_index[gid], st.epoch_term[gid], st.role_epoch[gid]
        head["is_leader"] = st.role[gid] == abi.LEADER
        trig = command | heartbeat
        T = np.flatnonzero(trig)
        if len(T):
            before = self.counts[gid[T]]
            h, s = orc.replicate(gid=gid[T], heartbeat=heartbeat[T].astype(np.uint8), in_flight=before.astype(np.uint16))
            for f in HEAD_FIELDS[:-1]:
                assert np.array_equal(h[f], head[f][T]), f             # (the state the model read is the state the oracle planned on)
            send[T] = s
            self.counts[gid[T]] = np.minimum(before + np.isin(s["kind"], SENT), 0xFFFF)
            keep = np.ones(len(T), dtype=bool) if note is None else note[T]
            gated = (s["kind"] == abi.SEND_GATED) & keep[:, None]
            hb = heartbeat[T][:, None]
            self.seen["gated_heartbeat_a_command_would_pass"] += int(np.count_nonzero(gated & hb & (before <= abi.IN_FLIGHT_LIMIT)))
            self.seen["gated_command"] += int(np.count_nonzero(gated & ~hb))
        head["reserved"] = trig * abi.SENT_TRIGGERED + heartbeat * abi.SENT_HEARTBEAT
        keep = np.ones(n, dtype=bool) if note is None else note
        self.seen["command"] += int(np.count_nonzero(command & keep))
        self.seen["heartbeat"] += int(np.count_nonzero(heartbeat & keep))
        self.seen["untriggered"] += int(np.count_nonzero(~trig & keep))
        return head, send

    def randomise(self, rng):
        self.counts[:] = rng.integers(0, 24, self.counts.shape)


def same_sends(got, want, ok, where):
    (hg, sg), (hw, sw) = got, want
    for f in HEAD_FIELDS:
        assert np.array_equal(hg[f][ok], hw[f][ok]), (where, "send_head." + f)
    for f in SEND_FIELDS:
        assert np.array_equal(sg[f][ok], sw[f][ok]), (where, "send." + f)


def _model_tick(model, orc, t, note=None):
    """the model's half of tick t (sparse_rounds_cases.lead / assemble_cases.lead): walk the oracle's rows, plan the sends"""
    hdr = t.batch.head["hdr"].reshape(t.R, t.n)
    flags = t.want.reply["flags"].reshape(t.R, t.n)
    command, heartbeat = model.walk(t.gid, hdr, flags)
    model.seen["deep"] += t.R >= 3
    model.seen["ragged"] += t.n % 64 != 0
    return model.plan(orc, t.gid, command, heartbeat, note)


def lead_only(G, P, seed, ticks, first=0, lead="rounds"):
    """the oracle's and the model's half of lockstep_case (lead="rounds") or assembled_case (lead="assembled"), no device -> what the stream shows (Model.seen).
    first: the number of the first tick, as in lockstep_case"""
    _, orc, _, fz, rng, rng2 = X._tables(G, P, seed, device=False)
    model = Model(G, P, 2 % P)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    for k in range(first, first + ticks):
        if k % SET_EVERY == SET_AT:
            model.randomise(rng2)
        t = X.lead(orc, fz, rng, G, k, fired_g, fired_e) if lead == "rounds" else A.lead(orc, fz, rng, G, k, fired_g, fired_e, P)
        if t.n:
            _model_tick(model, orc, t)
        fired_g, fired_e = t.expired[0], t.expired[1]
    orc.close()
    return model.seen


def _after_tick(gpu, orc, shadow, model, tick, t, where, before):
    """everything one tick of a lockstep is held to -> the rows that were repaired on the host (left out of the send / count comparison)"""
    bad = np.zeros(0, dtype=np.int64)
    if t.n:
        bad = X._check_rows(gpu, shadow, t, tick.outcome32(), where, fold=True)
    eo, epo, no = t.expired
    eg, epg, ng = tick.expired()
    assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo), where
    assert np.array_equal(gpu.timers_read(), orc.timers_read()), where
    for a, c in zip(gpu.health_read(), orc.health_read()):
        assert np.array_equal(a, c), where
    fine = np.ones(model.G, dtype=bool)
    if t.n:
        ok = np.ones(t.n, dtype=bool)
        ok[bad] = False
        want = _model_tick(model, orc, t, note=ok)
        same_sends(tick.sends(), want, ok, where)
        if len(bad):
            # a repaired leader: prepared as the oracle just prepared it where the model sent; its counts are the model's from here on
            trig = (want[0]["reserved"][bad] & abi.SENT_TRIGGERED) != 0
            if trig.any():
                b = bad[trig]
                gpu.replicate(gid=t.gid[b], heartbeat=((want[0]["reserved"][b] & abi.SENT_HEARTBEAT) != 0).astype(np.uint8), in_flight=np.zeros((len(b), model.F), np.uint16))
            fine[t.gid[bad]] = False
        rd, ro = tick.readiness(), orc.ready(t.nows[-1], 1, 60)[t.rows]
        assert np.array_equal(rd[ok], ro[ok]), where
    have = gpu.in_flight_read()
    assert np.array_equal(have[fine], model.counts[fine]), (where, "in-flight counts")
    if not fine.all():
        gpu.in_flight_set(model.counts)
    after = gpu.read_state()
    compare_states(orc.read_state(), after, where)
    assert_untouched(before, after, ~t.pick, where)
    assert np.array_equal(have[~t.pick], before.in_flight[~t.pick]), (where, "the counts of a group outside the list moved")
    return bad


def _snapshot(gpu):
    st = gpu.read_state()
    st.in_flight = gpu.in_flight_read()
    return st


def lockstep_case(G, P, seed, ticks, first=0, device_resident=False, compact_any=False, expect_all=True):
    """sparse_rounds_cases.rounds_tick_case's stream through a tick recorded for 8 rounds on a table with the option on. Every tick: outcome rows, deadlines, health,
    the expired list, send heads (reserved included) and send rows and readiness of the listed rows, the counts of the whole table, table state, groups outside
    the list untouched. Every fifth tick device and model get random counts 0 .. 23.
    first: the number the run's first tick carries. lead() takes its fill and its depth from the tick's number (depth DEPTHS[(k // 5) % 5]), so ten ticks
    counted from 0 never reach a depth of 3 at any seed; the caller of a run that short says where its count starts."""
    gpu, orc, shadow, fz, rng, rng2 = X._tables(G, P, seed)
    if compact_any:
        gpu.set_compact_any_cluster(True)
    gpu.set_device_in_flight(True)
    model = Model(G, P, 2 % P)
    tick = engine.Tick2(gpu, X.RMAX, entry_cap=8 * G * X.RMAX, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=G,
                        sparse_rounds=True)
    assert tick.heartbeat is None and tick.in_flight is None
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    listed = left_out = 0
    for k in range(first, first + ticks):
        if k % SET_EVERY == SET_AT:
            model.randomise(rng2)
            gpu.in_flight_set(model.counts)
        t = X.lead(orc, fz, rng, G, k, fired_g, fired_e)
        where = "tick %d (%d rounds x %d rows)" % (k, t.R, t.n)
        before = _snapshot(gpu)
        if t.n:
            tick.refill(t.batch, t.nows)
        else:
            tick.refill(abi.Batch(1, 0, gid=np.zeros(0, np.uint32)), t.nows)
        tick.launch()
        tick.wait()
        bad = _after_tick(gpu, orc, shadow, model, tick, t, where, before)
        listed += t.n
        left_out += len(bad)
        fired_g, fired_e = t.expired[0], t.expired[1]
    print("in-flight lockstep G=%d P=%d seed=%d: %d listed rows, %d left out, seen %s" % (G, P, seed, listed, left_out, model.seen))
    if expect_all:
        assert all(model.seen[k] > 0 for k in MUST_SEE), model.seen
    assert left_out * 50 <= listed, "%d of %d listed rows were left out of the send comparison (cap: 2 %%)" % (left_out, listed)
    tick.close()
    for x in (gpu, orc, shadow):
        x.close()
    return model.seen


# ---- 1. the constructed sequence ---------------------------------------------------------------------------------------------------------------------------------
def constructed_case(G=96):
    """one leader group L among G groups of a 3-node table (self = slot 0: follower A = slot 1, B = slot 2), a neighbour N that is never listed; a one-round sparse
    tick per step, every step held to the oracle and the model AND to literal counts and kinds"""
    L, N, A_, B_ = 5, 6, 1, 2
    st0 = make_state(3, G)
    set_group(st0, L, role=abi.LEADER, term=3, voted_for=0, role_epoch=7, commit=5, log=simple_log(10, term=3))
    gpu, orc = engine.Table(G, 3, 0, False), oracle_lib.OracleTable(G, 3, 0, False)
    gpu.set_device_in_flight(True)
    for x in (gpu, orc):
        x.load_state(st0)
        x.timers_configure(900, 300, 1)
        x.timers_arm(1000)
    model = Model(G, 3, 0)
    model.counts[N] = (7, 9)
    gpu.in_flight_set(model.counts)
    tick = engine.Tick2(gpu, 1, entry_cap=64, expired_cap=G, critical_point=1, cool_down_ms=60, sparse_cap=G)
    gid = np.array([L], dtype=np.uint32)
    clock = [clock_origin() - 9000]

    def step(kind, counts, kinds, reserved, status=None, role=None, **kw):
        clock[0] += 10
        now = [clock[0]]
        b = abi.Batch(1, 1, gid=gid)
        b.put(0, 0, kind, **kw)
        oo = orc.submit(b, now=now)
        orc.timers_update(1, 1, oo.reply, now, gid=gid)
        flags = int(oo.reply["flags"][0])
        if status is not None:
            assert abi.flags_status(flags) == status, (kind, abi.flags_status(flags))
        command, heartbeat = model.walk(gid, b.head["hdr"].reshape(1, 1), oo.reply["flags"].reshape(1, 1))
        want = model.plan(orc, gid, command, heartbeat)
        tick.refill(b, now)
        tick.launch()
        tick.wait()
        where = "step at %d (kind %d)" % (clock[0], kind)
        got = tick.sends()
        same_sends(got, want, np.ones(1, dtype=bool), where)
        orc.timers_expired_epochs(clock[0], capacity=G)
        have = gpu.in_flight_read()
        assert np.array_equal(have, model.counts), where
        assert tuple(have[L]) == counts and tuple(got[1]["kind"][0]) == kinds and int(got[0]["reserved"][0]) == reserved, (where, have[L], got[1]["kind"][0], got[0]["reserved"][0])
        assert tuple(have[N]) == (7, 9), where
        compare_states(orc.read_state(), gpu.read_state(), where)
        if role is not None:
            assert int(orc.read_state().role[L]) == role, where
        return got

    APPEND, GATED, NONE = (abi.SEND_APPEND,) * 2, (abi.SEND_GATED,) * 2, (abi.SEND_NONE,) * 2
    HB, CMD = abi.SENT_TRIGGERED | abi.SENT_HEARTBEAT, abi.SENT_TRIGGERED
    for c in (1, 2, 3):                                          # onTimeout: the limit is 2, so 0, 1 and 2 in flight pass
        sent = step(abi.EV_TIMEOUT, (c, c), APPEND, HB, status=abi.OK)
    step(abi.EV_TIMEOUT, (3, 3), GATED, HB, status=abi.OK)       # 3 > 2
    sent = step(abi.EV_CLIENT_APPEND, (4, 4), APPEND, CMD, status=abi.OK, n=1)      # acceptCommand: the limit is 20
    head, send = sent

    def ack(slot, counts, aux=None, status=None):
        j = slot - 1
        return step(abi.EV_AE_ACK, counts, NONE, 0, status=status, slot=slot, flag=1, a=int(head["term"][0]), b=int(head["epoch_index"][0]), c=int(send["last_index"][0][j]),
                    aux=int(head["role_epoch"][0]) if aux is None else aux)
    ack(A_, (3, 4), status=abi.OK)                               # a tick whose only row is an ack: one down, nothing sent, reserved 0
    ack(A_, (3, 4), aux=int(head["role_epoch"][0]) - 1, status=abi.DROPPED_STALE_ROLE)      # State objects that no longer exist
    for flag, want in ((abi.HEALTH_UNREACHABLE, (3, 3)), (abi.HEALTH_UNREACHABLE | abi.HEALTH_NO_REQUEST, (3, 3))):
        gpu.health_failure([L], [B_], [flag], clock[0])
        orc.health_failure([L], [B_], [flag & 3], clock[0])
        if not flag & abi.HEALTH_NO_REQUEST:
            model.counts[L, B_ - 1] -= 1
        assert tuple(gpu.in_flight_read()[L]) == want == tuple(model.counts[L]), flag
        for a, c in zip(gpu.health_read(), orc.health_read()):
            assert np.array_equal(a, c)
    gpu.health_failure([L, L, L], [B_, B_, A_], [0, 0, abi.HEALTH_NO_REQUEST], clock[0])       # entries may repeat a pair: each takes one off
    orc.health_failure([L, L, L], [B_, B_, A_], [0, 0, 0], clock[0])
    model.counts[L, B_ - 1] -= 2
    assert tuple(gpu.in_flight_read()[L]) == (3, 1)
    ack(B_, (3, 0))
    for c in (2, 1, 0, 0):                                       # down to 0, and one more: clamped
        ack(A_, (c, 0))
    assert model.seen["clamp"] >= 1
    step(abi.EV_CLIENT_APPEND, (1, 1), APPEND, CMD, status=abi.OK, n=1)
    step(abi.EV_AE_REQ, (1, 1), NONE, 0, role=abi.FOLLOWER, slot=A_, a=int(head["term"][0]) + 1, b=10, c=3, d=5)       # steps down; the counts of the dead State objects stay
    for _ in range(8):                                           # ... and wins again: timeouts until it stands, the vote of A
        st = orc.read_state()
        if int(st.role[L]) == abi.LEADER:
            break
        if int(st.role[L]) == abi.CANDIDATE:
            won = step(abi.EV_RV_REPLY, (0, 0), NONE, 0, slot=A_, flag=1, a=int(st.current_term[L]), aux=int(st.role_epoch[L]))
        else:
            step(abi.EV_TIMEOUT, (1, 1), NONE, 0)
    assert int(orc.read_state().role[L]) == abi.LEADER and int(won[0]["is_leader"][0]) == 1
    assert tuple(gpu.in_flight_read()[L]) == (0, 0) and tuple(gpu.in_flight_read()[N]) == (7, 9)
    # rg_load_state resets the counts of the groups it loads, as it resets their health
    step(abi.EV_TIMEOUT, (1, 1), APPEND, HB, status=abi.OK)
    one = make_state(3, 1)
    gpu.load_state(one, first=N)
    assert tuple(gpu.in_flight_read()[N]) == (0, 0) and tuple(gpu.in_flight_read()[L]) == (1, 1)
    tick.close()
    gpu.close()
    orc.close()


def saturation_case(G=96):
    """The counts at the end of a uint16: rg_in_flight_set gives follower A 0xFFFE and follower B 0xFFFF in flight, then a command and a heartbeat trigger the send
    step. Both followers are far beyond either limit, so every send is RG_SEND_GATED and nothing is counted up: the counts stand (no wrap to 0 — the model saturates
    at 0xFFFF, the kernel clamps where it adds); an ack takes exactly one off the follower it names, 0xFFFF included; the neighbour's counts never move."""
    L, N, A_, B_ = 5, 6, 1, 2
    TOP = 0xFFFF
    st0 = make_state(3, G)
    set_group(st0, L, role=abi.LEADER, term=3, voted_for=0, role_epoch=7, commit=5, log=simple_log(10, term=3))
    gpu, orc = engine.Table(G, 3, 0, False), oracle_lib.OracleTable(G, 3, 0, False)
    gpu.set_device_in_flight(True)
    for x in (gpu, orc):
        x.load_state(st0)
        x.timers_configure(900, 300, 1)
        x.timers_arm(1000)
    model = Model(G, 3, 0)
    model.counts[L] = (TOP - 1, TOP)
    model.counts[N] = (TOP, TOP - 1)
    gpu.in_flight_set(model.counts)
    assert np.array_equal(gpu.in_flight_read(), model.counts)
    tick = engine.Tick2(gpu, 1, entry_cap=64, expired_cap=G, critical_point=1, cool_down_ms=60, sparse_cap=G)
    gid = np.array([L], dtype=np.uint32)
    clock = [clock_origin() - 9000]

    def step(kind, counts, kinds, reserved, **kw):
        clock[0] += 10
        now = [clock[0]]
        b = abi.Batch(1, 1, gid=gid)
        b.put(0, 0, kind, **kw)
        oo = orc.submit(b, now=now)
        orc.timers_update(1, 1, oo.reply, now, gid=gid)
        assert abi.flags_status(int(oo.reply["flags"][0])) == abi.OK, (kind, abi.flags_status(int(oo.reply["flags"][0])))
        command, heartbeat = model.walk(gid, b.head["hdr"].reshape(1, 1), oo.reply["flags"].reshape(1, 1))
        want = model.plan(orc, gid, command, heartbeat)
        tick.refill(b, now)
        tick.launch()
        tick.wait()
        where = "step at %d (kind %d)" % (clock[0], kind)
        got = tick.sends()
        same_sends(got, want, np.ones(1, dtype=bool), where)
        orc.timers_expired_epochs(clock[0], capacity=G)
        have = gpu.in_flight_read()
        assert np.array_equal(have, model.counts), where
        assert tuple(have[L]) == counts and tuple(got[1]["kind"][0]) == kinds and int(got[0]["reserved"][0]) == reserved, (where, have[L], got[1]["kind"][0], got[0]["reserved"][0])
        assert tuple(have[N]) == (TOP, TOP - 1), where
        compare_states(orc.read_state(), gpu.read_state(), where)

    GATED, NONE = (abi.SEND_GATED,) * 2, (abi.SEND_NONE,) * 2
    HB, CMD = abi.SENT_TRIGGERED | abi.SENT_HEARTBEAT, abi.SENT_TRIGGERED
    step(abi.EV_CLIENT_APPEND, (TOP - 1, TOP), GATED, CMD, n=1)          # acceptCommand: the limit is 20
    step(abi.EV_TIMEOUT, (TOP - 1, TOP), GATED, HB)                     # onTimeout: the limit is 2
    step(abi.EV_AE_ACK, (TOP - 1, TOP - 1), NONE, 0, slot=B_, flag=1, a=3, b=0, c=10, aux=7)      # one down from the top
    step(abi.EV_AE_ACK, (TOP - 2, TOP - 1), NONE, 0, slot=A_, flag=1, a=3, b=0, c=10, aux=7)
    step(abi.EV_CLIENT_APPEND, (TOP - 2, TOP - 1), GATED, CMD, n=1)
    assert model.seen["gated_command"] >= 4 and model.seen["decrement"] == 2
    tick.close()
    gpu.close()
    orc.close()


# ---- 3. the forms agree -------------------------------------------------------------------------------------------------------------------------------------------
def _pair(G, P, seed):
    a, d, fz, rng = X._pair(G, P, seed)
    for t in (a, d):
        t.set_device_in_flight(True)
    return a, d, fz, rng


def _same(ta, td, a, d, where):
    ed = X._same_ticks(ta, td, a, d, where)
    assert np.array_equal(a.in_flight_read(), d.in_flight_read()), (where, "in-flight counts")
    return ed


def same_as_dense_case(G, R=4, ticks=8, seed=9, P=5, device_resident=False):
    """every group listed at full depth: the sparse tick with a depth against the dense R-round tick, two tables with the option on — every output column (send heads
    with `reserved`, send rows), the counts and the final state are identical; the run has moved counts both ways"""
    a, d, fz, rng = _pair(G, P, seed)
    kw = dict(entry_cap=8 * G * R, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident)
    ta, td = engine.Tick2(a, R, sparse_cap=G, sparse_rounds=True, **kw), engine.Tick2(d, R, **kw)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    every = np.arange(G, dtype=np.uint32)
    ups = downs = 0
    for k in range(ticks):
        if k % 3 == 1:
            c = rng.integers(0, 24, (G, P - 1))
            a.in_flight_set(c)
            d.in_flight_set(c)
        nows = [clock_origin() + 150 * k + 10 * r for r in range(R)]
        cur = a.read_state()
        b = abi.Batch(R, G)
        for r in range(R):
            fz.round(cur, b, r)
        for g, e in zip(fired_g, fired_e):
            b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
        listed = abi.Batch(R, G, gid=every)
        listed.head[:], listed.ab[:], listed.cd[:] = b.head, b.ab, b.cd
        listed.entry_terms, listed.entry_count = b.entry_terms, b.entry_count
        c0 = a.in_flight_read().astype(np.int64)
        ta.refill(listed, nows)
        td.refill(b, nows)
        for t in (ta, td):
            t.launch()
            t.wait()
        ed = _same(ta, td, a, d, "tick %d" % k)
        c1 = a.in_flight_read().astype(np.int64)
        ups, downs = ups + int(np.count_nonzero(c1 > c0)), downs + int(np.count_nonzero(c1 < c0))
        fired_g, fired_e = ed[0], ed[1]
    compare_states(d.read_state(), a.read_state(), "every group listed at full depth vs the dense tick")
    assert ups > 0 and downs > 0, (ups, downs)
    for t in (ta, td):
        t.close()
    a.close()
    d.close()


def one_round_case(G, ticks=8, seed=9, P=5, device_resident=False):
    """io->rounds == 1: the sparse tick with a depth against the one-round sparse tick, the option on: every column, the counts and the final state are identical"""
    a, d, fz, rng = _pair(G, P, seed)
    kw = dict(entry_cap=8 * G, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=G)
    ta, td = engine.Tick2(a, 1, sparse_rounds=True, **kw), engine.Tick2(d, 1, **kw)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    moved = 0
    for k in range(ticks):
        if k % 3 == 1:
            c = rng.integers(0, 24, (G, P - 1))
            a.in_flight_set(c)
            d.in_flight_set(c)
        b = abi.Batch(1, G)
        fz.round(a.read_state(), b, 0)
        pick = rng.random(G) < (0.5, 0.05, 1.0)[k % 3]
        pick[int(rng.integers(0, G))] = True
        for g, e in zip(fired_g, fired_e):
            b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
            pick[int(g)] = True
        sub = subset(b, np.flatnonzero(pick))
        c0 = a.in_flight_read()
        for t in (ta, td):
            t.refill(sub, [clock_origin() + 150 * k])
            t.launch()
            t.wait()
        ed = _same(ta, td, a, d, "tick %d" % k)
        c1 = a.in_flight_read()
        moved += int(np.count_nonzero(c1 != c0))
        assert np.array_equal(c1[~pick], c0[~pick]), "the counts of a group outside the list moved"
        fired_g, fired_e = ed[0], ed[1]
    compare_states(d.read_state(), a.read_state(), "one round: the tick with a depth vs the one-round sparse tick")
    assert moved > 0
    for t in (ta, td):
        t.close()
    a.close()
    d.close()


# ---- 4. from the arrival log ----------------------------------------------------------------------------------------------------------------------------------------
def assembled_case(G=1000, seed=77, ticks=20, P=5, device_resident=False):
    """rg_assemble32(RG_MEM_DEVICE) over the previous tick's expired_* columns and a shuffled arrival log, then the tick with the option on, on the same stream: the host
    fills no per-row column at all and reads gid, count and rounds only AFTER rg_tick2_wait, to check. Send rows and counts against the model, every tick."""
    gpu, orc, shadow, fz, rng, rng2 = X._tables(G, P, seed)
    gpu.set_device_in_flight(True)
    model = Model(G, P, 2 % P)
    RMAX = X.RMAX
    tick = engine.Tick2(gpu, RMAX, entry_cap=8 * G * RMAX, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=G,
                        sparse_rounds=True)
    asm = engine.Assembler(gpu, RMAX * G, max_expired=G)
    pins = []

    def pinned(dtype, k):
        a, p = engine.pinned_like(gpu, np.zeros(max(k, 1), dtype=dtype))
        pins.append(p)
        return a
    log_count, log_gid, log_head, log_abcd = pinned(np.uint32, 1), pinned(np.uint32, RMAX * G), pinned(abi.HEAD_DT, RMAX * G), pinned(abi.QUAD32_DT, RMAX * G)
    origin, deferred, stats = pinned(np.uint32, RMAX * G), pinned(np.uint32, 16), pinned(np.uint32, 4)
    arr = abi.CArrivals()
    arr.count, arr.capacity, arr.gid, arr.head, arr.abcd = log_count.ctypes.data, RMAX * G, log_gid.ctypes.data, log_head.ctypes.data, log_abcd.ctypes.data
    arr.expired_gid, arr.expired_epoch, arr.expired_count, arr.expired_capacity = tick.io.expired_gid, tick.io.expired_epoch, tick.io.expired_count, G
    out = asm.for_tick(tick, origin.ctypes.data, deferred.ctypes.data, 16, stats.ctypes.data)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    listed = left_out = 0
    for k in range(ticks):
        if k % SET_EVERY == SET_AT:
            model.randomise(rng2)
            gpu.in_flight_set(model.counts)
        t = A.lead(orc, fz, rng, G, k, fired_g, fired_e, P)
        where = "tick %d (%d rounds x %d rows)" % (k, t.R, t.n)
        before = _snapshot(gpu)
        lg, lh, la, _, _ = A.arrival_log(t, rng)
        m = len(lg)
        log_gid[:m], log_head[:m], log_abcd[:m], log_count[0] = lg, lh, la, m
        if t.n and t.b32.entry_count:
            tick._put(tick.entry_terms, t.b32.entry_terms[: t.b32.entry_count])
        tick.now[:] = [X.now_of(k, r) for r in range(RMAX)]
        asm.run_device(arr, out)
        tick.launch()
        tick.wait()
        tick.n, tick.depth = int(tick.count[0]), int(tick.depth_now[0])       # (only now, and only to check)
        assert (tick.n, tick.depth) == (t.n, t.R), (where, tick.n, tick.depth)
        assert not t.n or np.array_equal(tick._get(tick.gid, np.uint32, t.n), t.gid), where
        bad = _after_tick(gpu, orc, shadow, model, tick, t, where, before)
        listed += t.n
        left_out += len(bad)
        fired_g, fired_e = t.expired[0], t.expired[1]
    print("in-flight assembled G=%d: %d listed rows, %d left out, seen %s" % (G, listed, left_out, model.seen))
    for k in ("command", "heartbeat", "untriggered", "decrement"):
        assert model.seen[k] > 0, model.seen
    assert left_out * 50 <= listed
    asm.close()
    tick.close()
    for p in pins:
        p.free()
    for x in (gpu, orc, shadow):
        x.close()
    return model.seen


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def refusals_case(G=64):
    """each before any launch, with a message, the table's state as it was"""
    t = engine.Table(G, 3)
    before = t.read_state()

    def unchanged():
        after = t.read_state()
        for f in before.fields():
            assert np.array_equal(getattr(before, f), getattr(after, f)), f
    with pytest.raises(engine.EngineError, match="RG_OPT_DEVICE_IN_FLIGHT takes 0 or 1"):
        t.set_option(abi.OPT_DEVICE_IN_FLIGHT, 2)
    assert t.option(abi.OPT_DEVICE_IN_FLIGHT) == 0
    with pytest.raises(engine.EngineError, match="does not keep in-flight counts"):       # the option is off
        t.in_flight_read()
    with pytest.raises(engine.EngineError, match="does not keep in-flight counts"):
        t.in_flight_set(np.zeros((G, 2), np.uint16))
    unchanged()
    # a tick recorded before the option changed, either way
    for first in (0, 1):
        t.set_option(abi.OPT_DEVICE_IN_FLIGHT, first)
        tick = engine.Tick2(t, 2, expired_cap=G, sparse_cap=G, sparse_rounds=True)
        tick.refill(abi.Batch(1, 0, gid=np.zeros(0, np.uint32)), [5, 6])
        tick.launch()
        tick.wait()
        t.set_option(abi.OPT_DEVICE_IN_FLIGHT, 1 - first)
        with pytest.raises(engine.EngineError, match="changed after rg_tick2_create"):
            tick.launch()
        tick.close()
        unchanged()
    # with the option on: every constructor turns the two columns down
    t.set_option(abi.OPT_DEVICE_IN_FLIGHT, 1)
    assert np.array_equal(t.in_flight_read(), np.zeros((G, 2), np.uint16))       # (switched on again: zero-filled)
    import ctypes as C
    L = engine.lib()
    R = 2
    cols = dict(head=np.zeros(R * G, abi.HEAD_DT), abcd=np.zeros(R * G, abi.QUAD32_DT), now=np.zeros(R, np.int64), row=np.zeros(R * G, abi.OUT32_DT),
                persist32=np.zeros(R * G, abi.PERSIST32_DT), heartbeat=np.zeros(G, np.uint8), in_flight=np.zeros(2 * G, np.uint16))
    gid, count, depth = np.arange(G, dtype=np.uint32), np.zeros(1, np.uint32), np.ones(1, np.uint32)
    for form in ("dense", "sparse", "sparse_rounds"):
        for given in ("heartbeat", "in_flight"):
            io = abi.CTick2Io()
            io.rounds = 1 if form == "sparse" else R
            for name, v in cols.items():
                if name not in ("heartbeat", "in_flight") or name == given:
                    setattr(io, name, v.ctypes.data)
            h = C.c_void_p()
            if form == "dense":
                rc = L.rg_tick2_create(t._h, C.byref(io), C.byref(h))
            elif form == "sparse":
                rw = abi.CTick2Rows()
                rw.gid, rw.count, rw.capacity = gid.ctypes.data, count.ctypes.data, G
                rc = L.rg_tick2_create_sparse(t._h, C.byref(io), C.byref(rw), C.byref(h))
            else:
                rw = abi.CTick2Rounds()
                rw.gid, rw.count, rw.rounds, rw.capacity = gid.ctypes.data, count.ctypes.data, depth.ctypes.data, G
                rc = L.rg_tick2_create_sparse_rounds(t._h, C.byref(io), C.byref(rw), C.byref(h))
            assert rc == -1 and not h.value and b"RG_OPT_DEVICE_IN_FLIGHT" in L.rg_last_error(t._h), (form, given, rc, L.rg_last_error(t._h))
    unchanged()
    t.close()


# ---- 6. the option off ---------------------------------------------------------------------------------------------------------------------------------------------
def option_off_case(G=1000, P=5, seed=77, ticks=10, device_resident=False):
    """two tables on one stream with host columns: one that never heard of the option, one where it is explicitly 0 (after having been 1): every column of every
    tick — send heads with `reserved` == 0, send rows — and the final state are identical bit for bit"""
    a, d, fz, rng = X._pair(G, P, seed)
    a.set_option(abi.OPT_DEVICE_IN_FLIGHT, 1)
    a.set_option(abi.OPT_DEVICE_IN_FLIGHT, 0)
    R = 3
    kw = dict(entry_cap=8 * G * R, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=G, sparse_rounds=True)
    ta, td = engine.Tick2(a, R, **kw), engine.Tick2(d, R, **kw)
    assert ta.heartbeat is not None and ta.in_flight is not None
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    for k in range(ticks):
        nows = [clock_origin() + 150 * k + 10 * r for r in range(R)]
        cur = a.read_state()
        b = abi.Batch(R, G)
        for r in range(R):
            fz.round(cur, b, r)
        for g, e in zip(fired_g, fired_e):
            b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
        pick = rng.random(G) < (0.5, 0.05, 1.0)[k % 3]
        pick[fired_g] = True
        pick[int(rng.integers(0, G))] = True
        rows = np.flatnonzero(pick)
        n = len(rows)
        sub = abi.Batch(R, n, gid=rows.astype(np.uint32))
        sub.head[:] = b.head.reshape(R, G)[:, rows].reshape(-1)
        sub.ab[:], sub.cd[:] = b.ab.reshape(R, G)[:, rows].reshape(-1), b.cd.reshape(R, G)[:, rows].reshape(-1)
        sub.entry_terms, sub.entry_count = b.entry_terms, b.entry_count
        hb, fl = X._traffic(rng, n, P)
        for t in (ta, td):
            t.refill(sub, nows, heartbeat=hb, in_flight=fl.T.reshape(-1))
            t.launch()
            t.wait()
        ed = X._same_ticks(ta, td, a, d, "tick %d" % k)
        assert not np.any(ta.sends()[0]["reserved"]), "reserved is 0 with the option off"
        fired_g, fired_e = ed[0], ed[1]
    compare_states(d.read_state(), a.read_state(), "the option explicitly off vs a plain table")
    with pytest.raises(engine.EngineError, match="does not keep in-flight counts"):
        a.in_flight_read()
    for t in (ta, td):
        t.close()
    a.close()
    d.close()
