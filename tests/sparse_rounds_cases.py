"""Cases for R ROUNDS of a list of groups in one launch: rg_submit32c_sparse_rounds (stand-alone) and the sparse device-resident tick that reads its row
count AND its depth when the graph runs (rg_tick2_create_sparse_rounds). Shared by tests/test_sparse_rounds_gpu.py (an MI355X) and
tests/devemu/emu_cases_sparse_rounds.py (the host emulation of the kernels, small tables).

tests/oracle_lib.OracleTable takes a gid list with ONE round only, so the fuzzed cases LEAD WITH THE ORACLE, round by round: for every round of a launch the
oracle's state is read, fuzz.Fuzzer(allow_miss=False) draws a dense round from it, the listed rows are kept (sparse_tick_cases.subset), about 40 % of them
are blanked to RG_EV_NONE (so depths are ragged), the single round is submitted to the oracle (and folded into its timers). Then all R rounds go to the
device in ONE call, which must give the same rows, the same table state, the same deadlines, statistics, send rows and readiness.

RG_NEED_HOST. The oracle keeps a lossless log and never answers RG_NEED_HOST; the device does, where a lookup leaves the four term runs it caches — and the
fuzzer, which here sees the ORACLE's state between the rounds of a launch, cannot steer clear of every such lookup (on the emulation: about one row in
6 000). So the oracle alone cannot show that a stream is free of them (lead_only() below, the oracle's half of a case, counts 0 for every stream by
construction), and the fuzzed cases do what a host does instead: a SHADOW oracle, one launch behind, stands in for the host's log; the row that answered RG_NEED_HOST is resubmitted with its hint
and the rows of its group that the launch skipped are resubmitted after it, round by round (repair()). Every row — the repaired ones included — must then equal
the oracle's, and so must the table. For the tick the repaired rows are folded into the timers and statistics on the host, and their groups (at most 2 % of the
listed rows, asserted; the stand-alone case asserts the same cap on the rows it repairs) are left out of that tick's send / readiness comparison, as
tests/sparse_tick_cases.py does for its one-round ticks.
The constructed case need_host_case() pins what the launch itself answers: RG_NEED_HOST, then RG_SKIPPED_AFTER_NEED_HOST, the group's state as it was."""
import types

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import auto_base_stream as S
from tests import clock
from tests import fuzz, oracle_lib
from tests.helpers import check_out32_rows, compare_outcomes, compare_states
from tests.sparse_tick_cases import assert_untouched, repair_need_host, subset

FILLS = (0.0, 0.01, 0.1, 0.5, 1.0)
DEPTHS = (1, 2, 3, 5, 8)
RMAX = max(DEPTHS)
KEEP = 0.6                                                   # share of the listed rows of a round that keep their event


def now_of(k, r):
    return clock.origin() + 150 * k + 10 * r


def lead(orc, fz, rng, G, k, fired_g, fired_e, fold=True):
    """the oracle's half of launch k: pick the list and the depth, then decide round after round -> what the device is to be given and what it must answer"""
    fill, R = FILLS[k % len(FILLS)], DEPTHS[(k // len(FILLS)) % len(DEPTHS)]
    pick = rng.random(G) < fill if fill > 0 else np.zeros(G, dtype=bool)
    if fill > 0:
        pick[fired_g] = True                                 # the tickets that fired at the end of the previous tick: their onTimeout, fenced, in round 0
    rows = np.flatnonzero(pick)
    n = len(rows)
    gid = rows.astype(np.uint32)
    nows = [now_of(k, r) for r in range(R)]
    start = orc.read_state()
    subs, outs, dense = [], [], []
    early = 0
    for r in range(R):
        if not n:
            break
        cur = start if r == 0 else orc.read_state()
        b = abi.Batch(1, G)
        fz.round(cur, b, 0)
        if r == 0:
            for g, e in zip(fired_g, fired_e):
                b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
        sub = subset(b, rows)
        drop = rng.random(n) >= KEEP
        if r == 0:
            drop[np.isin(rows, fired_g)] = False             # (a fired group's TIMEOUT row is never blanked)
        sub.head[drop] = (0, 0)
        assert abi.batch_fits_32(sub)
        oo = orc.submit(sub, now=[nows[r]])
        if fold:
            orc.timers_update(1, n, oo.reply, [nows[r]], gid=gid)
        if r < R - 1:
            early += int(np.count_nonzero(oo.reply["flags"] & abi.F_ROLE_CHANGED))
        subs.append(sub)
        outs.append(oo)
        dense.append(b)
    batch = want = None
    if n:
        batch = fuzz.concat_batches(subs)
        batch.gid = gid
        want = fuzz.concat_outcomes(outs)
    expired = orc.timers_expired_epochs(nows[-1], capacity=G)
    return types.SimpleNamespace(k=k, fill=fill, R=R, pick=pick, rows=rows, gid=gid, n=n, nows=nows, start=start, batch=batch, want=want, expired=expired,
                                 early_conversions=early, subs=subs, dense=dense)


def _tables(G, P, seed, device=True):
    self_slot = 2 % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    orc = oracle_lib.OracleTable(G, P, self_slot, True)
    gpu = engine.Table(G, P, self_slot, True) if device else None
    shadow = oracle_lib.OracleTable(G, P, self_slot, True) if device else None       # the host's log: one launch behind (repair())
    if shadow is not None:
        shadow.load_state(st0)
    for t in (gpu, orc):
        if t is not None:
            t.load_state(st0)
            t.timers_configure(900, 300, 4321)
            t.timers_arm(clock.origin())
    return gpu, orc, shadow, fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False), np.random.default_rng(seed), np.random.default_rng(seed + 1000)


def _traffic(rng2, n, P):
    return (rng2.random(n) < 0.5).astype(np.uint8), rng2.integers(0, 24, (n, P - 1)).astype(np.uint16)


def lead_only(G, P, seed, ticks, replicate=True):
    """the oracle's half of standalone_rounds_case (replicate=False) or rounds_tick_case (replicate=True) -> (rows, RG_NEED_HOST rows)"""
    _, orc, _, fz, rng, rng2 = _tables(G, P, seed, device=False)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    rows = need = 0
    for k in range(ticks):
        t = lead(orc, fz, rng, G, k, fired_g, fired_e)
        if t.n:
            rows += t.R * t.n
            need += int(np.count_nonzero(abi.flags_status(t.want.reply["flags"]) == abi.NEED_HOST))
            if replicate:
                hb, fl = _traffic(rng2, t.n, P)
                orc.replicate(gid=t.gid, heartbeat=hb, in_flight=fl)
        fired_g, fired_e = t.expired[0], t.expired[1]
    orc.close()
    return rows, need


def _rows_of(t, q, idx):
    """rows idx of round q of launch t as a one-round list batch (the rows as the launch had them: blanked ones are RG_EV_NONE)"""
    s = subset(t.subs[q], idx)
    s.gid = t.gid[idx]
    return s


def repair(gpu, shadow, t, got, fold=False):
    """The host half of the RG_NEED_HOST protocol for one launch of R rounds, and the shadow oracle's step through it. `shadow` holds the state BEFORE the
    launch (the host's log); round by round: the rows the launch skipped are resubmitted (wide rows, one round, their groups listed), a row that answers
    RG_NEED_HOST — in the launch or now — gets its hint from the shadow (sparse_tick_cases.repair_need_host) and, with fold, the rows decided here are folded
    into the device's timers and statistics at the round's clock; then the shadow decides the round. `got` (the unpacked R x n rows) is repaired in place.
    -> the rows of the list (columns) that needed it"""
    R, n = t.R, t.n
    status = got.status.reshape(R, n).copy()
    cols = np.flatnonzero((status == abi.NEED_HOST).any(axis=0))
    first = np.argmax(status[:, cols] == abi.NEED_HOST, axis=0) if len(cols) else np.zeros(0, dtype=np.int64)
    kinds = (t.batch.head["hdr"] & 0xF).reshape(R, n)
    for q in range(R):
        if len(cols):
            sl = slice(q * n, (q + 1) * n)
            view = abi.Outcome(0)
            view.reply, view.logfx, view.persist = got.reply[sl], got.logfx[sl], got.persist[sl]
            # every later row of a stopped group: its events were skipped, and its RG_EV_NONE rows name the role epoch the launch left the group with
            skipped = cols[first < q]
            assert np.all((status[q, skipped] == abi.SKIPPED_AFTER_NEED_HOST) == (kinds[q, skipped] != abi.EV_NONE))
            assert np.count_nonzero(status[q] == abi.SKIPPED_AFTER_NEED_HOST) == np.count_nonzero(kinds[q, skipped] != abi.EV_NONE)
            if len(skipped):
                again = gpu.submit(_rows_of(t, q, skipped), fill=0xAB)
                view.reply[skipped], view.logfx[skipped], view.persist[skipped] = again.reply, again.logfx, again.persist
            need = np.flatnonzero(view.status == abi.NEED_HOST)
            if len(need):
                repair_need_host(gpu, shadow, t.dense[q], t.rows, view, shadow.read_state())
            done = np.union1d(skipped, need)
            if fold and len(done):
                gpu.timers_update(1, len(done), view.reply[done], [t.nows[q]], gid=t.gid[done])
                gpu.health_update(_rows_of(t, q, done), view.reply[done], [t.nows[q]])
        shadow.submit(t.subs[q])
    return cols


def _check_rows(gpu, shadow, t, raw, where, fold=False):
    """the R x n compact outcome rows of one launch against the oracle's (after the host's repair of what answered RG_NEED_HOST), and the raw-row rules of
    helpers.check_out32_rows for a launch that needed none -> the columns that were repaired"""
    got, _ = engine.unpack32(raw, t.R, t.n, t.start.role_epoch[t.rows])
    clean = not np.any(got.status == abi.NEED_HOST)
    cols = repair(gpu, shadow, t, got, fold)
    assert clean == (len(cols) == 0)
    compare_outcomes(t.want, got, where)
    if clean:
        after = gpu.read_state()
        check_out32_rows(raw, got, types.SimpleNamespace(commit_index=t.start.commit_index[t.rows], role_epoch=t.start.role_epoch[t.rows]),
                         types.SimpleNamespace(commit_index=after.commit_index[t.rows], role_epoch=after.role_epoch[t.rows]), t.R, t.n)
    return cols


def _note(seen, t, G):
    seen["deep"] += t.n > 0 and t.R >= 3
    seen["ragged"] += t.n % 64 != 0
    seen["full"] += t.n == G
    seen["early_conversion"] += t.early_conversions


def standalone_rounds_case(G, P, seed, ticks, expect_all=True):
    """rg_submit32c_sparse_rounds in lockstep with the oracle. The oracle keeps timers (they shape the stream: a fired group's fenced TIMEOUT row in round 0 of the
    next launch); the device only decides. A launch without rows is skipped: the call launches nothing."""
    gpu, orc, shadow, fz, rng, _ = _tables(G, P, seed)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    seen = dict(deep=0, ragged=0, full=0, early_conversion=0)
    rows = repaired = listed = 0
    for k in range(ticks):
        t = lead(orc, fz, rng, G, k, fired_g, fired_e)
        fired_g, fired_e = t.expired[0], t.expired[1]
        if not t.n:
            continue
        where = "launch %d (%d rounds x %d rows)" % (k, t.R, t.n)
        before = gpu.read_state()
        raw = gpu.submit32c_sparse_rounds(t.batch, fill=0xAB)
        assert_untouched(before, gpu.read_state(), ~t.pick, where)
        repaired += len(_check_rows(gpu, shadow, t, raw, where))
        after = gpu.read_state()
        compare_states(orc.read_state(), after, where)
        assert_untouched(before, after, ~t.pick, where)
        _note(seen, t, G)
        rows += t.R * t.n
        listed += t.n
    if expect_all:
        assert all(v > 0 for v in seen.values()), seen
    assert repaired * 50 <= listed, "%d of %d listed rows had to be repaired on the host (cap: 2 %%)" % (repaired, listed)
    for x in (gpu, orc, shadow):
        x.close()
    return rows, repaired


def rounds_tick_case(G, seed, ticks, P=5, device_resident=False, expect_all=True):
    """the sparse tick with a depth, recorded for 8 rounds at capacity G: tick k has fill FILLS[k % 5] (+ last tick's fired groups) and depth DEPTHS[(k // 5) % 5].
    Every tick: outcome rows, deadlines, health columns, the expired list with epochs and count, send heads and rows and readiness of the listed rows,
    whole-table state, groups outside the list untouched."""
    gpu, orc, shadow, fz, rng, rng2 = _tables(G, P, seed)
    tick = engine.Tick2(gpu, RMAX, entry_cap=8 * G * RMAX, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=G,
                        sparse_rounds=True)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    seen = dict(deep=0, ragged=0, full=0, early_conversion=0, empty_with_fired=0, append=0, ready0=0, ready1=0)
    rows = listed = left_out = 0
    for k in range(ticks):
        t = lead(orc, fz, rng, G, k, fired_g, fired_e)
        where = "tick %d (%d rounds x %d rows)" % (k, t.R, t.n)
        before = gpu.read_state()
        if t.n:
            hb, fl = _traffic(rng2, t.n, P)
            tick.refill(t.batch, t.nows, heartbeat=hb, in_flight=fl.T.reshape(-1))
        else:
            tick.refill(abi.Batch(1, 0, gid=np.zeros(0, np.uint32)), t.nows)
        tick.launch()
        tick.wait()
        bad = np.zeros(0, dtype=np.int64)
        if t.n:
            bad = _check_rows(gpu, shadow, t, tick.outcome32(), where, fold=True)
        eo, epo, no = t.expired
        eg, epg, ng = tick.expired()
        assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo), where
        assert np.array_equal(gpu.timers_read(), orc.timers_read()), where
        for a, c in zip(gpu.health_read(), orc.health_read()):
            assert np.array_equal(a, c), where
        if t.n:
            ok = np.ones(t.n, dtype=bool)
            ok[bad] = False                                  # (repaired on the host after the tick: the tick planned their sends on the state it had)
            (hg, sg), (ho, so) = tick.sends(), orc.replicate(gid=t.gid, heartbeat=hb, in_flight=fl)
            if len(bad):
                gpu.replicate(gid=t.gid[bad], heartbeat=hb[bad], in_flight=fl[bad])      # (prepareReplication of a repaired leader, as the oracle just ran it)
            for f in ("term", "leader_commit", "epoch_index", "epoch_term", "role_epoch", "is_leader"):
                assert np.array_equal(hg[f][ok], ho[f][ok]), (where, f)
            for f in ("prev_index", "prev_term", "last_index", "count", "kind"):
                assert np.array_equal(sg[f][ok], so[f][ok]), (where, f)
            rd, ro = tick.readiness(), orc.ready(t.nows[-1], 1, 60)[t.rows]
            assert np.array_equal(rd[ok], ro[ok]), where
            seen["append"] += int(np.count_nonzero(so["kind"] == abi.SEND_APPEND))
            seen["ready0"] += int(np.count_nonzero(ro == 0))
            seen["ready1"] += int(np.count_nonzero(ro == 1))
        after = gpu.read_state()                             # (the send side prepares the listed leaders)
        compare_states(orc.read_state(), after, where)
        assert_untouched(before, after, ~t.pick, where)
        seen["empty_with_fired"] += t.n == 0 and ng > 0
        _note(seen, t, G)
        rows += t.R * t.n
        listed += t.n
        left_out += len(bad)
        fired_g, fired_e = eg, epg
    if expect_all:
        assert all(v > 0 for v in seen.values()), seen
    assert left_out * 50 <= listed, "%d of %d listed rows were left out of the send / readiness comparison (cap: 2 %%)" % (left_out, listed)
    tick.close()
    for x in (gpu, orc, shadow):
        x.close()
    return rows, left_out


# ---- RG_NEED_HOST inside a launch --------------------------------------------------------------------------------------------------------------------------
def need_host_case(G=512, P=3, R=4, seed=23):
    """Hand-made AppendEntries whose prevLogIndex lies below the four cached term runs (groups with six runs, as test_gpu_parity.test_need_host_blocks_later_rounds
    builds them), no hint column, R = 4 rounds, a third of the groups listed: a miss in round 0, 1 or 2, events after it, groups without a miss beside them.
    The oracle's log is lossless: it never answers RG_NEED_HOST. So the device decides first; what it must then have done is the oracle's DENSE R-round
    submit of the embedded batch (RG_EV_NONE outside the list) in which every group that answered RG_NEED_HOST in round r carries RG_EV_NONE from round r
    on: the rows before r equal the oracle's, row r says RG_NEED_HOST, every later event of the group RG_SKIPPED_AFTER_NEED_HOST, and the whole table — the
    stopped groups' state as round r found it — equals the oracle's. The same rows, bit for bit, come from rg_submit32c on the dense embedded batch."""
    self_slot = 0
    st0 = abi.GroupState(G, P, runs_total=6 * G)
    for g in range(G):
        st0.role[g], st0.current_term[g] = abi.FOLLOWER, 9
        st0.run_count[g], st0.run_offset[g] = 6, 6 * g
        st0.first_index[g], st0.last_index[g] = 1, 60
        for k in range(6):
            st0.run_start[6 * g + k], st0.run_term[6 * g + k] = 1 + 10 * k, 1 + k
    gpu, dev, orc = engine.Table(G, P, self_slot, True), engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    for t in (gpu, dev, orc):
        t.load_state(st0)
    st0 = gpu.read_state()                                       # (the newest four runs: what the device keeps)
    miss, hit, older = dict(a=9, b=15, c=2, d=0), dict(a=9, b=60, c=6, d=30), dict(a=9, b=25, c=3, d=0)      # (index 15 lies in a forgotten run; 25 and 60 are cached)
    plans = ([miss, hit, None, hit], [hit, miss, hit, older], [older, hit, None, hit], [None, None, miss, hit])
    dense = abi.Batch(R, G)
    for g in range(G):
        for r, ev in enumerate(plans[g % len(plans)]):
            if ev is not None:
                dense.put(r, g, abi.EV_AE_REQ, slot=1, **ev)
    pick = np.random.default_rng(seed).random(G) < 0.34
    rows = np.flatnonzero(pick)
    n = len(rows)
    head2 = dense.head.reshape(R, G)
    head2[:, ~pick] = (0, 0)                                     # the embedded batch: nothing outside the list
    assert abi.batch_fits_32(dense)
    sub = abi.Batch(R, n, gid=rows.astype(np.uint32))
    sub.head[:] = head2[:, rows].reshape(-1)
    sub.ab[:], sub.cd[:] = dense.ab.reshape(R, G)[:, rows].reshape(-1), dense.cd.reshape(R, G)[:, rows].reshape(-1)
    sub.entry_terms, sub.entry_count = dense.entry_terms, dense.entry_count
    raw = gpu.submit32c_sparse_rounds(sub, wide=False)
    full = dev.submit32c(dense, wide=False)                      # contract (1): outcome row (r, i) equals dense row (r, gid[i])
    picked = abi.Outcome32(R * n, wide=False)
    picked.row, picked.persist = full.row.reshape(R, G)[:, rows].reshape(-1), full.persist.reshape(R, G)[:, rows].reshape(-1)
    _same_rows(raw, picked, "the list call vs rg_submit32c on the embedded batch")
    compare_states(dev.read_state(), gpu.read_state(), "the list call vs rg_submit32c on the embedded batch")
    got, _ = engine.unpack32(raw, R, n, st0.role_epoch[rows])
    st = got.status.reshape(R, n)
    kinds = (sub.head["hdr"] & 0xF).reshape(R, n)
    stopped = early = skipped = 0
    decided = np.ones((R, n), dtype=bool)                        # rows the device decided: all but an RG_NEED_HOST row and what follows it
    for i in np.flatnonzero((st == abi.NEED_HOST).any(axis=0)):
        r = int(np.argmax(st[:, i] == abi.NEED_HOST))
        later = kinds[r + 1:, i] != abi.EV_NONE
        assert np.all(st[r + 1:, i][later] == abi.SKIPPED_AFTER_NEED_HOST), (i, r)
        decided[r:, i] = False
        head2[r:, rows[i]] = (0, 0)
        stopped += 1
        early += r < R - 1
        skipped += int(np.count_nonzero(later))
    assert not np.any(st[decided] == abi.SKIPPED_AFTER_NEED_HOST)
    assert stopped > 0 and early > 0 and skipped > 0, (stopped, early, skipped)
    oo = orc.submit(dense, fill=0xAB)
    keep = np.flatnonzero(decided.reshape(-1))
    want, have = abi.Outcome(len(keep)), abi.Outcome(len(keep))
    for name in ("reply", "logfx", "persist"):
        getattr(want, name)[:] = getattr(oo, name).reshape(R, G)[:, rows].reshape(-1)[keep]
        getattr(have, name)[:] = getattr(got, name)[keep]
    compare_outcomes(want, have, "RG_NEED_HOST inside a launch: the rows decided")
    after = gpu.read_state()
    compare_states(orc.read_state(), after, "RG_NEED_HOST inside a launch")
    at0 = np.zeros(G, dtype=bool)
    at0[rows[st[0] == abi.NEED_HOST]] = True
    assert_untouched(st0, after, ~pick | at0, "a group stopped in round 0, or outside the list")
    for t in (gpu, dev, orc):
        t.close()
    return stopped, skipped


# ---- equivalences with the existing forms (the same tree: a second yardstick beside the oracle) -------------------------------------------------------------
def _same_rows(ra, rd, where):
    flags = rd.row["flags"]
    for f in ("resp_term", "flags", "commit_index"):
        assert np.array_equal(ra.row[f], rd.row[f]), (where, f)
    lf = ((flags & (abi.F_LOG_APPEND | abi.F_LOG_TRUNC)) != 0) | (abi.flags_status(flags) == abi.NEED_HOST)      # (log_from is defined under these marks only)
    assert np.array_equal(ra.row["log_from"][lf], rd.row["log_from"][lf]), where
    per = (flags & abi.F_PERSIST) != 0
    assert np.array_equal(ra.persist[per], rd.persist[per]), where


def _same_ticks(ta, td, a, d, where):
    _same_rows(ta.outcome32(), td.outcome32(), where)
    ea, ed = ta.expired(), td.expired()
    assert ea[2] == ed[2] and np.array_equal(ea[0], ed[0]) and np.array_equal(ea[1], ed[1]), where
    (ha, sa), (hd, sd) = ta.sends(), td.sends()
    assert np.array_equal(ha, hd) and np.array_equal(sa, sd), where
    assert np.array_equal(ta.readiness(), td.readiness()), where
    assert np.array_equal(a.timers_read(), d.timers_read()), where
    for x, y in zip(a.health_read(), d.health_read()):
        assert np.array_equal(x, y), where
    return ed


def _pair(G, P, seed):
    self_slot = 2 % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    a, d = engine.Table(G, P, self_slot, True), engine.Table(G, P, self_slot, True)
    for t in (a, d):
        t.load_state(st0)
        t.timers_configure(900, 300, 99)
        t.timers_arm(clock.origin())
    return a, d, fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False), np.random.default_rng(seed)


def one_round_case(G, ticks=12, seed=9, P=5, device_resident=False):
    """R = 1: rg_submit32c_sparse_rounds against rg_submit32c_sparse, and a tick recorded with rg_tick2_create_sparse_rounds for ONE round against
    rg_tick2_create_sparse, on two tables fed the same stream: every column and the final state are identical"""
    a, d, fz, rng = _pair(G, P, seed)
    kw = dict(entry_cap=8 * G, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=G)
    ta, td = engine.Tick2(a, 1, sparse_rounds=True, **kw), engine.Tick2(d, 1, **kw)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    for k in range(ticks):
        now = clock.origin() + 150 * k
        b = abi.Batch(1, G)
        fz.round(a.read_state(), b, 0)
        pick = rng.random(G) < (0.5, 0.05, 1.0)[k % 3]
        pick[int(rng.integers(0, G))] = True
        rows = np.flatnonzero(pick)
        sub = subset(b, rows)
        if k % 2 == 0:                                           # the stand-alone pair
            ra, rd = a.submit32c_sparse_rounds(sub, wide=False), d.submit32c_sparse(sub, wide=False)
            _same_rows(ra, rd, "stand-alone, launch %d" % k)
            continue
        for g, e in zip(fired_g, fired_e):
            b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
            pick[int(g)] = True
        rows = np.flatnonzero(pick)
        sub = subset(b, rows)
        hb, fl = _traffic(rng, len(rows), P)
        for t in (ta, td):
            t.refill(sub, [now], heartbeat=hb, in_flight=fl.T.reshape(-1))
            t.launch()
            t.wait()
        ed = _same_ticks(ta, td, a, d, "tick %d" % k)
        fired_g, fired_e = ed[0], ed[1]
    compare_states(d.read_state(), a.read_state(), "one round: the forms with a depth vs the one-round forms")
    for t in (ta, td):
        t.close()
    a.close()
    d.close()


def same_as_dense_case(G, R=4, ticks=10, seed=9, P=5, device_resident=False, depth_pointer=True):
    """every group listed at full depth (gid[i] = i, n = capacity = groups, *rounds = io->rounds — or no `rounds` pointer at all) against the dense R-round tick:
    every output column and the final state are identical"""
    a, d, fz, rng = _pair(G, P, seed)
    kw = dict(entry_cap=8 * G * R, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident)
    ta, td = engine.Tick2(a, R, sparse_cap=G, sparse_rounds=True, depth_pointer=depth_pointer, **kw), engine.Tick2(d, R, **kw)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    every = np.arange(G, dtype=np.uint32)
    for k in range(ticks):
        nows = [clock.origin() + 150 * k + 10 * r for r in range(R)]
        cur = a.read_state()
        b = abi.Batch(R, G)
        for r in range(R):
            fz.round(cur, b, r)
        for g, e in zip(fired_g, fired_e):
            b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
        listed = abi.Batch(R, G, gid=every)
        listed.head[:], listed.ab[:], listed.cd[:] = b.head, b.ab, b.cd
        listed.entry_terms, listed.entry_count = b.entry_terms, b.entry_count
        hb, fl = _traffic(rng, G, P)
        ta.refill(listed, nows, heartbeat=hb, in_flight=fl.T.reshape(-1))
        td.refill(b, nows, heartbeat=hb, in_flight=fl.T.reshape(-1))
        for t in (ta, td):
            t.launch()
            t.wait()
        ed = _same_ticks(ta, td, a, d, "tick %d" % k)
        fired_g, fired_e = ed[0], ed[1]
    compare_states(d.read_state(), a.read_state(), "every group listed at full depth vs the dense tick")
    for t in (ta, td):
        t.close()
    a.close()
    d.close()


SENTINEL = 0xAB


def partial_depth_case(G=256, P=5, seed=31, n=100):
    """a tick recorded for 8 rounds at capacity G, run with *rounds = 2 and n < capacity rows: rounds 0 and 1 of the n rows equal the oracle's, rounds 2 .. 7 and
    rows >= n of EVERY output column keep a sentinel fill. Then *rounds = 100 on an 8-round refill: clamped to 8."""
    gpu, orc, shadow, fz, rng, rng2 = _tables(G, P, seed)
    F = P - 1
    tick = engine.Tick2(gpu, RMAX, entry_cap=8 * G * RMAX, expired_cap=G, critical_point=1, cool_down_ms=60, sparse_cap=G, sparse_rounds=True)   # (host-pinned: numpy views)
    rows = np.sort(rng.choice(G, n, replace=False))
    gid = rows.astype(np.uint32)

    def rounds_of(R, k):
        start = orc.read_state()
        subs, outs, dense = [], [], []
        for r in range(R):
            b = abi.Batch(1, G)
            fz.round(orc.read_state(), b, 0)
            sub = subset(b, rows)
            oo = orc.submit(sub, now=[now_of(k, r)])
            orc.timers_update(1, n, oo.reply, [now_of(k, r)], gid=gid)
            subs.append(sub)
            outs.append(oo)
            dense.append(b)
        batch = fuzz.concat_batches(subs)
        batch.gid = gid
        return types.SimpleNamespace(R=R, n=n, rows=rows, gid=gid, nows=[now_of(k, r) for r in range(R)], start=start, batch=batch,
                                     want=fuzz.concat_outcomes(outs), subs=subs, dense=dense)

    def run(R, k, given=None):
        where = "depth %d of %d" % (R, RMAX)
        t = rounds_of(R, k)
        hb, fl = _traffic(rng2, n, P)
        tick.refill(t.batch, t.nows, heartbeat=hb, in_flight=fl.T.reshape(-1))
        if given is not None:
            tick.depth_now[0] = given
        for col in (tick.row, tick.persist32, tick.send_head, tick.send, tick.ready):
            col.view(np.uint8)[:] = SENTINEL
        tick.launch()
        tick.wait()
        ok = np.ones(n, dtype=bool)
        ok[_check_rows(gpu, shadow, t, tick.outcome32(), where, fold=True)] = False
        eo, epo, no = orc.timers_expired_epochs(t.nows[-1], capacity=G)
        eg, epg, ng = tick.expired()
        assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo)
        assert np.array_equal(gpu.timers_read(), orc.timers_read())
        (hg, sg), (ho, so) = tick.sends(), orc.replicate(gid=gid, heartbeat=hb, in_flight=fl)
        if not ok.all():
            gpu.replicate(gid=gid[~ok], heartbeat=hb[~ok], in_flight=fl[~ok])
        assert np.array_equal(hg["is_leader"][ok], ho["is_leader"][ok]) and np.array_equal(sg["kind"][ok], so["kind"][ok])
        assert np.array_equal(tick.readiness()[ok], orc.ready(t.nows[-1], 1, 60)[rows][ok])
        compare_states(orc.read_state(), gpu.read_state(), where)
        for name, col in (("row", tick.row), ("persist32", tick.persist32)):
            img = col.view(np.uint8).reshape(RMAX, G, 16)
            assert np.all(img[R:] == SENTINEL), "%s: a round at or beyond the depth was written" % name
            assert np.all(img[:R, n:] == SENTINEL), "%s: a row at or beyond the count was written" % name
        assert np.all(tick.send_head.view(np.uint8).reshape(G, -1)[n:] == SENTINEL), "send_head: a row at or beyond the count was written"
        assert np.all(tick.send.view(np.uint8).reshape(F, G, -1)[:, n:] == SENTINEL), "send: a row at or beyond the count was written"
        assert np.all(tick.ready[n:G] == SENTINEL), "ready: a row at or beyond the count was written"
        flags = tick.row["flags"].reshape(RMAX, G)[:R, :n]
        assert not np.any(flags == 0xABABABAB), "a row below the count and the depth was not written"
    run(2, 0)
    run(RMAX, 1, given=100)                                      # above the greatest depth: clamped
    run(1, 2, given=0)                                           # below 1: clamped
    tick.close()
    for x in (gpu, orc, shadow):
        x.close()


# ---- automatic index bases across rounds --------------------------------------------------------------------------------------------------------------------
def auto_base_rounds_case(G, launches, seed, R=3, P=5, self_slot=1, fills=(1.0, 0.5, 0.25)):
    """sparse_tick_cases.auto_base_case's stream with R = 3 rounds per launch, through the tick: the table's bases equal a host mirror advanced with
    rg_index_base_advance32 on the multi-round list, no workgroup takes the 64-bit body, the rows equal the oracle's after unpack32 with the bases the launch
    STARTED with. A group may be wiped up to three times in one launch while its base stands still (the moves apply from the next launch), and once more before
    its next AppendEntries arrives: the wipes jump by 2^25 .. 2^26, so that everything stays within the window (2^28) of where the base will go."""
    st0, base = S.start_state(G, P, self_slot, seed)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    gpu.set_index_base(base)
    gpu.set_auto_index_base(S.WINDOW)
    gpu.load_state(st0)
    orc.load_state(st0)
    gpu.wide_body_workgroups(reset=True)
    tick = engine.Tick2(gpu, R, entry_cap=G * R, expired_cap=0, send=False, ready=False, sparse_cap=G, sparse_rounds=True)
    rng = np.random.default_rng(seed)
    mirror = base.copy()
    wiped = np.zeros(G, dtype=bool)
    flushes = late = 0
    for k in range(launches):
        pick = rng.random(G) < fills[k % len(fills)]
        pick[wiped] = True
        pick[int(rng.integers(0, G))] = True
        rows = np.flatnonzero(pick)
        start = orc.read_state()
        subs, outs = [], []
        for r in range(R):
            cur = orc.read_state()
            b = S.next_batch(cur, rng, P, self_slot, wipe=0.35, jump=(1 << 25, 1 << 26))
            fresh = S.refresh_batch(cur, wiped, P, self_slot, rng)
            redo = np.flatnonzero((fresh.head["hdr"] & 0xF) != abi.EV_NONE)
            b.head[redo], b.ab[redo], b.cd[redo] = fresh.head[redo], fresh.ab[redo], fresh.cd[redo]
            b.entry_terms, b.entry_count = fresh.entry_terms, fresh.entry_count
            sub = subset(b, rows)
            oo = orc.submit(sub, fill=0xAB)
            is_flush = (sub.head["hdr"] & 0xF) == abi.EV_LOG_FLUSH
            flushes += int(np.count_nonzero(is_flush))
            late += int(np.count_nonzero(is_flush)) if r > 0 else 0
            wiped[:] = False
            wiped[rows] = is_flush & (sub.ab["x"] > orc.read_state().last_index[rows]) & (abi.flags_status(oo.reply["flags"]) == abi.OK)
            subs.append(sub)
            outs.append(oo)
        batch = fuzz.concat_batches(subs)
        batch.gid = rows.astype(np.uint32)
        b32 = engine.pack32(batch, index_base=mirror)
        tick.refill(b32, [100 + 10 * k + r for r in range(R)])
        tick.launch()
        tick.wait()
        got, _ = engine.unpack32(tick.outcome32(), R, len(rows), start.role_epoch[rows], index_base=mirror[rows])      # (the rows speak the bases the launch started with)
        compare_outcomes(fuzz.concat_outcomes(outs), got, "automatic bases, launch %d" % k)
        want = S.advance(batch, mirror)
        engine.advance_index_base(b32, mirror, S.WINDOW)
        assert np.array_equal(mirror, want)
        wide_rows = mirror.copy()
        assert np.array_equal(engine.advance_index_base(batch, wide_rows, S.WINDOW), mirror)      # (rg_index_base_advance on the wide rows of the same list: no move left)
        assert np.array_equal(gpu.index_base(), mirror), "launch %d" % k
        assert gpu.wide_body_workgroups() == 0, "launch %d" % k
    compare_states(orc.read_state(), gpu.read_state(), "automatic bases final")
    assert flushes > 0 and late > 0 and np.count_nonzero(mirror != base) > 0
    tick.close()
    gpu.close()
    orc.close()
    return flushes, int(np.count_nonzero(mirror != base))


# ---- stale recordings ---------------------------------------------------------------------------------------------------------------------------------------
def stale_recording_case(G=64):
    """the handle of rg_tick2_create_sparse_rounds is an ordinary rg_tick2_t: refused after the table's options changed, refused after its index bases changed,
    and — its table gone — launch / wait answer -1 while destroy frees the handle. Nothing is launched by a refused call."""
    for change in ("option", "index base"):
        gpu = engine.Table(G, 3, 0, True)
        tick = engine.Tick2(gpu, 4, expired_cap=G, sparse_cap=G, sparse_rounds=True)
        tick.refill(abi.Batch(1, 0, gid=np.zeros(0, np.uint32)), [5, 6])
        tick.launch()
        tick.wait()
        before = gpu.read_state()
        if change == "option":
            gpu.set_option(abi.OPT_REQUIRE_FENCED_TIMEOUTS, 1)
        else:
            gpu.set_index_base(np.full(G, 1000, dtype=np.int64))
        with pytest.raises(engine.EngineError, match="changed after rg_tick2_create"):
            tick.launch()
        after = gpu.read_state()
        for f in before.fields():
            assert np.array_equal(getattr(before, f), getattr(after, f)), (change, f)
        tick.close()
        gpu.close()
    small = engine.Table(G, 3, 0, True)
    orphan = engine.Tick2(small, 4, expired_cap=G, sparse_cap=G, sparse_rounds=True)
    small.close()
    L = engine.lib()
    assert L.rg_tick2_launch(orphan._h) == -1 and L.rg_tick2_wait(orphan._h) == -1 and L.rg_tick2_destroy(orphan._h) == 0
    orphan._h = None                                             # (its page-locked columns went with the table's context: nothing to free through it any more)


# ---- both memspaces -----------------------------------------------------------------------------------------------------------------------------------------
def device_memspace_case(G=1000, P=5, R=3, seed=8, fill=0.3):
    """one stand-alone launch of R rounds with every column in device memory (RG_MEM_DEVICE: the list is trusted, nothing is staged) against the same call
    on host memory, two tables: the same rows, the same state — and the oracle's, where no row answered RG_NEED_HOST"""
    import ctypes as C
    self_slot = 2 % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    a, d, orc = engine.Table(G, P, self_slot, True), engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    for t in (a, d, orc):
        t.load_state(st0)
    fz = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False)
    rows = np.flatnonzero(np.random.default_rng(seed).random(G) < fill)
    n = len(rows)
    subs, outs = [], []
    for r in range(R):
        b = abi.Batch(1, G)
        fz.round(orc.read_state(), b, 0)
        subs.append(subset(b, rows))
        outs.append(orc.submit(subs[-1]))
    batch = fuzz.concat_batches(subs)
    batch.gid = rows.astype(np.uint32)
    b32 = engine.pack32(batch)
    host = a.submit32c_sparse_rounds(b32, wide=False)
    bufs = [engine.DeviceBuffer.from_host(d, x) for x in (b32.gid, b32.head, b32.abcd, b32.entry_terms[: max(b32.entry_count, 1)])]
    row, per = engine.DeviceBuffer.from_host(d, np.zeros(R * n, abi.OUT32_DT)), engine.DeviceBuffer.from_host(d, np.zeros(R * n, abi.PERSIST32_DT))
    cb, co = abi.CBatch32(), abi.COutcome32()
    cb.rounds, cb.count, cb.gid, cb.head, cb.abcd = R, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr
    cb.entry_terms, cb.entry_count = (bufs[3].ptr if b32.entry_count else None), b32.entry_count
    co.row, co.persist = row.ptr, per.ptr
    d._check(engine.lib().rg_submit32c_sparse_rounds(d._h, C.byref(cb), C.byref(co), abi.MEM_DEVICE))
    d.sync()
    dev = abi.Outcome32(R * n, wide=False)
    dev.row, dev.persist = row.to_host(abi.OUT32_DT, R * n), per.to_host(abi.PERSIST32_DT, R * n)
    _same_rows(dev, host, "RG_MEM_DEVICE vs RG_MEM_HOST")
    compare_states(a.read_state(), d.read_state(), "RG_MEM_DEVICE vs RG_MEM_HOST")
    got, _ = engine.unpack32(dev, R, n, st0.role_epoch[rows])
    if not np.any(got.status == abi.NEED_HOST):
        compare_outcomes(fuzz.concat_outcomes(outs), got, "RG_MEM_DEVICE")
        compare_states(orc.read_state(), d.read_state(), "RG_MEM_DEVICE")
    for x in bufs + [row, per]:
        x.free()
    for t in (a, d, orc):
        t.close()
    return n
