"""Cases for RG_OPT_COMPACT_ANY_CLUSTER (include/raftgpu.h): tables of 8 .. 15 nodes through the compact formats and the ticks. Shared by
tests/test_compact_large_cluster_gpu.py (an MI355X) and tests/devemu/emu_cases_compact_large_cluster.py (the host emulation of the kernels, small tables).

ROUTING. test_gpu_parity.route_through_compact stops at abi.MAX_COMPACT_CLUSTER nodes, so the cases bring a router of their own: routed(route) wraps
engine.Table.__init__ so that EVERY table of the block gets the option, and sends every hint-free batch that fits 32 bits through rg_submit32 (route
"submit32") or — dense batches — rg_submit32c ("submit32c"); a "-forced-wide" suffix sets RG_FORCE_WIDE=1 (the 64-bit body of the compact-row kernels). The raw
compact outcome rows are held to helpers.check_out32_rows and unpacked with engine.unpack32, as that function does. Rows that answer RG_NEED_HOST are repaired
through the hint protocol; hinted rows travel as wide rows, i.e. they are NOT decided by the kernels under test — hence the cap on them (lockstep_case).

Everything is held bit-exactly against tests/oracle_lib.OracleTable."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

from rafting_amd import abi, engine, workload
from tests import oracle_lib
from tests import sparse_rounds_cases as X
from tests import sparse_tick_cases as S
from tests import test_gpu_parity as T
from tests.helpers import check_out32_rows, compare_outcomes, compare_states, make_state, simple_log

ROUTES = ("submit32", "submit32c", "submit32-forced-wide", "submit32c-forced-wide")
SHAPES = ((9, 4, True, 61), (11, 10, False, 62), (15, 0, True, 63), (8, 7, True, 64))      # (cluster, self_slot, pre_vote, seed): test_gpu_parity's wide-row shapes


@contextlib.contextmanager
def routed(route=None, option=True):
    """inside the block: every engine.Table has RG_OPT_COMPACT_ANY_CLUSTER (option=True) and Table.submit takes the compact route named (None: untouched)"""
    init, wide_submit, saved = engine.Table.__init__, engine.Table.submit, os.environ.get("RG_FORCE_WIDE")

    def __init__(self, *a, **kw):
        init(self, *a, **kw)
        if option:
            self.set_compact_any_cluster(True)

    def submit(self, batch, out=None, fill=0):
        if batch.hint is None and abi.batch_fits_32(batch):
            if route.startswith("submit32c") and batch.gid is None:
                before = self.read_state()
                raw = self.submit32c(batch, fill=fill)
                got, _ = engine.unpack32(raw, batch.rounds, batch.count, before.role_epoch)
                check_out32_rows(raw, got, before, self.read_state(), batch.rounds, batch.count)
                if out is not None:
                    out.reply[:], out.logfx[:], out.persist[:] = got.reply, got.logfx, got.persist
                    return out
                return got
            return self.submit32(batch, out, fill)
        return wide_submit(self, batch, out, fill)
    engine.Table.__init__ = __init__
    if route is not None:
        assert route in ROUTES, route
        engine.Table.submit = submit
        if route.endswith("forced-wide"):
            os.environ["RG_FORCE_WIDE"] = "1"
        else:
            os.environ.pop("RG_FORCE_WIDE", None)
    try:
        yield
    finally:
        engine.Table.__init__, engine.Table.submit = init, wide_submit
        if saved is None:
            os.environ.pop("RG_FORCE_WIDE", None)
        else:
            os.environ["RG_FORCE_WIDE"] = saved


# ---- 1. lockstep fuzz ------------------------------------------------------------------------------------------------------------------------------------------
def lockstep_case(groups, rounds, cluster, self_slot, pre_vote, seed, route):
    """test_gpu_parity._lockstep (hints included) on a table above 7 nodes through one compact route: every outcome row and the final state equal the oracle's.
    RG_NEED_HOST rows are repaired as hinted WIDE rows, so they are not decided by the kernels under test: at most 2 % of all rows (the cap of
    tests/sparse_rounds_cases.py). The same four shapes through the wide-row route (the parent commit's kernels), 64 groups x 40 rounds on the emulation, miss
    4, 4, 5 and 4 of 2 560 rows (0.16 %, 0.16 %, 0.20 %, 0.16 %): every shape is below 1 %, the seeds stand as the wide-row test has them. (The miss count
    is a property of the stream and the four cached term runs, not of the route: every route decides the same rows on the same state.)
    -> (status histogram, misses, rows)"""
    with routed(route):
        _, _, _, hist, misses, gpu = T._lockstep(groups, cluster, self_slot, pre_vote, rounds, seed, allow_miss=True)
        seen = set(np.flatnonzero(hist).tolist())
        assert {abi.OK, abi.DROPPED_STALE_ROLE, abi.NOT_LEADER} <= seen, seen
        c = gpu.counters()
        assert c[0] > 0 and c[1] > 0 and c[2] > 0 and c[3] > 0, c
        rows = groups * rounds
        print("lockstep %s cluster %d: %d of %d rows repaired through the hint protocol (%.2f %%)" % (route, cluster, misses, rows, 100.0 * misses / rows))
        assert misses * 50 <= rows, "%d of %d rows were repaired as wide rows (cap: 2 %%)" % (misses, rows)
        gpu.close()
    return hist, misses, rows


# ---- 2. the 32-bit body really decides -------------------------------------------------------------------------------------------------------------------------
def body32_case(groups, cluster, rounds=16, at_two_to_the_forty=False):
    """config 3's stream at `cluster` nodes, `rounds` rounds in ONE device-resident launch through rg_submit32c: the oracle's rows, the rows of the same
    stream through wide-row rg_submit bit for bit, the same final state, and no workgroup on the 64-bit body. at_two_to_the_forty: every log compacted at
    2^40 (epoch.index = 2^40), index bases at 2^40 - 1, RG_OPT_AUTO_INDEX_BASE = 2^28 — again no workgroup on the 64-bit body."""
    kw = dict(cluster=cluster, name="config3 at %d nodes" % cluster)
    if at_two_to_the_forty:
        kw["index_base"] = 1 << 40
    cfg = dataclasses.replace(workload.config(3, groups), **kw)
    gen = workload.ReplayGenerator(cfg)
    st0 = gen.initial_state()
    b = gen.next_batch(rounds)
    base = np.full(groups, (1 << 40) - 1, dtype=np.int64) if at_two_to_the_forty else None
    with routed(None):
        gpu, wide = (engine.Table(groups, cfg.cluster, cfg.self_slot, cfg.pre_vote) for _ in range(2))
    orc = oracle_lib.OracleTable(groups, cfg.cluster, cfg.self_slot, cfg.pre_vote)
    if base is not None:
        assert np.all(st0.epoch_index >= 1 << 40)
        gpu.set_index_base(base)
        gpu.set_auto_index_base(1 << 28)
    for t in (gpu, wide, orc):
        t.load_state(st0)
    gpu.wide_body_workgroups(reset=True)
    ref = orc.submit(b)
    db = engine.DeviceBatch32(gpu, engine.pack32(b, index_base=base), compact=True)
    gpu.submit_device(db)
    gpu.sync()
    got, _ = engine.unpack32(db.outcome32(), db.rounds, db.count, st0.role_epoch, index_base=base)
    db.free()
    where = "config 3 at %d nodes%s" % (cluster, " and 2^40" if at_two_to_the_forty else "")
    compare_outcomes(ref, got, where)
    compare_states(orc.read_state(), gpu.read_state(), where)
    assert gpu.wide_body_workgroups() == 0, "%s: %d workgroups took the 64-bit body" % (where, gpu.wide_body_workgroups())
    w = wide.submit(b)                                        # (rg_submit: the wide-row kernels)
    compare_outcomes(w, got, where + " (wide rows)")          # (bit for bit, every field under the flag that makes it valid)
    compare_states(wide.read_state(), gpu.read_state(), where + " (wide rows)")
    dec = workload.batch_stats(b, cfg.cluster - 1)[0]
    assert dec > groups * rounds // 2
    for t in (gpu, wide, orc):
        t.close()
    return dec


# ---- 3. directed rows the 3-bit follower index would get wrong --------------------------------------------------------------------------------------------------
def _pair(P, self_slot, G, **kw):
    st = make_state(P, G, **kw)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    gpu.load_state(st)
    orc.load_state(st)
    return gpu, orc


def _row(gpu, orc, where, kind, **kw):
    """the same row for every group -> the oracle's outcome (the device's equals it, and so does the table)"""
    b = abi.Batch(1, gpu.groups)
    for g in range(gpu.groups):
        b.put(0, g, kind, **kw)
    og, oo = gpu.submit(b, fill=0xAB), orc.submit(b, fill=0xAB)
    compare_outcomes(oo, og, where)
    compare_states(orc.read_state(), gpu.read_state(), where)
    assert np.all(oo.status == oo.status[0]) and np.all(oo.reply["flags"] == oo.reply["flags"][0])
    return oo


def directed_case(self_slot, route, G=70, P=15):
    """A 15-node table, hand-built state, every group the same (70 groups: a full wavefront and a ragged one). Followers are indexed 0 .. 13 (slot, or
    slot - 1 above the own slot); the seven highest remote slots are followers 7 .. 13 whatever the own slot is — every one of them an index a 3-bit field
    truncates (8 .. 13), or its neighbour. Expected values: the oracle, side by side."""
    F = P - 1
    high = [s for s in range(P) if s != self_slot][-7:]                 # followers 7 .. 13
    follower = lambda s: s if s < self_slot else s - 1                  # noqa: E731
    assert [follower(s) for s in high] == list(range(7, 14))
    leader = dict(role=abi.LEADER, term=5, voted_for=self_slot, leader=abi.NO_NODE, repl_prepared=1, role_epoch=7, commit=10, log=simple_log(20, term=5))
    fresh = [(0, 21, 0, 0, 0)] * F
    with routed(route):
        # successful acks from followers 7 .. 13 in turn: majority() of 15 is 8, the leader itself and seven followers — the commit index moves exactly when the
        # seventh follower (the eighth node) has matched, not before
        gpu, orc = _pair(P, self_slot, G, peers=fresh, **leader)
        moved = []
        for s in high:
            oo = _row(gpu, orc, "ack from slot %d" % s, abi.EV_AE_ACK, slot=s, flag=1, a=5, b=0, c=20, aux=7)
            assert oo.status[0] == abi.OK
            moved.append(bool(oo.reply["flags"][0] & abi.F_COMMIT))
        assert moved == [False] * 6 + [True], moved
        st = gpu.read_state()
        assert np.all(st.commit_index == 20)
        m = st.peer_match_index.reshape(G, F)
        assert np.all(m[:, 7:] == 20) and np.all(m[:, :7] == 0)
        gpu.close()
        orc.close()
        # a rejecting ack from the highest slot before anything matched: Leadership.State.updateIndex backs nextIndex off (tier 1.5 of the 32-bit body)
        gpu, orc = _pair(P, self_slot, G, peers=fresh, **leader)
        oo = _row(gpu, orc, "rejecting ack from slot %d" % high[-1], abi.EV_AE_ACK, slot=high[-1], flag=0, a=5, b=0, c=20, aux=7)
        assert oo.status[0] == abi.OK
        st = gpu.read_state()
        nx, rj = st.peer_next_index.reshape(G, F), st.peer_rejection.reshape(G, F)
        assert np.all(nx[:, 13] < 21) and np.all(rj[:, 13] == 1) and np.all(nx[:, :13] == 21) and np.all(rj[:, :13] == 0)
        # ... and once more, twice: the back-off grows with the rejections, still at follower 13 only
        for k in range(2):
            _row(gpu, orc, "rejecting ack %d from slot %d" % (k + 2, high[-1]), abi.EV_AE_ACK, slot=high[-1], flag=0, a=5, b=0, c=20, aux=7)
        st = gpu.read_state()
        assert np.all(st.peer_rejection.reshape(G, F)[:, 13] == 3) and np.all(st.peer_rejection.reshape(G, F)[:, :13] == 0)
        gpu.close()
        orc.close()
        # an ack from the follower whose pending-installation bit is set, at follower index 13 (bit 13 of `pending`, shift 31 - 13 in the class word);
        # then the same ack from follower 12, whose bit is clear: it is applied
        pend = fresh[:13] + [(0, 21, 0, 0, 1)]
        gpu, orc = _pair(P, self_slot, G, peers=pend, **leader)
        _row(gpu, orc, "ack from a follower with a snapshot pending", abi.EV_AE_ACK, slot=high[-1], flag=1, a=5, b=0, c=20, aux=7)
        assert np.all(gpu.read_state().peer_match_index.reshape(G, F)[:, :13] == 0)      # (what the ack does to follower 13 is the oracle's to say; nobody else moved)
        _row(gpu, orc, "ack from the follower beside it", abi.EV_AE_ACK, slot=high[-2], flag=1, a=5, b=0, c=20, aux=7)
        assert np.all(gpu.read_state().peer_match_index.reshape(G, F)[:, 12] == 20)
        gpu.close()
        orc.close()
        # vote replies from the seven highest slots elect a Candidate at the eighth grant (its own vote + seven)
        cand = dict(role=abi.CANDIDATE, term=6, voted_for=self_slot, role_epoch=9, votes=1, commit=10, log=simple_log(20, term=5))
        gpu, orc = _pair(P, self_slot, G, **cand)
        roles = []
        for s in high:
            _row(gpu, orc, "vote from slot %d" % s, abi.EV_RV_REPLY, slot=s, flag=1, a=6, aux=9)
            roles.append(int(gpu.read_state().role[0]))
        assert roles == [abi.CANDIDATE] * 6 + [abi.LEADER], roles
        gpu.close()
        orc.close()


# ---- 4. lists of groups ----------------------------------------------------------------------------------------------------------------------------------------
def _embed(sub, G):
    """the dense batch that holds the rows of the list batch `sub` (R rounds, gid list) and RG_EV_NONE everywhere else"""
    R, n, rows = sub.rounds, sub.count, sub.gid.astype(np.int64)
    d = abi.Batch(R, G)
    d.head.reshape(R, G)[:, rows] = sub.head.reshape(R, n)
    d.ab.reshape(R, G)[:, rows] = sub.ab.reshape(R, n)
    d.cd.reshape(R, G)[:, rows] = sub.cd.reshape(R, n)
    d.entry_terms, d.entry_count = sub.entry_terms, sub.entry_count
    return d


def lists_case(G, P, seed, fills=(0.01, 0.25, 1.0), R=3):
    """rg_submit32c_sparse (one round) and rg_submit32c_sparse_rounds (R = 3) at three fills: the raw rows and the table equal those of the DENSE compact launch
    (rg_submit32c) of the same rows on a second table, and — after the host's repair of whatever answered RG_NEED_HOST — the oracle's. Led by the oracle, round
    by round (tests/sparse_rounds_cases.lead)."""
    fills_saved, depths_saved = X.FILLS, X.DEPTHS
    try:
        with routed(None):
            for depths in ((1,), (R,)):
                X.FILLS, X.DEPTHS = tuple(fills), depths
                gpu, orc, shadow, fz, rng, _ = X._tables(G, P, seed)
                dense = engine.Table(G, P, 2 % P, True)
                dense.load_state(gpu.read_state())
                fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
                listed = repaired = 0
                for k in range(2 * len(fills)):
                    t = X.lead(orc, fz, rng, G, k, fired_g, fired_e)
                    fired_g, fired_e = t.expired[0], t.expired[1]
                    if not t.n:
                        continue
                    assert t.R == depths[0]
                    where = "fill %.2f, %d rounds x %d rows" % (t.fill, t.R, t.n)
                    raw = gpu.submit32c_sparse(t.batch, fill=0xAB) if t.R == 1 else gpu.submit32c_sparse_rounds(t.batch, fill=0xAB)
                    full = dense.submit32c(_embed(t.batch, G), wide=False)
                    picked = abi.Outcome32(t.R * t.n, wide=False)
                    picked.row, picked.persist = full.row.reshape(t.R, G)[:, t.rows].reshape(-1), full.persist.reshape(t.R, G)[:, t.rows].reshape(-1)
                    X._same_rows(raw, picked, where + ": the list against the dense compact launch")
                    compare_states(dense.read_state(), gpu.read_state(), where + ": the list against the dense compact launch")
                    bad = X._check_rows(gpu, shadow, t, raw, where)
                    if len(bad):                              # (the dense table takes the same repair: the rows the list table just had repaired, as wide rows)
                        dense.load_state(gpu.read_state())
                    compare_states(orc.read_state(), gpu.read_state(), where)
                    listed += t.n
                    repaired += len(bad)
                assert listed > G, listed
                assert repaired * 50 <= listed, "%d of %d listed rows had to be repaired on the host (cap: 2 %%)" % (repaired, listed)
                for x in (gpu, orc, shadow, dense):
                    x.close()
    finally:
        X.FILLS, X.DEPTHS = fills_saved, depths_saved


# ---- 5. ticks --------------------------------------------------------------------------------------------------------------------------------------------------
def ticks_case(G, P, ticks, seed, device_resident=False):
    """The device-resident tick on a table above 7 nodes, three recordings, >= 50 ticks each, every tick held to the oracle (decisions, deadlines, health
    columns, fired tickets with epochs, the F-wide send table, readiness, the table): dense (test_gpu_parity.tick2_case: tick_kernel), a list of groups
    (sparse_tick_cases.sparse_tick_case: tick_sparse_kernel), a list of groups with a depth run below the depth it was recorded for
    (sparse_rounds_cases.rounds_tick_case)."""
    assert ticks >= 50
    with routed(None):
        T.tick2_case(G=G, P=P, ticks=ticks, seed=seed, device_resident=device_resident)
        S.sparse_tick_case(G, seed + 1, ticks, P=P, device_resident=device_resident, expect_all=False)
        X.rounds_tick_case(G, seed + 2, ticks, P=P, device_resident=device_resident, expect_all=False)


def tick_recordings_case(G, P, ticks, seed):
    """the other two recordings of the dense tick: step + tick_tail_kernel (RG_TICK_NODES=2) and the step-by-step one (4: timers_update32, health_update32, the
    expiry, replicate_kernel, ready_kernel — their health columns are [F][G])"""
    with routed(None):
        T.tick2_case(G=G, P=P, ticks=ticks, seed=seed, nodes=2)
        T.tick2_case(G=G, P=P, ticks=ticks, seed=seed + 1, nodes=4)


def tick_graph_case(G, P=9, ticks=24, seed=123):
    """rg_tick_create, the once-per-tick graph (upload, step kernel, list packing, download), on a 9-node table: tick after tick against the oracle's separate
    calls, dense and a sparse shape (test_gpu_parity.tick_path_case)"""
    with routed(None):
        T.tick_path_case(G=G, P=P, ticks=ticks, seed=seed)


# ---- 6. the option -----------------------------------------------------------------------------------------------------------------------------------------------
def _refused_everywhere(t):
    """every compact entry point and every tick constructor turns the table down with "wide rows"; nothing is launched"""
    G = t.groups
    before = t.read_state()
    dense, one = abi.Batch(1, G), abi.Batch(1, 1, gid=np.array([3], np.uint32))
    three = abi.Batch(3, 1, gid=np.array([3], np.uint32))
    refused = lambda: pytest.raises(engine.EngineError, match="wide rows")      # noqa: E731
    with refused():
        t.submit32(dense)
    with refused():
        t.submit32c(dense)
    with refused():
        t.submit32c_sparse(one)
    with refused():
        t.submit32c_sparse_rounds(three)
    pb = engine.PackedBatch(t, dense)
    with refused():
        t.submit_async_packed(pb)
    with refused():
        engine.Tick(t, pb)
    pb.free()
    for kw in (dict(), dict(sparse_cap=G), dict(sparse_cap=G, sparse_rounds=True)):
        with refused():
            engine.Tick2(t, 2 if kw.get("sparse_rounds") else 1, expired_cap=G, **kw)
    after = t.read_state()
    for f in before.fields():
        assert np.array_equal(getattr(before, f), getattr(after, f)), f


def option_off_by_default_case(G=64, P=9):
    t = engine.Table(G, P, 4, True)
    _refused_everywhere(t)
    t.submit(abi.Batch(1, G))                                 # (wide rows: as ever)
    t.close()


def option_values_case(G=64, P=9, launch=True):
    """2 and -1 give -1 with a message and change nothing; 1 lifts the limit (launch=True: and the entry points then decide); 0 after 1 restores the refusals"""
    L = engine.lib()
    t = engine.Table(G, P, 4, True)
    for bad in (2, -1):
        assert L.rg_table_option(t._h, abi.OPT_COMPACT_ANY_CLUSTER, bad) == -1
        assert b"RG_OPT_COMPACT_ANY_CLUSTER" in L.rg_last_error(t._h)
        _refused_everywhere(t)
    t.set_compact_any_cluster(True)
    dense = abi.Batch(1, G)
    if launch:
        t.submit32(dense)
        t.submit32c(dense)
        t.submit32c_sparse(abi.Batch(1, 1, gid=np.array([3], np.uint32)))
        t.submit32c_sparse_rounds(abi.Batch(3, 1, gid=np.array([3], np.uint32)))
    assert L.rg_table_option(t._h, abi.OPT_COMPACT_ANY_CLUSTER, 2) == -1      # (a bad value leaves the option as it was)
    if launch:
        t.submit32(dense)
    else:                                                     # (the constructors get past the cluster check: what they refuse next is something else)
        with pytest.raises(engine.EngineError, match="rows for"):
            t.submit32c_sparse(abi.Batch(1, G + 1, gid=np.arange(G + 1, dtype=np.uint32)))
    t.set_compact_any_cluster(False)
    _refused_everywhere(t)
    t.close()


def option_recorded_tick_case(G=64, P=9):
    """a Tick2 recorded with the option on refuses to launch once it is switched off (config_gen), and launches nothing; switched on again the table has moved
    on all the same: a recording belongs to the configuration it was made under"""
    t = engine.Table(G, P, 4, True)
    t.set_compact_any_cluster(True)
    tick = engine.Tick2(t, 1, expired_cap=G)
    tick.refill(abi.Batch(1, G), [5])
    tick.launch()
    tick.wait()
    before = t.read_state()
    t.set_compact_any_cluster(False)
    with pytest.raises(engine.EngineError, match="changed after rg_tick2_create"):
        tick.launch()
    after = t.read_state()
    for f in before.fields():
        assert np.array_equal(getattr(before, f), getattr(after, f)), f
    t.set_compact_any_cluster(True)
    with pytest.raises(engine.EngineError, match="changed after rg_tick2_create"):
        tick.launch()
    again = engine.Tick2(t, 1, expired_cap=G)                 # (a new recording under the new configuration runs)
    again.refill(abi.Batch(1, G), [6])
    again.launch()
    again.wait()
    for x in (tick, again):
        x.close()
    t.close()


def option_small_cluster_case(G, rounds, P=5, self_slot=2, seed=12):
    """a 5-node table decides a fuzz stream bit-identically with the option on and off: the same outcome rows (both equal the oracle's, row for row, inside
    _lockstep) and the same final state, through rg_submit32 and rg_submit32c"""
    for route in ("submit32", "submit32c"):
        finals = []
        for on in (False, True):
            with routed(route, option=on):
                _, _, outs, hist, misses, gpu = T._lockstep(G, P, self_slot, True, rounds, seed, allow_miss=True)
                finals.append((gpu.read_state(), outs, misses, gpu.wide_body_workgroups()))
                gpu.close()
        (sa, oa, ma, wa), (sb, ob, mb, wb) = finals
        for f in sa.fields():
            assert np.array_equal(getattr(sa, f), getattr(sb, f)), (route, f)
        assert ma == mb and wa == wb and len(oa) == len(ob)
        for x, y in zip(oa, ob):
            assert np.array_equal(x.reply, y.reply) and np.array_equal(x.logfx, y.logfx) and np.array_equal(x.persist, y.persist), route
