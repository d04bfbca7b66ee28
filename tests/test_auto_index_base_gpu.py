"""RG_OPT_AUTO_INDEX_BASE on the MI355X: the stream of tests/auto_base_stream.py (long-lived groups carried forward by LOG_FLUSH rows) through every
submission path — wide rows, compact rows, compact outcome rows, the pipelined packed path, a multi-round device-memory launch, recorded ticks — against
the oracle on the absolute stream, with the table's bases equal to the host's mirror (rg_index_base_advance*) after every launch."""

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import auto_base_stream as S
from tests import fuzz, oracle_lib
from tests.helpers import compare_outcomes, compare_states

pytestmark = pytest.mark.gpu

G, P, SELF = 1024, 5, 1


def _pair(seed, window=S.WINDOW, G=G):
    st0, base = S.start_state(G, P, SELF, seed)
    gpu, orc = engine.Table(G, P, SELF, True), oracle_lib.OracleTable(G, P, SELF, True)
    gpu.set_index_base(base)
    if window:
        gpu.set_auto_index_base(window)
    gpu.load_state(st0)
    orc.load_state(st0)
    gpu.wide_body_workgroups(reset=True)
    return st0, base.copy(), gpu, orc


def _finish(gpu, orc, where):
    compare_states(orc.read_state(), gpu.read_state(), where)
    gpu.close()
    orc.close()


@pytest.mark.parametrize("route", ["submit", "async", "submit32", "submit32c", "async_packed", "tick"])
def test_every_route_moves_the_bases_like_the_mirror(route):
    st0, mirror, gpu, orc = _pair(seed=41)
    rng = np.random.default_rng(41)
    tick = pbt = None
    for k in range(10):
        b, ref, cur = S.launch(orc, rng, P, SELF)
        where = "%s, launch %d" % (route, k)
        if route in ("submit", "async"):                       # wide rows: absolute a
            if route == "submit":
                got = gpu.submit(b, fill=0xAB)
            else:                                              # rg_submit_async: the pipelined host-memory path
                got = abi.Outcome(b.rounds * b.count)
                gpu.submit_async(b, got)
                gpu.submit_wait()
            compare_outcomes(ref, got, where)
            engine.advance_index_base(b, mirror, S.WINDOW)
        else:
            b32 = engine.pack32(b, index_base=mirror)
            if route == "submit32":
                got = gpu.submit32(b32, fill=0xAB)
            elif route == "submit32c":
                got, _ = engine.unpack32(gpu.submit32c(b32, fill=0xAB), b.rounds, G, cur.role_epoch, index_base=mirror)
            elif route == "async_packed":
                pb = engine.PackedBatch(gpu, S.relative(b, mirror))
                gpu.submit_async_packed(pb)
                gpu.submit_wait()
                got = pb.unpack()
                pb.free()
            else:                                              # rg_tick_*: one recording, replayed with the rows of every launch
                if tick is None:
                    pbt = engine.PackedBatch(gpu, S.relative(b, mirror), entry_cap=G)
                    tick = engine.Tick(gpu, pbt)
                tick.refill(S.relative(b, mirror))
                tick.launch()
                tick.wait()
                got = pbt.unpack()
            compare_outcomes(ref, got, where)
            engine.advance_index_base(b32, mirror, S.WINDOW)
        assert np.array_equal(gpu.index_base(), mirror), where
        if route not in ("submit", "async"):
            assert gpu.wide_body_workgroups() == 0, where
    if tick is not None:
        tick.close()
        pbt.free()
    assert np.count_nonzero(mirror != S.OFFSET - 1000) > G // 2
    _finish(gpu, orc, route)


def test_a_multi_round_device_memory_launch():
    """eight launches' worth of rows in ONE launch (RG_MEM_DEVICE, compact rows, compact outcome rows): every row relative to the bases the launch started
    with, the new bases from all of its LOG_FLUSH rows (two wipes of a group in one launch: the larger one counts). Smaller jumps so that eight rounds of
    them stay in the 32-bit image of the starting base."""
    st0, mirror, gpu, orc = _pair(seed=42)
    rng = np.random.default_rng(42)
    for k in range(3):
        parts = [S.launch(orc, rng, P, SELF, jump=(1 << 24, 1 << 26)) for _ in range(4)]
        b, ref = _stack([x[0] for x in parts]), fuzz.concat_outcomes([x[1] for x in parts])
        cur = parts[0][2]
        db = engine.DeviceBatch32(gpu, engine.pack32(b, index_base=mirror), compact=True)
        gpu.submit_device(db)
        gpu.sync()
        got, _ = engine.unpack32(db.outcome32(), db.rounds, db.count, cur.role_epoch, index_base=mirror)
        db.free()
        compare_outcomes(ref, got, "multi-round launch %d" % k)
        engine.advance_index_base(b, mirror, S.WINDOW)
        assert np.array_equal(gpu.index_base(), mirror)
        assert gpu.wide_body_workgroups() == 0
    _finish(gpu, orc, "multi-round")


def test_recorded_ticks_move_the_bases_and_a_tick_recorded_before_the_option_refuses():
    st0, mirror, gpu, orc = _pair(seed=43, window=0)
    stale = engine.Tick2(gpu, 2, entry_cap=0, send=False, ready=False, expired_cap=0)
    gpu.set_auto_index_base(S.WINDOW)
    stale.refill(abi.Batch(2, G), [1, 2], index_base=mirror)
    with pytest.raises(engine.EngineError):
        stale.launch()                                        # recorded before the option: refused (-1)
    stale.close()
    tick = engine.Tick2(gpu, 2, entry_cap=0, send=False, ready=False, expired_cap=0)
    rng = np.random.default_rng(43)
    for k in range(8):
        b, ref, cur = S.launch(orc, rng, P, SELF)
        tick.refill(b, [10 * k + 1, 10 * k + 2], index_base=mirror)
        tick.launch()
        tick.wait()
        got, _ = engine.unpack32(tick.outcome32(), 2, G, cur.role_epoch, index_base=mirror)
        compare_outcomes(ref, got, "tick %d" % k)
        engine.advance_index_base(b, mirror, S.WINDOW)
        assert np.array_equal(gpu.index_base(), mirror), "tick %d" % k
        assert gpu.wide_body_workgroups() == 0
    tick.close()
    _finish(gpu, orc, "ticks")


def _with_long_logs(st, groups, leader, runs=6, span=5):
    """`st` with the logs of `groups` made of more term runs than the table caches (RG_TERM_RUNS): Followers of `leader` at term runs + 2 whose log
    holds `runs` runs of `span` entries above the epoch — an AppendEntries whose prevLogIndex lies in the oldest runs misses the cache (RG_NEED_HOST)"""
    G, K = st.count, abi.TERM_RUNS
    out = abi.GroupState(G, st.cluster, runs_total=G * K + runs * len(groups))
    for name, _, shape in abi._STATE_FIELDS:
        if shape != "runs":
            getattr(out, name)[:] = getattr(st, name)
    out.run_start[:G * K], out.run_term[:G * K] = st.run_start, st.run_term
    out.run_offset[:] = np.arange(G, dtype=np.uint32) * K
    pos = G * K
    for g in groups:
        ei = int(st.epoch_index[g])
        out.role[g], out.current_term[g], out.current_leader[g], out.voted_for[g] = abi.FOLLOWER, runs + 2, leader, abi.NO_NODE
        out.repl_prepared[g], out.timeout_detected[g], out.epoch_term[g], out.commit_index[g] = 0, 0, 1, ei
        for k in range(runs):
            out.run_start[pos + k], out.run_term[pos + k] = ei + 1 + span * k, k + 1
        out.run_offset[g], out.run_count[g] = pos, runs
        out.first_index[g], out.last_index[g] = ei + 1, ei + span * runs
        pos += runs
    return out


def test_flushes_behind_a_need_host_move_the_base_on_the_compact_path():
    """Two groups whose AppendEntries misses the term cache (RG_NEED_HOST) in round 0 of a compact launch (rg_submit32c) and whose LOG_FLUSH follows in
    round 1 (RG_SKIPPED_AFTER_NEED_HOST): both bases move all the same. Group 5's flush lies inside the 32-bit image (the 32-bit body counts it on a skipped
    row); group 130's lies 2^30 or more above its base — a skipped row outside the domain, whose workgroup (and only it) the 64-bit body redoes and counts.
    Then the host repairs the two groups' rows (the AppendEntries with the term of its prevLogIndex as a hint, the flush again: max is idempotent) and
    every outcome row and the final state equal the oracle's on the original batch."""
    Gs, leader = 256, 0
    st0, base = S.start_state(Gs, P, SELF, seed=44)
    g1, g2 = 5, 130
    st0 = _with_long_logs(st0, (g1, g2), leader)
    gpu, orc = engine.Table(Gs, P, SELF, True), oracle_lib.OracleTable(Gs, P, SELF, True)
    gpu.set_index_base(base)
    gpu.set_auto_index_base(S.WINDOW)
    gpu.load_state(st0)
    orc.load_state(st0)
    gpu.wide_body_workgroups(reset=True)
    mirror = base.copy()
    b = abi.Batch(2, Gs)
    flush_at = {g1: int(st0.last_index[g1]) + S.WINDOW + 100, g2: int(base[g2]) + (1 << 30) + 12345}
    for g in (g1, g2):
        b.head["hdr"][g] = abi.hdr_make(abi.EV_AE_REQ, slot=leader)
        b.ab["x"][g], b.ab["y"][g] = int(st0.current_term[g]), int(st0.first_index[g]) + 1      # prevLogIndex in the oldest (uncached) run, term 1
        b.cd["x"][g], b.cd["y"][g] = 1, 0
        b.head["hdr"][Gs + g] = abi.hdr_make(abi.EV_LOG_FLUSH)
        b.ab["x"][Gs + g], b.ab["y"][Gs + g] = flush_at[g], int(st0.current_term[g])
    ref = orc.submit(b, fill=0xAB)
    b32 = engine.pack32(b, index_base=mirror)
    got, _ = engine.unpack32(gpu.submit32c(b32, fill=0xAB), 2, Gs, st0.role_epoch, index_base=mirror)
    engine.advance_index_base(b32, mirror, S.WINDOW)
    for g in (g1, g2):
        assert got.status[g] == abi.NEED_HOST and got.status[Gs + g] == abi.SKIPPED_AFTER_NEED_HOST, g
        assert mirror[g] == flush_at[g] - S.WINDOW
    assert np.array_equal(gpu.index_base(), mirror)
    assert gpu.wide_body_workgroups() == 1                 # group 130's workgroup only
    # the host's half: the missing term from its log, the two groups' rows again (wide rows: hints travel there)
    rep = abi.Batch(2, Gs, hints=True)
    for g in (g1, g2):
        for r in (0, 1):
            row = r * Gs + g
            rep.head[row], rep.ab[row], rep.cd[row] = b.head[row], b.ab[row], b.cd[row]
        rep.set_hint(g, orc_term(st0, g, int(b.ab["y"][g])), 0)
    o2 = gpu.submit(rep, fill=0xAB)
    engine.advance_index_base(rep, mirror, S.WINDOW)
    assert np.array_equal(gpu.index_base(), mirror)
    for g in (g1, g2):
        for r in (0, 1):
            row = r * Gs + g
            got.reply[row], got.logfx[row], got.persist[row] = o2.reply[row], o2.logfx[row], o2.persist[row]
    compare_outcomes(ref, got, "repaired rows")
    _finish(gpu, orc, "repaired rows")


def orc_term(st, g, idx):
    """the term of index idx in group g's log as `st` holds it (the host's RaftLog)"""
    off, n = int(st.run_offset[g]), int(st.run_count[g])
    starts, terms = st.run_start[off:off + n], st.run_term[off:off + n]
    return int(terms[np.searchsorted(starts, idx, side="right") - 1])


def test_forced_wide_and_a_launch_that_leaves_the_32_bit_body_give_the_mirror(monkeypatch):
    """the 64-bit body applies the same rule: RG_FORCE_WIDE=1 (every compact launch on it) and a launch whose workgroup bails mid-way (a term >= 2^30)"""
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    st0, mirror, gpu, orc = _pair(seed=45, G=256)
    monkeypatch.delenv("RG_FORCE_WIDE")
    rng = np.random.default_rng(45)
    for k in range(4):
        b, ref, cur = S.launch(orc, rng, P, SELF)
        got, _ = engine.unpack32(gpu.submit32c(engine.pack32(b, index_base=mirror), fill=0xAB), b.rounds, 256, cur.role_epoch, index_base=mirror)
        compare_outcomes(ref, got, "forced wide, launch %d" % k)
        engine.advance_index_base(b, mirror, S.WINDOW)
        assert np.array_equal(gpu.index_base(), mirror)
    assert gpu.wide_body_workgroups() > 0
    _finish(gpu, orc, "forced wide")
    st0, mirror, gpu, orc = _pair(seed=46, G=256)
    rng = np.random.default_rng(46)
    b, ref, cur = S.launch(orc, rng, P, SELF)
    gpu.submit32c(engine.pack32(b, index_base=mirror))
    engine.advance_index_base(b, mirror, S.WINDOW)
    b, ref, cur = S.launch(orc, rng, P, SELF)
    # a RequestVote with a term of 2^30 in round 1 of group 3: its workgroup leaves the 32-bit body after round 0 and is decided again in 64-bit
    b2 = _stack([b, abi.Batch(1, 256)])
    b2.head["hdr"][512 + 3] = abi.hdr_make(abi.EV_RV_REQ, slot=0)
    b2.ab["x"][512 + 3], b2.ab["y"][512 + 3] = 1 << 30, int(orc.read_state().last_index[3]) or int(orc.read_state().epoch_index[3])
    orc2_out = orc.submit(_round(b2, 2), fill=0xAB)
    ref2 = fuzz.concat_outcomes([ref, orc2_out])
    got, _ = engine.unpack32(gpu.submit32c(engine.pack32(b2, index_base=mirror), fill=0xAB), 3, 256, cur.role_epoch, index_base=mirror)
    compare_outcomes(ref2, got, "bail mid-way")
    engine.advance_index_base(b2, mirror, S.WINDOW)
    assert np.array_equal(gpu.index_base(), mirror)
    assert gpu.wide_body_workgroups() >= 1
    _finish(gpu, orc, "bail mid-way")


def _stack(batches):
    """dense batches of any number of rounds, one after the other, as one batch"""
    return fuzz.concat_batches([_round(b, r) for b in batches for r in range(b.rounds)])


def _round(b, r):
    """round r of a dense batch as a batch of its own"""
    out = abi.Batch(1, b.count)
    s = slice(r * b.count, (r + 1) * b.count)
    out.head[:], out.ab[:], out.cd[:] = b.head[s], b.ab[s], b.cd[s]
    out.entry_terms, out.entry_count = b.entry_terms, b.entry_count
    return out


def test_control_without_the_option_the_stream_leaves_the_32_bit_body():
    """CONTROL (passes without the feature; it documents the cliff): the same stream with the host never moving the bases — rows that the format can
    still carry relative to the starting bases go compact, and the groups' workgroups end up on the 64-bit body"""
    st0, base, gpu, orc = _pair(seed=47, window=0, G=256)
    rng = np.random.default_rng(47)
    for k in range(3):                                    # (two wipes of a group take it past 2^30 above its base; three still pack below 2^31)
        b, ref, cur = S.launch(orc, rng, P, SELF, wipe=0.5, jump=(1 << 29, (1 << 29) + (1 << 27)))
        got, _ = engine.unpack32(gpu.submit32c(engine.pack32(b, index_base=base), fill=0xAB), b.rounds, 256, cur.role_epoch, index_base=base)
        compare_outcomes(ref, got, "control, launch %d" % k)
    assert np.array_equal(gpu.index_base(), base)
    assert gpu.wide_body_workgroups() > 0
    _finish(gpu, orc, "control")
