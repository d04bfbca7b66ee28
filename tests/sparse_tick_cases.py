"""Cases for the sparse forms of the compact-row path: rg_submit32c_sparse (compact rows of a LIST of groups in, compact outcome rows out) and the sparse
device-resident tick (rg_tick2_create_sparse). Shared by tests/test_sparse_tick_gpu.py (an MI355X) and tests/devemu/emu_cases_sparse_tick.py (the host
emulation of the kernels, small tables); everything is held bit-exactly against tests/oracle_lib.OracleTable, which takes gid lists in submit,
timers_update and replicate."""
import types

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import auto_base_stream as S
from tests import clock
from tests import fuzz, oracle_lib
from tests import test_gpu_parity as T
from tests.helpers import check_out32_rows, compare_outcomes, compare_states


def subset(b, rows):
    """the single-round sparse batch that holds rows `rows` (= group ids, ascending) of the dense single-round batch b; no hint column"""
    rows = np.asarray(rows, dtype=np.int64)
    s = abi.Batch(1, len(rows), gid=rows.astype(np.uint32))
    s.head[:], s.ab[:], s.cd[:] = b.head[rows], b.ab[rows], b.cd[rows]
    s.entry_terms, s.entry_count = b.entry_terms, b.entry_count          # (aux offsets stay what they were)
    return s


def repair_need_host(gpu, orc, b, rows, got, cur):
    """the host half of the NEED_HOST protocol for the listed rows (test_gpu_parity._resolve_need_host works on dense rows: scatter, repair, gather)"""
    full = abi.Outcome(b.count)
    full.reply[rows], full.logfx[rows], full.persist[rows] = got.reply, got.logfx, got.persist
    n = T._resolve_need_host(gpu, orc, b, full, cur)
    got.reply[:], got.logfx[:], got.persist[:] = full.reply[rows], full.logfx[rows], full.persist[rows]
    return n


def assert_untouched(before, after, outside, where):
    """groups outside the list keep their state bit for bit"""
    G, F, K = before.count, before.followers, abi.TERM_RUNS
    for name, _, shape in abi._STATE_FIELDS:
        if name == "run_offset":
            continue
        a, b = getattr(before, name), getattr(after, name)
        per = 1 if shape == 1 else (K if shape == "runs" else F)
        m = np.repeat(outside, per)
        assert np.array_equal(a.reshape(-1)[: G * per][m], b.reshape(-1)[: G * per][m]), "%s: %s of a group outside the list changed" % (where, name)


def standalone_case(G, P, rounds, seed, fills=(1.0, 0.5, 0.1, 0.01)):
    """rg_submit32c_sparse in lockstep with the oracle (as test_gpu_parity._lockstep): every round keeps a random subset of the fuzzer's dense round"""
    self_slot = seed % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    gpu.load_state(st0)
    orc.load_state(st0)
    fz = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False)
    rng = np.random.default_rng(seed)
    ragged = full = repaired = 0
    hist = np.zeros(256, dtype=np.int64)
    for r in range(rounds):
        cur = gpu.read_state()
        b = abi.Batch(1, G)
        fz.round(cur, b, 0)
        fill = fills[r % len(fills)]
        pick = rng.random(G) < fill
        pick[int(rng.integers(0, G))] = True                 # (never an empty list: rg_submit32c_sparse with no rows launches nothing)
        rows = np.flatnonzero(pick)
        n = len(rows)
        ragged += n % 64 != 0
        full += n == G
        sub = subset(b, rows)
        raw = gpu.submit32c_sparse(sub, fill=0xAB)
        after = gpu.read_state()
        got, _ = engine.unpack32(raw, 1, n, cur.role_epoch[rows])
        if not np.any(got.status == abi.NEED_HOST):
            check_out32_rows(raw, got, types.SimpleNamespace(commit_index=cur.commit_index[rows], role_epoch=cur.role_epoch[rows]),
                             types.SimpleNamespace(commit_index=after.commit_index[rows], role_epoch=after.role_epoch[rows]), 1, n)
        assert_untouched(cur, after, ~pick, "round %d" % r)
        repaired += repair_need_host(gpu, orc, b, rows, got, cur)
        oo = orc.submit(sub, fill=0xAB)
        compare_outcomes(oo, got, "round %d (%d rows)" % (r, n))
        hist += np.bincount(oo.status, minlength=256)
        compare_states(orc.read_state(), gpu.read_state(), "round %d" % r)
    assert ragged > 0 and hist[abi.OK] > 0
    gpu.close()
    orc.close()
    return hist, full, repaired


FILLS = (0.0, 0.01, 0.1, 0.5, 1.0)


def sparse_tick_case(G, seed, ticks, P=5, device_resident=False, capacity=None, expect_all=True):
    """test_gpu_parity.tick2_case's loop through the SPARSE tick: tick k has fill FILLS[k % 5]; its list = a random subset at that fill + the groups whose
    ticket fired in tick k - 1 (their TIMEOUT rows carry the reported epochs); a fill-0 tick submits nothing and the timeouts due in it are lost.
    -> (rows seen, rows left out of the send / readiness comparison because their tick repaired an RG_NEED_HOST row)"""
    self_slot = 2 % P
    cap = G if capacity is None else capacity
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    fz = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False)
    for t in (gpu, orc):
        t.load_state(st0)
        t.timers_configure(900, 300, 4321)
        t.timers_arm(clock.origin())
    tick = engine.Tick2(gpu, 1, entry_cap=8 * G, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=cap)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    rng = np.random.default_rng(seed)
    seen = dict(empty_with_fired=0, full=0, ragged=0, conversion=0, append=0, ready0=0, ready1=0)
    all_rows = left_out = 0
    for k in range(ticks):
        now = clock.origin() + 150 * k
        fill = FILLS[k % len(FILLS)]
        cur = gpu.read_state()
        b = abi.Batch(1, G)
        fz.round(cur, b, 0)
        pick = np.zeros(G, dtype=bool)
        if fill > 0:
            pick = rng.random(G) < fill
            for g, e in zip(fired_g, fired_e):              # the tickets that fired at the end of the previous tick: their onTimeout, fenced
                b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
                pick[int(g)] = True
        rows = np.flatnonzero(pick)
        assert len(rows) <= cap
        n = len(rows)
        sub = subset(b, rows)
        assert abi.batch_fits_32(sub)
        hb = (rng.random(n) < 0.5).astype(np.uint8)
        fl = rng.integers(0, 24, (n, P - 1)).astype(np.uint16)
        tick.refill(sub, [now], heartbeat=hb, in_flight=fl.T.reshape(-1))
        tick.launch()
        tick.wait()
        bad = np.zeros(0, dtype=np.int64)
        if n:
            got, _ = engine.unpack32(tick.outcome32(), 1, n, cur.role_epoch[rows])
            bad = np.flatnonzero(got.status == abi.NEED_HOST)
            if len(bad):                                    # (as tick2_case: repaired on the host, folded like the others, left out of this tick's send / readiness comparison)
                repair_need_host(gpu, orc, b, rows, got, cur)
                gpu.timers_update(1, len(bad), got.reply[bad], [now], gid=rows[bad].astype(np.uint32))
                gpu.health_update(subset(b, rows[bad]), got.reply[bad], [now])
            oo = orc.submit(sub, now=[now])
            compare_outcomes(oo, got, "tick %d (%d rows)" % (k, n))
            orc.timers_update(1, n, oo.reply, [now], gid=rows.astype(np.uint32))
            seen["conversion"] += int(np.count_nonzero(oo.reply["flags"] & abi.F_ROLE_CHANGED))
        eo, epo, no = orc.timers_expired_epochs(now, capacity=G)
        eg, epg, ng = tick.expired()
        assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo), k
        assert np.array_equal(gpu.timers_read(), orc.timers_read()), k
        for a, c in zip(gpu.health_read(), orc.health_read()):
            assert np.array_equal(a, c), k
        if n:
            ok = np.ones(n, dtype=bool)
            ok[bad] = False
            (hg, sg), (ho, so) = tick.sends(), orc.replicate(gid=rows.astype(np.uint32), heartbeat=hb, in_flight=fl)
            if len(bad):
                gpu.replicate(gid=rows[bad].astype(np.uint32), heartbeat=hb[bad], in_flight=fl[bad])     # (prepareReplication of a repaired leader, as the oracle just ran it)
            for f in ("term", "leader_commit", "epoch_index", "epoch_term", "role_epoch", "is_leader"):
                assert np.array_equal(hg[f][ok], ho[f][ok]), (k, f)
            for f in ("prev_index", "prev_term", "last_index", "count", "kind"):
                assert np.array_equal(sg[f][ok], so[f][ok]), (k, f)
            rd, ro = tick.readiness(), orc.ready(now, 1, 60)[rows]
            assert np.array_equal(rd[ok], ro[ok]), k
            seen["append"] += int(np.count_nonzero(so["kind"] == abi.SEND_APPEND))
            seen["ready0"] += int(np.count_nonzero(ro == 0))
            seen["ready1"] += int(np.count_nonzero(ro == 1))
        compare_states(orc.read_state(), gpu.read_state(), "tick %d" % k)
        seen["empty_with_fired"] += n == 0 and ng > 0
        seen["full"] += n == cap
        seen["ragged"] += n % 64 != 0
        all_rows += n
        left_out += len(bad)
        fired_g, fired_e = eg, epg
    if expect_all:
        assert all(v > 0 for v in seen.values()), seen
    assert left_out * 50 <= all_rows, "%d of %d rows were left out of the send / readiness comparison (cap: 2 %%)" % (left_out, all_rows)
    # a recording is refused once the table's options have moved on, as the dense one is
    gpu.set_option(abi.OPT_REQUIRE_FENCED_TIMEOUTS, 1)
    with pytest.raises(engine.EngineError):
        tick.launch()
    tick.close()
    gpu.close()
    orc.close()
    return all_rows, left_out


def same_as_dense_case(G, ticks=20, seed=9, P=5, device_resident=False):
    """one stream at fill 1.0 with gid = arange(G) through the sparse tick on one table and through the dense tick on another: every output column and the
    final state are identical"""
    self_slot = 2 % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    a, d = engine.Table(G, P, self_slot, True), engine.Table(G, P, self_slot, True)
    fz = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False)
    for t in (a, d):
        t.load_state(st0)
        t.timers_configure(900, 300, 99)
        t.timers_arm(clock.origin())
    kw = dict(entry_cap=8 * G, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident)
    ta, td = engine.Tick2(a, 1, sparse_cap=G, **kw), engine.Tick2(d, 1, **kw)
    rng = np.random.default_rng(seed)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    every = np.arange(G)
    for k in range(ticks):
        now = clock.origin() + 150 * k
        b = abi.Batch(1, G)
        fz.round(a.read_state(), b, 0)
        for g, e in zip(fired_g, fired_e):
            b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
        hb = (rng.random(G) < 0.5).astype(np.uint8)
        fl = rng.integers(0, 24, (G, P - 1)).astype(np.uint16)
        ta.refill(subset(b, every), [now], heartbeat=hb, in_flight=fl.T.reshape(-1))
        td.refill(b, [now], heartbeat=hb, in_flight=fl.T.reshape(-1))
        for t in (ta, td):
            t.launch()
            t.wait()
        ra, rd = ta.outcome32(), td.outcome32()
        flags = rd.row["flags"]
        for f in ("resp_term", "flags", "commit_index"):
            assert np.array_equal(ra.row[f], rd.row[f]), (k, f)
        lf = ((flags & (abi.F_LOG_APPEND | abi.F_LOG_TRUNC)) != 0) | (abi.flags_status(flags) == abi.NEED_HOST)      # (log_from is defined under these marks only)
        assert np.array_equal(ra.row["log_from"][lf], rd.row["log_from"][lf]), k
        per = (flags & abi.F_PERSIST) != 0
        assert np.array_equal(ra.persist[per], rd.persist[per]), k
        ea, ed = ta.expired(), td.expired()
        assert ea[2] == ed[2] and np.array_equal(ea[0], ed[0]) and np.array_equal(ea[1], ed[1]), k
        (ha, sa), (hd, sd) = ta.sends(), td.sends()
        assert np.array_equal(ha, hd) and np.array_equal(sa, sd), k
        assert np.array_equal(ta.readiness(), td.readiness()), k
        assert np.array_equal(a.timers_read(), d.timers_read()), k
        for x, y in zip(a.health_read(), d.health_read()):
            assert np.array_equal(x, y), k
        fired_g, fired_e = ed[0], ed[1]
    compare_states(d.read_state(), a.read_state(), "sparse tick with every group listed vs the dense tick")
    for t in (ta, td):
        t.close()
    a.close()
    d.close()


def auto_base_case(G, ticks, seed, P=5, self_slot=1, fills=(1.0, 0.5, 0.25)):
    """RG_OPT_AUTO_INDEX_BASE (window 2^28) with LOG_FLUSH rows arriving in sparse ticks, groups at 2^40: the table's bases equal a host mirror advanced with
    rg_index_base_advance32 tick by tick, no workgroup takes the 64-bit body, rows equal the oracle's after unpack32 with the mirror's bases.
    The stream is auto_base_stream.next_batch; the tick's list is a random subset of the round plus, for every group the previous tick wiped, the
    AppendEntries its leader sends next (refresh_batch). A one-round tick moves a wiped group's base BEFORE that row arrives — commitIndex and the emptied
    log's bounds then still lie where they were — so the wipes jump by 2^26 .. 2^27, below the window: what stays behind stays inside the 32-bit image."""
    st0, base = S.start_state(G, P, self_slot, seed)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    gpu.set_index_base(base)
    gpu.set_auto_index_base(S.WINDOW)
    gpu.load_state(st0)
    orc.load_state(st0)
    gpu.wide_body_workgroups(reset=True)
    tick = engine.Tick2(gpu, 1, entry_cap=G, expired_cap=0, send=False, ready=False, sparse_cap=G)
    rng = np.random.default_rng(seed)
    mirror = base.copy()
    wiped = np.zeros(G, dtype=bool)
    flushes = 0
    for k in range(ticks):
        cur = orc.read_state()
        b = S.next_batch(cur, rng, P, self_slot, wipe=0.35, jump=(1 << 26, 1 << 27))
        pick = rng.random(G) < fills[k % len(fills)]
        fresh = S.refresh_batch(cur, wiped, P, self_slot, rng)
        redo = np.flatnonzero((fresh.head["hdr"] & 0xF) != abi.EV_NONE)
        b.head[redo], b.ab[redo], b.cd[redo] = fresh.head[redo], fresh.ab[redo], fresh.cd[redo]
        b.entry_terms, b.entry_count = fresh.entry_terms, fresh.entry_count
        pick[redo] = True
        pick[int(rng.integers(0, G))] = True
        rows = np.flatnonzero(pick)
        sub = subset(b, rows)
        b32 = engine.pack32(sub, index_base=mirror)
        tick.refill(b32, [100 + k])
        tick.launch()
        tick.wait()
        got, _ = engine.unpack32(tick.outcome32(), 1, len(rows), cur.role_epoch[rows], index_base=mirror[rows])      # (the rows speak the bases the tick started with)
        oo = orc.submit(sub, fill=0xAB)
        compare_outcomes(oo, got, "automatic bases, tick %d" % k)
        want = S.advance(sub, mirror)
        engine.advance_index_base(b32, mirror, S.WINDOW)
        assert np.array_equal(mirror, want)
        assert np.array_equal(gpu.index_base(), mirror), "tick %d" % k
        assert gpu.wide_body_workgroups() == 0, "tick %d" % k
        is_flush = (sub.head["hdr"] & 0xF) == abi.EV_LOG_FLUSH
        flushes += int(np.count_nonzero(is_flush))
        wiped[:] = False
        wiped[rows] = is_flush & (sub.ab["x"] > orc.read_state().last_index[rows]) & (abi.flags_status(oo.reply["flags"]) == abi.OK)
    compare_states(orc.read_state(), gpu.read_state(), "automatic bases final")
    assert flushes > 0 and np.count_nonzero(mirror != base) > 0
    tick.close()
    gpu.close()
    orc.close()
    return flushes, int(np.count_nonzero(mirror != base))


def stale_recording_case(G=64):
    gpu = engine.Table(G, 3, 0, True)
    tick = engine.Tick2(gpu, 1, expired_cap=G, sparse_cap=G)
    tick.refill(abi.Batch(1, 0, gid=np.zeros(0, np.uint32)), [5])
    tick.launch()
    tick.wait()
    gpu.set_option(abi.OPT_REQUIRE_FENCED_TIMEOUTS, 1)
    with pytest.raises(engine.EngineError, match="changed after rg_tick2_create"):
        tick.launch()
    tick.close()
    gpu.close()
