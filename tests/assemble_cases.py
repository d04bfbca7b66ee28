"""Cases for rg_assemble32 (include/raftgpu.h, "assembling a batch on the device"): arrival-ordered events, and the tickets a tick listed, into the [round][row]
columns rg_submit32c_sparse_rounds and the sparse tick with a depth read. Shared by tests/test_assemble_gpu.py (an MI355X) and tests/devemu/emu_cases_assemble.py
(the host emulation of the kernels, small tables).

The LAYOUT is held bit for bit against model() below, a numpy restatement of the header's contract (a stable sort of the sequence S by gid). The DECISIONS are
held against tests/oracle_lib.OracleTable by assembled_tick_case(): the oracle leads round after round (lead(), modelled on sparse_rounds_cases.lead but
HOLE-FREE: a group of depth d has its events in rounds 0 .. d - 1, which is what an arrival log can express), the tick's events minus the fired groups' TIMEOUT
rows are shuffled into an arrival log that keeps every group's order, and the device gets rg_assemble32(RG_MEM_DEVICE) — the previous tick's expired_* columns as
its second source — followed by rg_tick2_launch of ONE rg_tick2_create_sparse_rounds recording made over the assembler's output columns. The host writes the
arrival log, the entry terms its rows address, the clocks and the per-row send inputs (heartbeat / in_flight: producing those on the device is not part of the
feature), and waits. RG_NEED_HOST rows are repaired with the shadow-oracle protocol of tests/sparse_rounds_cases.py; their share is capped at 2 % of the listed
rows, asserted."""
import ctypes as C
import types

import numpy as np

from rafting_amd import abi, engine
from tests import auto_base_stream as S
from tests.clock import origin as clock_origin
from tests import fuzz, oracle_lib
from tests import sparse_rounds_cases as X
from tests.helpers import compare_outcomes, compare_states
from tests.sparse_tick_cases import assert_untouched, subset

FILL = 0xAB
NONE, EXPIRED = 0xFFFFFFFF, 0x80000000
TIMEOUT_HDR = int(abi.hdr_make(abi.EV_TIMEOUT))


# ---- the model: the header's contract in numpy ----------------------------------------------------------------------------------------------------------------
def model(groups, gid, head, abcd, capacity, max_rounds, expired=None, count=None, deferred_capacity=None):
    """-> SimpleNamespace(n, R, gid[n], head / abcd / origin [R][n], deferred (all of them, S order), stats[4]). expired = (gids, epochs, *expired_count)"""
    gid = np.asarray(gid, np.uint32)
    m = min(len(gid) if count is None else int(count), len(gid))
    e = 0
    if expired is not None:
        e = 0 if int(expired[2]) == 0xFFFFFFFF else min(int(expired[2]), len(expired[0]))
    sg = np.concatenate([np.asarray(expired[0], np.uint32)[:e] if e else np.zeros(0, np.uint32), gid[:m]]).astype(np.int64)
    ids = np.concatenate([EXPIRED | np.arange(e, dtype=np.uint32), np.arange(m, dtype=np.uint32)])
    sh, sa = np.zeros(e + m, abi.HEAD_DT), np.zeros(e + m, abi.QUAD32_DT)
    if e:
        sh["hdr"][:e], sh["aux"][:e] = TIMEOUT_HDR, np.asarray(expired[1], np.uint32)[:e]
    sh[e:], sa[e:] = np.asarray(head)[:m], np.asarray(abcd)[:m]
    valid = sg < groups
    listed = np.unique(sg[valid])[:capacity]
    n = len(listed)
    order = np.flatnonzero(valid)[np.argsort(sg[valid], kind="stable")]              # S by gid, stably: a group's events in S order, groups ascending
    first = np.searchsorted(sg[order], sg[order], side="left")                       # (where each event's group starts in that order)
    rank = np.empty(e + m, np.int64)
    rank[order] = np.arange(len(order)) - first
    row = np.searchsorted(listed, sg)
    placed = valid & (row < n) & (rank < max_rounds)
    placed[placed] &= listed[row[placed]] == sg[placed]
    R = int(rank[placed].max()) + 1 if placed.any() else 1
    oh, oa, oo = np.zeros((R, max(n, 1)), abi.HEAD_DT), np.zeros((R, max(n, 1)), abi.QUAD32_DT), np.full((R, max(n, 1)), NONE, np.uint32)
    oh[rank[placed], row[placed]], oa[rank[placed], row[placed]], oo[rank[placed], row[placed]] = sh[placed], sa[placed], ids[placed]
    deferred = ids[valid & ~placed]
    stats = np.array([np.count_nonzero(placed), len(deferred), np.count_nonzero(~valid), 0], np.uint32)
    return types.SimpleNamespace(n=n, R=R, gid=listed.astype(np.uint32), head=oh[:, :n], abcd=oa[:, :n], origin=oo[:, :n], deferred=deferred, stats=stats)


def check_layout(got, want, capacity, max_rounds, where):
    """the device's columns (engine.Assembler.assemble's namespace: [D][C] images over FILL bytes) against the model's, bit for bit, and FILL wherever the contract
    says NOT TOUCHED"""
    n, R, Cc, D = want.n, want.R, capacity, max_rounds
    assert (got.n, got.R) == (n, R), (where, got.n, got.R, n, R)
    assert np.array_equal(got.stats, want.stats), (where, got.stats, want.stats)
    assert np.array_equal(got.gid[:n], want.gid), where
    assert np.all(got.gid[n:Cc] == FILL * 0x01010101), "%s: gid beyond the count was written" % where
    for name, width in (("head", 8), ("abcd", 16), ("origin", 4)):
        img = getattr(got, name).view(np.uint8)[: D * Cc * width].reshape(D, Cc, width)
        ref = np.ascontiguousarray(getattr(want, name)).view(np.uint8).reshape(R, n, width)
        assert np.array_equal(img[:R, :n], ref), "%s: %s" % (where, name)
        assert np.all(img[R:] == FILL), "%s: %s: a round at or beyond the depth was written" % (where, name)
        assert np.all(img[:R, n:] == FILL), "%s: %s: a row at or beyond the count was written" % (where, name)
    k = min(len(want.deferred), got.deferred_capacity)
    assert np.array_equal(got.deferred[:k], want.deferred[:k]), where
    assert np.all(got.deferred[k: got.deferred_capacity] == FILL * 0x01010101), "%s: deferred beyond the list was written" % where


def assemble_device(asm, gid, head, abcd, capacity, max_rounds, expired=None, deferred_capacity=None, count=None, log_capacity=None):
    """engine.Assembler.assemble's twin in RG_MEM_DEVICE: every column in device memory (outputs over FILL bytes), one asynchronous run, one sync, read back"""
    t = asm.table
    gid = np.ascontiguousarray(gid, np.uint32)
    m, Cc, D = len(gid), int(capacity), int(max_rounds)
    dcap = m + (len(expired[0]) if expired is not None else 0) if deferred_capacity is None else int(deferred_capacity)
    up = lambda a: engine.DeviceBuffer.from_host(t, a)      # noqa: E731
    bufs = dict(count=up(np.array([m if count is None else count], np.uint32)), gid=up(gid), head=up(np.ascontiguousarray(head, abi.HEAD_DT)),
                abcd=up(np.ascontiguousarray(abcd, abi.QUAD32_DT)))
    a = abi.CArrivals()
    a.count, a.capacity, a.gid, a.head, a.abcd = bufs["count"].ptr, m if log_capacity is None else log_capacity, bufs["gid"].ptr, bufs["head"].ptr, bufs["abcd"].ptr
    if expired is not None:
        bufs.update(eg=up(np.ascontiguousarray(expired[0], np.uint32)), ee=up(np.ascontiguousarray(expired[1], np.uint32)), ec=up(np.array([expired[2]], np.uint32)))
        a.expired_gid, a.expired_epoch, a.expired_count, a.expired_capacity = bufs["eg"].ptr, bufs["ee"].ptr, bufs["ec"].ptr, len(expired[0])
    cells = max(Cc * D, 1)
    fill = lambda dt, k: up(np.full(max(k, 1) * np.dtype(dt).itemsize, FILL, np.uint8))      # noqa: E731
    outs = dict(gid=fill(np.uint32, Cc), count=fill(np.uint32, 1), rounds=fill(np.uint32, 1), head=fill(abi.HEAD_DT, cells), abcd=fill(abi.QUAD32_DT, cells),
                origin=fill(np.uint32, cells), deferred=fill(np.uint32, dcap), stats=fill(np.uint32, 4))
    b = abi.CAssembled()
    b.capacity, b.max_rounds, b.deferred_capacity = Cc, D, dcap
    for k, v in outs.items():
        setattr(b, k, v.ptr)
    asm.run_device(a, b)
    t.sync()
    out = types.SimpleNamespace(gid=outs["gid"].to_host(np.uint32, max(Cc, 1)), head=outs["head"].to_host(abi.HEAD_DT, cells), abcd=outs["abcd"].to_host(abi.QUAD32_DT, cells),
                                origin=outs["origin"].to_host(np.uint32, cells), deferred=outs["deferred"].to_host(np.uint32, max(dcap, 1)),
                                stats=outs["stats"].to_host(np.uint32, 4), deferred_capacity=dcap)
    out.n, out.R = int(outs["count"].to_host(np.uint32, 1)[0]), int(outs["rounds"].to_host(np.uint32, 1)[0])
    for x in list(bufs.values()) + list(outs.values()):
        x.free()
    return out


def _rows(rng, m):
    """m rows of anything: the assembler moves them verbatim"""
    head, abcd = np.zeros(m, abi.HEAD_DT), np.zeros(m, abi.QUAD32_DT)
    head["hdr"], head["aux"] = rng.integers(0, 1 << 32, m, dtype=np.uint64), rng.integers(0, 1 << 32, m, dtype=np.uint64)
    for f in "abcd":
        abcd[f] = rng.integers(-(1 << 31), 1 << 31, m)
    return head, abcd


def layout_inputs(G, seed, events=None):
    """the seeded inputs of the layout check for a table of G groups -> [(name, kwargs of model() / Assembler.assemble())]. events: the size of the large logs
    (default G)."""
    rng = np.random.default_rng(seed)
    big = G if events is None else events
    cases = []

    def add(name, gid, C_=G, D=3, **kw):
        gid = np.asarray(gid, np.uint32)
        head, abcd = _rows(rng, len(gid))
        cases.append((name, dict(gid=gid, head=head, abcd=abcd, capacity=C_, max_rounds=D, **kw)))

    def fired(k, lo=0, hi=G):
        return (np.sort(rng.choice(np.arange(lo, hi), min(k, hi - lo), replace=False)).astype(np.uint32), rng.integers(1, 1 << 20, min(k, hi - lo)).astype(np.uint32))
    for fill in (0.0, 0.01, 0.1, 0.5, 1.0):                                           # random logs, repeats included, with and without the second source
        m = int(round(fill * big))
        add("fill %g" % fill, rng.integers(0, G, m))
        eg, ee = fired(max(G // 50, 1))
        add("fill %g + fired tickets" % fill, rng.integers(0, G, m), expired=(eg, ee, len(eg)))
    add("no events", [])
    eg, ee = fired(5)
    add("no events, fired tickets", [], expired=(eg, ee, 5))
    add("one group, more events than rounds", np.full(10, G // 2), C_=16, D=4)             # depth overflow, ordered by one lane
    add("one group, a long segment", np.full(max(big // 4, 300), G - 1), C_=16, D=4)       # ... by a workgroup (the radix select)
    eg, ee = fired(3, lo=G // 3, hi=G // 3 + 3)
    add("three groups of hundreds, fired tickets first", rng.integers(G // 3, G // 3 + 3, 700), C_=8, D=64, expired=(eg, ee, 3))
    add("a long and a short segment at depth 1", np.concatenate([np.full(100, 7), rng.integers(0, G, 50)])[rng.permutation(150)], D=1)
    add("more groups than rows", rng.permutation(G)[: G // 2], C_=max(G // 8, 1))     # capacity overflow
    add("both overflows, a short deferred list", rng.integers(0, max(G // 4, 1), big), C_=max(G // 16, 1), D=2, deferred_capacity=17)
    add("no room for any deferred id", rng.integers(0, 4, 64), D=2, deferred_capacity=0)
    g = rng.integers(0, G, 200)
    g[::7], g[3::11], g[5] = G, G + 12345, 0xFFFFFFFF
    add("gids at and above the group count", g)
    eg, ee = fired(40)
    eg[5] = G + 3
    add("a fired list longer than its columns", rng.integers(0, G, 100), expired=(eg[:24], ee[:24], 1000))
    add("a fired list from a look-back that hit its bound", rng.integers(0, G, 100), expired=(eg, ee, 0xFFFFFFFF))
    add("a log longer than its count", rng.integers(0, G, 300), count=120)
    add("a count beyond the log", rng.integers(0, G, 90), count=5000)
    add("depth 64", rng.integers(0, 3, 150), C_=8, D=64)
    return cases


def layout_case(G, seed, device=False, events=None, P=3):
    """every input of layout_inputs() through ONE assembler, each TWICE (the scratch is put back, the result is a function of the inputs), against the model"""
    t = engine.Table(G, P)
    cases = layout_inputs(G, seed, events)
    most = max(len(kw["gid"]) for _, kw in cases)
    asm = engine.Assembler(t, most, max_expired=max(G // 50, 64))
    for name, kw in cases:
        want = model(G, **kw)
        for again in (0, 1):
            got = assemble_device(asm, **kw) if device else asm.assemble(fill=FILL, **kw)
            check_layout(got, want, kw["capacity"], kw["max_rounds"], "%s (%d groups, run %d)" % (name, G, again))
    asm.close()
    t.close()
    return len(cases)


# ---- the oracle leads, hole-free --------------------------------------------------------------------------------------------------------------------------------
def lead(orc, fz, rng, G, k, fired_g, fired_e, P, Rmax=X.RMAX):
    """The oracle's half of tick k. The list: the groups whose ticket fired at the end of the previous tick (their fenced TIMEOUT in round 0) and a random share
    FILLS[k % 5] of the groups for which the fuzzer drew an event in round 0. Every listed group draws a depth 1 .. DEPTHS[(k // 5) % 5] and keeps its events
    round after round until that depth — or until the fuzzer draws RG_EV_NONE for it, which ends its run of events: no holes. The oracle decides round after round
    (all rounds of a tick share one list; a group past its depth carries RG_EV_NONE, as the assembler fills it) for R = the greatest depth reached, 1 for an empty
    list. -> sparse_rounds_cases.lead's namespace (so that its _check_rows / repair serve) + the compact rows (b32) and, per cell, whether it is an arrival."""
    fill, Rk = X.FILLS[k % len(X.FILLS)], X.DEPTHS[(k // len(X.FILLS)) % len(X.DEPTHS)]
    start = orc.read_state()
    fired = np.zeros(G, dtype=bool)
    fired[fired_g] = True
    b = abi.Batch(1, G)
    fz.round(start, b, 0)
    for g, e in zip(fired_g, fired_e):
        b.head[int(g)], b.ab[int(g)], b.cd[int(g)] = (TIMEOUT_HDR, int(e)), (0, 0), (0, 0)       # (the row the assembler makes of a fired ticket)
    drawn = (b.head["hdr"] & 0xF) != abi.EV_NONE
    pick = ((rng.random(G) < fill) & drawn) | fired
    rows = np.flatnonzero(pick)
    n = len(rows)
    gid = rows.astype(np.uint32)
    depth = rng.integers(1, Rk + 1, n)
    alive = np.ones(n, dtype=bool)
    subs, outs, dense, nows = [], [], [], []
    early = 0
    for r in range(Rk if n else 0):
        if r:
            b = abi.Batch(1, G)
            fz.round(orc.read_state(), b, 0)
        sub = subset(b, rows)
        alive &= (depth > r) & ((sub.head["hdr"] & 0xF) != abi.EV_NONE)
        if not alive.any():
            break
        sub.head[~alive] = (0, 0)
        keep = np.zeros(G, dtype=bool)
        keep[rows[alive]] = True
        b.head[~keep] = (0, 0)
        assert abi.batch_fits_32(sub)
        nows.append(X.now_of(k, r))
        oo = orc.submit(sub, now=[nows[-1]])
        orc.timers_update(1, n, oo.reply, [nows[-1]], gid=gid)
        subs.append(sub)
        outs.append(oo)
        dense.append(b)
    R = max(len(subs), 1)
    if not nows:
        nows = [X.now_of(k, 0)]
    for r in range(1, len(outs)):
        early += int(np.count_nonzero(outs[r - 1].reply["flags"] & abi.F_ROLE_CHANGED))
    batch = want = b32 = arrival = None
    if n:
        batch = fuzz.concat_batches(subs)
        batch.gid = gid
        want = fuzz.concat_outcomes(outs)
        b32 = engine.pack32(batch)
        arrival = ((b32.head["hdr"] & 0xF) != abi.EV_NONE).reshape(R, n)
        arrival[0, fired[rows]] = False
    expired = orc.timers_expired_epochs(nows[-1], capacity=G)
    return types.SimpleNamespace(k=k, fill=fill, R=R, pick=pick, rows=rows, gid=gid, n=n, nows=nows, start=start, batch=batch, want=want, expired=expired,
                                 early_conversions=early, subs=subs, dense=dense, b32=b32, arrival=arrival)


def arrival_log(t, rng):
    """the tick's arrivals in a random interleaving that keeps every group's order -> (gid, head, abcd of the log, and where event k must land: round, row)"""
    if not t.n:
        return np.zeros(0, np.uint32), np.zeros(0, abi.HEAD_DT), np.zeros(0, abi.QUAD32_DT), np.zeros(0, np.int64), np.zeros(0, np.int64)
    r, i = np.nonzero(t.arrival)
    order = np.argsort(r + rng.random(len(r)), kind="stable")
    r, i = r[order], i[order]
    cell = r * t.n + i
    return t.gid[i], t.b32.head[cell], t.b32.abcd[cell], r, i


def lead_only(G, P, seed, ticks):
    """the oracle's half of assembled_tick_case alone (no device) -> rows decided; what a stream looks like can be checked without the emulation"""
    _, orc, _, fz, rng, rng2 = X._tables(G, P, seed, device=False)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    rows = 0
    for k in range(ticks):
        t = lead(orc, fz, rng, G, k, fired_g, fired_e, P)
        if t.n:
            hb, fl = X._traffic(rng2, t.n, P)
            orc.replicate(gid=t.gid, heartbeat=hb, in_flight=fl)
            rows += t.R * t.n
        fired_g, fired_e = t.expired[0], t.expired[1]
    orc.close()
    return rows


def assembled_tick_case(G, seed, ticks, P=5, device_resident=False, expect_all=True):
    """rg_assemble32(RG_MEM_DEVICE) -> rg_tick2_launch, tick after tick, in lockstep with the oracle (module docstring). Checked every tick, as
    sparse_rounds_cases.rounds_tick_case checks them: the list, the count and the depth the assembler wrote; `origin` of every cell (an arrival's log index where the
    lead put it, a fired ticket's entry in round 0, none elsewhere); the outcome rows — row (r, i) answers the event origin[r][i] names —, table state, groups outside
    the list bit for bit, deadlines, health columns, the expired list, send rows and readiness."""
    gpu, orc, shadow, fz, rng, rng2 = X._tables(G, P, seed)
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
    seen = dict(deep=0, ragged=0, early_conversion=0, fired_rows=0, uneven_depths=0, append=0, ready0=0, ready1=0)
    rows = listed = left_out = 0
    for k in range(ticks):
        t = lead(orc, fz, rng, G, k, fired_g, fired_e, P)
        where = "tick %d (%d rounds x %d rows)" % (k, t.R, t.n)
        before = gpu.read_state()
        # the host's part: the arrival log, the entry terms its rows address, all clocks (it does not know the depth), the send inputs of the rows
        lg, lh, la, at_r, at_i = arrival_log(t, rng)
        m = len(lg)
        log_gid[:m], log_head[:m], log_abcd[:m], log_count[0] = lg, lh, la, m
        if t.n and t.b32.entry_count:
            tick._put(tick.entry_terms, t.b32.entry_terms[: t.b32.entry_count])
        tick.now[:] = [X.now_of(k, r) for r in range(RMAX)]
        assert list(tick.now[: t.R]) == t.nows
        if t.n:
            hb, fl = X._traffic(rng2, t.n, P)
            tick._put(tick.heartbeat, hb)
            for j in range(P - 1):
                tick._put(tick.in_flight, np.ascontiguousarray(fl.T[j]), at=j * G)
        origin[:] = 0xABABABAB
        asm.run_device(arr, out)
        tick.launch()
        tick.wait()
        # what the assembler wrote: the list, n, R, the routing
        tick.n, tick.depth = int(tick.count[0]), int(tick.depth_now[0])
        assert (tick.n, tick.depth) == (t.n, t.R), (where, tick.n, tick.depth)
        assert not t.n or np.array_equal(tick._get(tick.gid, np.uint32, t.n), t.gid), where
        assert list(stats) == [m + len(fired_g), 0, 0, 0], (where, list(stats))
        if t.n:
            want_origin = np.full((t.R, t.n), NONE, np.uint32)
            want_origin[at_r, at_i] = np.arange(m, dtype=np.uint32)
            fr = np.flatnonzero(np.isin(t.rows, fired_g))
            want_origin[0, fr] = EXPIRED | np.searchsorted(fired_g, t.gid[fr]).astype(np.uint32)
            assert np.array_equal(origin.reshape(RMAX, G)[: t.R, : t.n], want_origin), where
            assert np.all(origin.reshape(RMAX, G)[t.R:] == 0xABABABAB) and np.all(origin.reshape(RMAX, G)[:, t.n:] == 0xABABABAB), where
            seen["fired_rows"] += len(fr)
            seen["uneven_depths"] += len(np.unique(t.arrival.sum(axis=0))) > 1
        bad = np.zeros(0, dtype=np.int64)
        if t.n:
            bad = X._check_rows(gpu, shadow, t, tick.outcome32(), where, fold=True)
        eo, epo, no = t.expired
        eg, epg, ng = tick.expired()
        assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo), where
        assert np.array_equal(gpu.timers_read(), orc.timers_read()), where
        for a, c in zip(gpu.health_read(), orc.health_read()):
            assert np.array_equal(a, c), where
        if t.n:
            ok = np.ones(t.n, dtype=bool)
            ok[bad] = False
            (hg, sg), (ho, so) = tick.sends(), orc.replicate(gid=t.gid, heartbeat=hb, in_flight=fl)
            if len(bad):
                gpu.replicate(gid=t.gid[bad], heartbeat=hb[bad], in_flight=fl[bad])
            for f in ("term", "leader_commit", "epoch_index", "epoch_term", "role_epoch", "is_leader"):
                assert np.array_equal(hg[f][ok], ho[f][ok]), (where, f)
            for f in ("prev_index", "prev_term", "last_index", "count", "kind"):
                assert np.array_equal(sg[f][ok], so[f][ok]), (where, f)
            rd, ro = tick.readiness(), orc.ready(t.nows[-1], 1, 60)[t.rows]
            assert np.array_equal(rd[ok], ro[ok]), where
            seen["append"] += int(np.count_nonzero(so["kind"] == abi.SEND_APPEND))
            seen["ready0"] += int(np.count_nonzero(ro == 0))
            seen["ready1"] += int(np.count_nonzero(ro == 1))
        after = gpu.read_state()
        compare_states(orc.read_state(), after, where)
        assert_untouched(before, after, ~t.pick, where)
        seen["deep"] += t.n > 0 and t.R >= 3
        seen["ragged"] += t.n % 64 != 0
        seen["early_conversion"] += t.early_conversions
        rows += t.R * t.n
        listed += t.n
        left_out += len(bad)
        fired_g, fired_e = eg, epg
    if expect_all:
        assert all(v > 0 for v in seen.values()), seen
    assert left_out * 50 <= listed, "%d of %d listed rows were left out of the send / readiness comparison (cap: 2 %%)" % (left_out, listed)
    asm.close()
    tick.close()
    for p in pins:
        p.free()
    for x in (gpu, orc, shadow):
        x.close()
    return rows, left_out


# ---- the stand-alone form ---------------------------------------------------------------------------------------------------------------------------------------
def standalone_case(G, P, seed, launches):
    """the assembled columns, n and R read back, through rg_submit32c_sparse_rounds on one table; the model's columns through the same call on a second; the
    oracle leads (lead(): real rows on real state). Rows and table state are identical, launch after launch."""
    a, d, orc, fz, rng = None, None, None, None, None
    self_slot = 2 % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    a, d, orc = engine.Table(G, P, self_slot, True), engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    for t in (a, d, orc):
        t.load_state(st0)
    orc.timers_configure(900, 300, 4321)
    orc.timers_arm(clock_origin())
    fz, rng = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False), np.random.default_rng(seed)
    asm = engine.Assembler(a, X.RMAX * G, max_expired=G)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    rows = 0
    for k in range(launches):
        t = lead(orc, fz, rng, G, k, fired_g, fired_e, P)
        fired_g, fired_e = t.expired[0], t.expired[1]
        if not t.n:
            continue
        lg, lh, la, _, _ = arrival_log(t, rng)
        exp = (np.flatnonzero(~t.arrival[0] & ((t.b32.head["hdr"][: t.n] & 0xF) != abi.EV_NONE)),)
        exp_g = t.gid[exp[0]]
        exp_e = t.b32.head["aux"][: t.n][exp[0]]
        kw = dict(gid=lg, head=lh, abcd=la, capacity=G, max_rounds=X.RMAX, expired=(exp_g, exp_e, len(exp_g)))
        got, want = asm.assemble(fill=FILL, **kw), model(G, **kw)
        check_layout(got, want, G, X.RMAX, "launch %d" % k)
        n, R = got.n, got.R
        assert (n, R) == (t.n, t.R)

        def batch_of(head, abcd, gid):
            return abi.Batch32(R, n, np.ascontiguousarray(gid[:n]), np.ascontiguousarray(head).reshape(-1), np.ascontiguousarray(abcd).reshape(-1),
                               t.b32.entry_terms, t.b32.entry_count)
        ba = batch_of(got.head.reshape(X.RMAX, G)[:R, :n], got.abcd.reshape(X.RMAX, G)[:R, :n], got.gid)
        bd = batch_of(want.head, want.abcd, want.gid)
        ra, rd = a.submit32c_sparse_rounds(ba, wide=False), d.submit32c_sparse_rounds(bd, wide=False)
        X._same_rows(ra, rd, "launch %d: the assembled columns vs the model's" % k)
        compare_states(d.read_state(), a.read_state(), "launch %d" % k)
        got32, _ = engine.unpack32(ra, R, n, t.start.role_epoch[t.rows])
        if not np.any(got32.status == abi.NEED_HOST):                      # ... and they are the oracle's, where the device needed no help
            compare_outcomes(t.want, got32, "launch %d" % k)
            compare_states(orc.read_state(), a.read_state(), "launch %d" % k)
        else:                                                              # (a group the device stopped: bring both tables back in step with the oracle)
            st = orc.read_state()
            a.load_state(st)
            d.load_state(st)
        rows += R * n
    assert rows > 0
    asm.close()
    for t in (a, d, orc):
        t.close()
    return rows


# ---- automatic index bases: verbatim rows, moving bases -----------------------------------------------------------------------------------------------------------
def auto_base_case(G, launches, seed, R=3, P=5, self_slot=1, fills=(1.0, 0.5, 0.25)):
    """sparse_rounds_cases.auto_base_rounds_case's stream at 2^40 (tests/auto_base_stream.py), hole-free, its rows packed against a host mirror of the bases and
    handed over as an ARRIVAL LOG: rg_assemble32(RG_MEM_DEVICE) -> the tick. The assembler moves rows verbatim, the launch that decides them reads the table's
    bases: the rows equal the oracle's after unpack32 with the bases the launch started with, the table's bases equal the mirror, no workgroup takes the 64-bit body."""
    st0, base = S.start_state(G, P, self_slot, seed)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    gpu.set_index_base(base)
    gpu.set_auto_index_base(S.WINDOW)
    gpu.load_state(st0)
    orc.load_state(st0)
    gpu.wide_body_workgroups(reset=True)
    tick = engine.Tick2(gpu, R, entry_cap=G * R, expired_cap=0, send=False, ready=False, sparse_cap=G, sparse_rounds=True)
    asm = engine.Assembler(gpu, R * G)
    pins = []

    def pinned(dtype, k):
        a, p = engine.pinned_like(gpu, np.zeros(max(k, 1), dtype=dtype))
        pins.append(p)
        return a
    log_count, log_gid, log_head, log_abcd = pinned(np.uint32, 1), pinned(np.uint32, R * G), pinned(abi.HEAD_DT, R * G), pinned(abi.QUAD32_DT, R * G)
    origin, stats = pinned(np.uint32, R * G), pinned(np.uint32, 4)
    arr = abi.CArrivals()
    arr.count, arr.capacity, arr.gid, arr.head, arr.abcd = log_count.ctypes.data, R * G, log_gid.ctypes.data, log_head.ctypes.data, log_abcd.ctypes.data
    out = asm.for_tick(tick, origin.ctypes.data, None, 0, stats.ctypes.data)
    rng = np.random.default_rng(seed)
    mirror = base.copy()
    wiped = np.zeros(G, dtype=bool)
    flushes = late = deep = 0
    for k in range(launches):
        start = orc.read_state()
        subs, outs = [], []
        rows = alive = None
        for r in range(R):
            cur = orc.read_state()
            b = S.next_batch(cur, rng, P, self_slot, wipe=0.35, jump=(1 << 25, 1 << 26), idle=0.1)
            fresh = S.refresh_batch(cur, wiped, P, self_slot, rng)
            redo = np.flatnonzero((fresh.head["hdr"] & 0xF) != abi.EV_NONE)
            b.head[redo], b.ab[redo], b.cd[redo] = fresh.head[redo], fresh.ab[redo], fresh.cd[redo]
            b.entry_terms, b.entry_count = fresh.entry_terms, fresh.entry_count
            drawn = (b.head["hdr"] & 0xF) != abi.EV_NONE
            if r == 0:
                pick = ((rng.random(G) < fills[k % len(fills)]) | wiped) & drawn
                pick[int(np.flatnonzero(drawn)[0])] = True
                rows = np.flatnonzero(pick)
                alive = np.ones(len(rows), dtype=bool)
            sub = subset(b, rows)
            # (a group ends its run of events at random — never right after a wipe: its leader's next AppendEntries belongs to the stream, refresh_batch's docstring)
            alive &= drawn[rows] & ((rng.random(len(rows)) < 0.8) | wiped[rows])
            if r == 0:
                alive[:] = True
            if not alive.any():
                break
            sub.head[~alive] = (0, 0)
            oo = orc.submit(sub, fill=0xAB)
            is_flush = (sub.head["hdr"] & 0xF) == abi.EV_LOG_FLUSH
            flushes += int(np.count_nonzero(is_flush))
            late += int(np.count_nonzero(is_flush)) if r > 0 else 0
            wiped[:] = False
            wiped[rows] = is_flush & (sub.ab["x"] > orc.read_state().last_index[rows]) & (abi.flags_status(oo.reply["flags"]) == abi.OK)
            subs.append(sub)
            outs.append(oo)
        Rk, n = len(subs), len(rows)
        deep += Rk >= 2
        batch = fuzz.concat_batches(subs)
        batch.gid = rows.astype(np.uint32)
        b32 = engine.pack32(batch, index_base=mirror)                     # (the reader's side: rows relative to the mirror of the bases)
        rr, ii = np.nonzero(((b32.head["hdr"] & 0xF) != abi.EV_NONE).reshape(Rk, n))
        order = np.argsort(rr + rng.random(len(rr)), kind="stable")
        cell = rr[order] * n + ii[order]
        m = len(cell)
        log_gid[:m], log_head[:m], log_abcd[:m], log_count[0] = batch.gid[ii[order]], b32.head[cell], b32.abcd[cell], m
        if b32.entry_count:
            tick._put(tick.entry_terms, b32.entry_terms[: b32.entry_count])
        tick.now[:] = [100 + 10 * k + r for r in range(R)]
        asm.run_device(arr, out)
        tick.launch()
        tick.wait()
        tick.n, tick.depth = int(tick.count[0]), int(tick.depth_now[0])
        assert (tick.n, tick.depth) == (n, Rk) and list(stats) == [m, 0, 0, 0], (k, tick.n, tick.depth, n, Rk, list(stats))
        got, _ = engine.unpack32(tick.outcome32(), Rk, n, start.role_epoch[rows], index_base=mirror[rows])
        compare_outcomes(fuzz.concat_outcomes(outs), got, "automatic bases, launch %d" % k)
        want = S.advance(batch, mirror)
        engine.advance_index_base(b32, mirror, S.WINDOW)
        assert np.array_equal(mirror, want)
        assert np.array_equal(gpu.index_base(), mirror), "launch %d" % k
        assert gpu.wide_body_workgroups() == 0, "launch %d" % k
    compare_states(orc.read_state(), gpu.read_state(), "automatic bases final")
    assert flushes > 0 and late > 0 and deep > 0 and np.count_nonzero(mirror != base) > 0
    asm.close()
    tick.close()
    for p in pins:
        p.free()
    gpu.close()
    orc.close()
    return flushes, int(np.count_nonzero(mirror != base))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def refusal_structs(G, D=4, m=16, e=4):
    """a correct call on host memory -> (arrivals, assembled, the arrays that back them)"""
    cols = dict(count=np.array([m], np.uint32), gid=np.arange(m, dtype=np.uint32) % G, head=np.zeros(m, abi.HEAD_DT), abcd=np.zeros(m, abi.QUAD32_DT),
                expired_gid=np.arange(e, dtype=np.uint32), expired_epoch=np.ones(e, np.uint32), expired_count=np.array([e], np.uint32),
                o_gid=np.zeros(G, np.uint32), o_count=np.zeros(1, np.uint32), o_rounds=np.zeros(1, np.uint32), o_head=np.zeros(D * G, abi.HEAD_DT),
                o_abcd=np.zeros(D * G, abi.QUAD32_DT), o_origin=np.zeros(D * G, np.uint32), o_deferred=np.zeros(8, np.uint32), o_stats=np.zeros(4, np.uint32))
    a, b = abi.CArrivals(), abi.CAssembled()
    a.capacity, a.expired_capacity = m, e
    for f in ("count", "gid", "head", "abcd", "expired_gid", "expired_epoch", "expired_count"):
        setattr(a, f, cols[f].ctypes.data)
    b.capacity, b.max_rounds, b.deferred_capacity = G, D, 8
    for f in ("gid", "count", "rounds", "head", "abcd", "origin", "deferred", "stats"):
        setattr(b, f, cols["o_" + f].ctypes.data)
    return a, b, cols


def refusals_case(G=64):
    """every refusal of the header's list answers -1 with a message, before any launch; the emulation cannot tell pageable from page-locked memory, so that one
    refusal is checked on the GPU (tests/test_assemble_gpu.py)"""
    t = engine.Table(G, 3)
    L = engine.lib()
    asm = engine.Assembler(t, 16, max_expired=4)

    def refused(text, memspace=abi.MEM_HOST, **change):
        a, b, cols = refusal_structs(G)
        for k, v in change.items():
            setattr(a if k.startswith("a_") else b, k[2:], v)
        rc = L.rg_assemble32(asm._h, C.byref(a), C.byref(b), memspace)
        err = L.rg_last_error(t._h)
        assert rc == -1 and text in err, (change, rc, err)
    for col in ("count", "gid", "head", "abcd"):
        refused(b"of the arrival log are required", **{"a_" + col: None})
    for col in ("gid", "count", "rounds", "head", "abcd", "origin", "stats", "deferred"):
        refused(b"of the batch are required", **{"b_" + col: None})
    refused(b"capacity 0 outside", b_capacity=0)
    refused(b"capacity %d outside" % (G + 1), b_capacity=G + 1)
    refused(b"max_rounds 0 outside 1 .. 64", b_max_rounds=0)
    refused(b"max_rounds 65 outside 1 .. 64", b_max_rounds=65)
    refused(b"the assembler was created for 16", a_capacity=17)
    refused(b"the assembler was created for 4", a_expired_capacity=5)
    for col in ("expired_gid", "expired_epoch", "expired_count"):
        refused(b"all three columns or none", **{"a_" + col: None})
    refused(b"unknown memspace", memspace=7)
    a, b, cols = refusal_structs(G)
    assert L.rg_assemble32(asm._h, None, C.byref(b), abi.MEM_HOST) == -1 and L.rg_assemble32(asm._h, C.byref(a), None, abi.MEM_HOST) == -1
    assert L.rg_assemble32(None, C.byref(a), C.byref(b), abi.MEM_HOST) == -1
    h = C.c_void_p()
    assert L.rg_assembler_create(t._h, 1 << 31, 0, C.byref(h)) == -1 and not h.value and b"2^31" in L.rg_last_error(t._h)
    asm.close()
    t.close()
