"""Cases for rg_scan (the class word of every group, the counts and the ascending list of the selected ones) and for the state exchange by a list of groups
(rg_read_state_list / rg_load_state_list). Shared by tests/test_scan_gpu.py (an MI355X) and tests/devemu/emu_cases_scan.py (the host emulation of the kernels,
at small sizes); tests/test_scan_cpu.py checks the numpy model below on a hand-made table, without any library.

THE MODEL reads only what a host can read without the scan: read_state(), index_base() and timers_read(). It states the header's contract (include/raftgpu.h,
"WHICH GROUPS NEED THE HOST") in numpy. One clause of the contract is out of its sight: RG_SCAN_OFF_IMAGE looks at the words the step kernel loads, and for a
group whose log is EMPTY those include the window and run slot 0 the log's last flush left behind, which read_state() reports as zeros. Every state here is either
loaded through rg_load_state — which stores zeros there — or grown from such a state by traffic whose values stay far below 2^30 on a table without bases, where a
left-over cannot leave the image; the step kernel itself is the witness that does see those words (off_image_kernel_case)."""
import ctypes as C
import types

import numpy as np

from rafting_amd import abi, engine

K = abi.TERM_RUNS
LIM = 1 << 30
SENTINEL = 0xA5A5A5A5
SIZES = ((1000, 3), (4096, 5), (65600, 5), (300, 9))


# ---- the numpy model ---------------------------------------------------------------------------------------------------------------------------------------
def _rel(x, base):
    """an index relative to its group's base: 0 stays 0, x == base != 0 has no image (-1)"""
    b = base.reshape((-1,) + (1,) * (x.ndim - 1))
    return np.where(x == 0, 0, np.where(x == b, -1, x - b))


def off_image(st, base):
    """groups whose state cannot start a compact launch on the 32-bit body: a term or relative index outside [0, 2^30), a small field outside its domain, an
    epoch.index at or below a non-zero base, a negative base, a follower record of a PREPARED group without an image"""
    G, F = st.count, st.followers
    i64 = lambda a: np.asarray(a).astype(np.int64)
    live = np.arange(K)[None, :] < i64(st.run_count)[:, None]
    starts, terms = np.where(live, i64(st.run_start).reshape(G, K), 0), np.where(live, i64(st.run_term).reshape(G, K), 0)
    index = np.concatenate([np.stack([i64(st.commit_index), i64(st.epoch_index), i64(st.first_index), i64(st.last_index)], axis=1), starts], axis=1)
    term = np.concatenate([np.stack([i64(st.current_term), i64(st.epoch_term), i64(st.elected_term)], axis=1), terms], axis=1)
    vals = np.concatenate([_rel(index, base), term], axis=1)
    bad = ((vals < 0) | (vals >= LIM)).any(axis=1)
    small = np.stack([i64(st.role_epoch), i64(st.elected_epoch), i64(st.votes), i64(st.current_leader) + 1, i64(st.voted_for) + 1], axis=1)
    bad |= ((small < 0) | (small >= LIM)).any(axis=1) | (i64(st.role) < 0) | (i64(st.role) > abi.LEADER)
    bad |= ((base != 0) & (_rel(i64(st.epoch_index), base) <= 0)) | (base < 0)
    peers = np.concatenate([_rel(i64(st.peers(n)), base) for n in ("last_epoch", "next_index", "match_index")], axis=1).reshape(G, 3 * F)
    bad |= (st.repl_prepared != 0) & ((peers < 0) | (peers >= LIM)).any(axis=1)
    return bad


def class_words(st, base, deadline, backlog=0, lag=0, now=0):
    i64 = lambda a: np.asarray(a).astype(np.int64)
    role, has_log = i64(st.role), st.run_count > 0
    leader, prepared = role == abi.LEADER, st.repl_prepared != 0
    ready = leader & prepared
    last = i64(st.last_index)
    behind = last - i64(st.commit_index)
    lagging = (last[:, None] - i64(st.peers("match_index"))).max(axis=1)
    flags = [role == abi.FOLLOWER, role == abi.CANDIDATE, leader, (role == abi.FOLLOWER) & (st.current_leader == abi.NO_NODE), st.timeout_detected != 0,
             ~has_log, st.run_count == K, has_log & (behind > backlog), leader & ~prepared, ready & (st.peers("pending") != 0).any(axis=1),
             ready & has_log & (lagging > lag), off_image(st, base), base != 0, deadline == 0, deadline == -1, (deadline > 0) & (deadline <= now)]
    bits = np.zeros(st.count, np.uint32)
    for b, f in enumerate(flags):
        bits |= f.astype(np.uint32) << np.uint32(b)
    return bits, np.where(has_log, np.maximum(behind, 0), 0), np.where(ready & has_log, np.maximum(lagging, 0), 0)


def model(st, base, deadline, any=0, all=0, none=0, backlog=0, lag=0, now=0, capacity=None):
    """-> namespace(bits, selected (every selected gid, ascending), list (its first `capacity`), summary)"""
    bits, behind, lagging = class_words(st, base, deadline, backlog, lag, now)
    chosen = ((bits & np.uint32(any)) != 0 if any else np.ones(st.count, bool)) & ((bits & np.uint32(all)) == all) & ((bits & np.uint32(none)) == 0)
    selected = np.flatnonzero(chosen).astype(np.uint32)
    summary = np.zeros(abi.SCAN_SUMMARY, np.uint64)
    for b in range(16):
        summary[b] = np.count_nonzero(bits & np.uint32(1 << b))
    summary[abi.SCAN_SELECTED] = len(selected)
    summary[abi.SCAN_MAX_TERM] = np.asarray(st.current_term).astype(np.uint64).max()
    summary[abi.SCAN_MAX_BACKLOG], summary[abi.SCAN_SUM_BACKLOG] = behind.max(), behind.astype(np.uint64).sum()
    summary[abi.SCAN_MAX_LAG] = lagging.max()
    return types.SimpleNamespace(bits=bits, selected=selected, list=selected[: len(selected) if capacity is None else capacity], summary=summary)


def model_of(t, **q):
    """the model over what the table's read-back entry points say"""
    return model(t.read_state(), t.index_base(), t.timers_read(), **q)


# ---- states ---------------------------------------------------------------------------------------------------------------------------------------------------
def random_state(G, P, rng, lag=10):
    """all three roles, prepared and unprepared leaders, empty logs and 1 to 4 runs, pending bits, followers on both sides of `lag`; vectorised"""
    st = abi.GroupState(G, P)
    F = P - 1
    role = rng.integers(0, 3, G)
    st.role[:] = role
    st.current_term[:] = rng.integers(1, 60, G)
    st.voted_for[:] = rng.integers(-1, P, G)
    st.current_leader[:] = np.where((role == abi.FOLLOWER) & (rng.random(G) < 0.6), rng.integers(0, P, G), -1)
    st.timeout_detected[:] = (role == abi.FOLLOWER) & (rng.random(G) < 0.3)
    prepared = (role == abi.LEADER) & (rng.random(G) < 0.7)
    st.repl_prepared[:] = prepared
    st.role_epoch[:] = rng.integers(1, 40, G)
    st.votes[:] = rng.integers(1, P + 1, G)
    st.elected_epoch[:] = rng.integers(0, 40, G)
    st.elected_term[:] = rng.integers(0, 60, G)
    rc = rng.integers(0, K + 1, G)
    st.run_count[:] = rc
    st.epoch_index[:] = rng.integers(0, 200, G)
    st.epoch_term[:] = rng.integers(0, 5, G)
    live = np.arange(K)[None, :] < rc[:, None]
    length = rng.integers(1, 30, (G, K))
    first = st.epoch_index + rng.integers(0, 2, G)
    start = first[:, None] + np.concatenate([np.zeros((G, 1), np.int64), np.cumsum(length, axis=1)[:, :-1]], axis=1)
    term = 5 + np.cumsum(rng.integers(1, 4, (G, K)), axis=1)
    st.run_start[:] = np.where(live, start, 0).reshape(-1)
    st.run_term[:] = np.where(live, term, 0).reshape(-1)
    last = np.where(rc > 0, first + np.where(live, length, 0).sum(axis=1) - 1, 0)
    st.first_index[:] = np.where(rc > 0, first, 0)
    st.last_index[:] = last
    st.commit_index[:] = np.where(rc > 0, np.maximum(last - rng.integers(0, 40, G), st.epoch_index), st.epoch_index)
    match = np.where(rng.random((G, F)) < 0.1, 0, np.maximum(last[:, None] - rng.integers(0, 2 * lag + 1, (G, F)), st.epoch_index[:, None]))      # (0: a follower that has not answered)
    keep = prepared[:, None]
    st.peer_match_index[:] = np.where(keep, match, 0).reshape(-1)
    st.peer_next_index[:] = np.where(keep, np.where(match == 0, last[:, None], match) + 1, 0).reshape(-1)
    st.peer_last_epoch[:] = np.where(keep, np.repeat(st.epoch_index[:, None], F, axis=1), 0).reshape(-1)
    st.peer_rejection[:] = np.where(keep, rng.integers(0, 5, (G, F)), 0).reshape(-1)
    st.peer_pending[:] = (keep & (rng.random((G, F)) < 0.1)).reshape(-1)
    return st


def rows_of(st, idx):
    """rows idx of a state image (the default layout: TERM_RUNS run slots per group) as an image of their own"""
    idx = np.asarray(idx, dtype=np.int64)
    out = abi.GroupState(len(idx), st.cluster)
    for name, _, shape in abi._STATE_FIELDS:
        a = getattr(st, name)
        width = 1 if shape == 1 else (K if shape == "runs" else st.followers)
        getattr(out, name)[:] = a.reshape(st.count, width)[idx].reshape(-1)
    out.run_offset[:] = np.arange(len(idx), dtype=np.uint32) * K
    return out


def same_state(a, b, where):
    for name in a.fields():
        assert np.array_equal(getattr(a, name), getattr(b, name)), (where, name)


def dressed_table(G, P, seed, bases=True):
    """a table with a random state, some index bases — half of those groups moved above their base so they stay in the image, the others left below it —, every
    timer armed, some tickets fired and some groups loaded again (no ticket)"""
    rng = np.random.default_rng(seed)
    t = engine.Table(G, P, 1 % P)
    st = random_state(G, P, rng)
    base = np.zeros(G, np.int64)
    if bases:
        based = rng.random(G) < 0.2
        lift = np.where(based & (rng.random(G) < 0.6) & (st.epoch_index > 0), 1 << 33, 0)      # (an epoch.index of 0 stays 0: such a group is off the image under any base)
        for name in ("commit_index", "epoch_index", "first_index", "last_index"):
            a = getattr(st, name)
            a[:] = np.where(a != 0, a + lift, 0)
        for name, width in (("run_start", K), ("peer_last_epoch", P - 1), ("peer_next_index", P - 1), ("peer_match_index", P - 1)):
            a = getattr(st, name).reshape(G, width)
            a[:] = np.where(a != 0, a + lift[:, None], 0)
        base = np.where(based, (1 << 33) - rng.integers(1, 50, G), 0)
        t.set_index_base(base)
    t.load_state(st)
    t.timers_configure(900, 300, seed)
    t.timers_arm(1000)
    t.timers_expired(1000 + 1100, capacity=G // 3)              # (the first third of the overdue tickets fire; the rest stay overdue)
    again = np.flatnonzero(rng.random(G) < 0.1)
    if len(again):
        t.load_state_list(rows_of(st, again), again)            # (loaded groups hold no ticket)
    return t


QUERIES = (dict(), dict(all=0xFFFF), dict(any=abi.SCAN_NO_LEADER | abi.SCAN_TIMEOUT_DETECTED | abi.SCAN_OFF_IMAGE), dict(all=abi.SCAN_LEADER | abi.SCAN_LAGGING),
           dict(none=abi.SCAN_FOLLOWER | abi.SCAN_EMPTY_LOG),
           dict(any=abi.SCAN_BACKLOG | abi.SCAN_RUNS_FULL | abi.SCAN_OVERDUE, all=abi.SCAN_HAS_BASE, none=abi.SCAN_CANDIDATE | abi.SCAN_TICKET_FIRED))
THRESHOLDS = dict(backlog=12, lag=10, now=1000 + 1500)


def scan_device(t, q, capacity, bits=True):
    """one RG_MEM_DEVICE scan into device memory pre-filled with sentinel bytes, one word of slack behind every array -> namespace(bits, list, summary) as they
    lie in device memory (the whole arrays)"""
    G = t.groups
    blank = lambda n: np.full(n + 1, SENTINEL, np.uint32)
    db = engine.DeviceBuffer.from_host(t, blank(G)) if bits else None
    dl = engine.DeviceBuffer.from_host(t, blank(capacity))
    ds = engine.DeviceBuffer.from_host(t, np.full(abi.SCAN_SUMMARY + 1, SENTINEL, np.uint64))
    r = abi.CScanResult(bits=db.ptr if bits else None, list=dl.ptr if capacity else None, list_capacity=capacity, summary=ds.ptr)
    t.scan_device(abi.CScanQuery(reserved=0, **q), r)
    t.sync()
    got = types.SimpleNamespace(bits=db.to_host(np.uint32, G + 1) if bits else None, list=dl.to_host(np.uint32, capacity + 1), summary=ds.to_host(np.uint64, abi.SCAN_SUMMARY + 1))
    for b in (db, dl, ds):
        if b is not None:
            b.free()
    return got


def scan_host(t, q, capacity, bits=True):
    """the same through RG_MEM_HOST, on sentinel-filled numpy arrays"""
    G = t.groups
    words, gids = np.full(G + 1, SENTINEL, np.uint32), np.full(capacity + 1, SENTINEL, np.uint32)
    summary = np.full(abi.SCAN_SUMMARY + 1, SENTINEL, np.uint64)
    r = abi.CScanResult(bits=words.ctypes.data if bits else None, list=gids.ctypes.data if capacity else None, list_capacity=capacity, summary=summary.ctypes.data)
    cq = abi.CScanQuery(reserved=0, **q)
    t._check(engine.lib().rg_scan(t._h, C.byref(cq), C.byref(r), abi.MEM_HOST))
    return types.SimpleNamespace(bits=words if bits else None, list=gids, summary=summary)


def check_scan(got, want, capacity, where):
    """bit for bit, and every NOT TOUCHED clause: list entries beyond what was written and the word behind every array keep their sentinel"""
    G = len(want.bits)
    if got.bits is not None:
        assert np.array_equal(got.bits[:G], want.bits), (where, "bits", np.flatnonzero(got.bits[:G] != want.bits)[:8])
        assert got.bits[G] == SENTINEL, where
    assert np.array_equal(got.summary[: abi.SCAN_SUMMARY], want.summary), (where, got.summary, want.summary)
    assert got.summary[abi.SCAN_SUMMARY] == (SENTINEL if got.summary.dtype == np.uint32 else np.uint64(SENTINEL)), where
    k = min(len(want.selected), capacity)
    assert np.array_equal(got.list[:k], want.selected[:k]), (where, "list")
    assert np.all(got.list[k:] == SENTINEL), (where, "list entries beyond the count were written")


def layout_case(G, P, seed, device=False):
    """a dressed table against the model: six queries, list capacities of 0, below and above the count, with and without the bits column, every input scanned twice
    -> scans checked"""
    t = dressed_table(G, P, seed)
    st, base, deadline = t.read_state(), t.index_base(), t.timers_read()
    run = scan_device if device else scan_host
    full = model(st, base, deadline, **THRESHOLDS)
    for b in range(16):                                       # (the table shows every bit set in some group and clear in another)
        assert 0 < full.summary[b] < G, (b, full.summary)
    scans = 0
    for k, q in enumerate(QUERIES):
        q = dict(q, **THRESHOLDS)
        want = model(st, base, deadline, **q)
        n = len(want.selected)
        assert (n == G) if k == 0 else (n == 0) if k == 1 else (0 < n < G), (k, n)
        for capacity in sorted({0, n // 2, n + 7}):
            where = "G=%d P=%d query %d capacity %d %s" % (G, P, k, capacity, "device" if device else "host")
            first = run(t, q, capacity, bits=capacity != n // 2 or n == 0)
            check_scan(first, want, capacity, where)
            again = run(t, q, capacity, bits=capacity != n // 2 or n == 0)
            for a, b in ((first.bits, again.bits), (first.list, again.list), (first.summary, again.summary)):
                assert (a is None and b is None) or np.array_equal(a, b), (where, "two runs differ")
            scans += 2
    ns = t.scan(capacity=5, **dict(QUERIES[2], **THRESHOLDS))       # (the convenience form)
    want = model(st, base, deadline, capacity=5, **dict(QUERIES[2], **THRESHOLDS))
    assert np.array_equal(ns.bits, want.bits) and np.array_equal(ns.list, want.list) and np.array_equal(ns.summary, want.summary)
    t.close()
    return scans


def live_case(G=1000, P=5, seed=21, ticks=6, rounds=3):
    """a few ticks of mixed traffic (tests/fuzz.py) with the timers folded after every batch and the fired tickets taken: the scan equals the model over
    read_state, timers and bases after every tick. No bases: every value stays far below 2^30 (the module's note on left-overs) -> groups ever selected"""
    from tests import fuzz
    self_slot = 1 % P
    t = engine.Table(G, P, self_slot)
    t.load_state(fuzz.random_initial_state(G, P, self_slot, seed))
    t.timers_configure(90, 30, seed)
    t.timers_arm(0)
    fz = fuzz.Fuzzer(G, P, self_slot, seed)
    picked = 0
    for k in range(ticks):
        b = abi.Batch(rounds, G, max_entries=8 * G * rounds)
        cur = t.read_state()
        for r in range(rounds):
            fz.round(cur, b, r)
        now = [100 * k + 10 * r for r in range(rounds)]
        t.submit_and_update_timers(b, now)
        t.timers_expired(now[-1] + 5, capacity=G // 4)
        q = dict(any=abi.SCAN_NO_LEADER | abi.SCAN_TIMEOUT_DETECTED | abi.SCAN_PENDING_INSTALL | abi.SCAN_RUNS_FULL | abi.SCAN_TICKET_FIRED, none=abi.SCAN_CANDIDATE,
                 backlog=3, lag=5, now=now[-1] + 40)
        want = model_of(t, **q)
        check_scan(scan_host(t, q, G), want, G, "live tick %d" % k)
        picked += len(want.selected)
    assert not (want.bits & abi.SCAN_OFF_IMAGE).any() and (want.bits & abi.SCAN_LEADER).any() and (want.bits & abi.SCAN_TICKET_FIRED).any()
    t.close()
    return picked


# ---- RG_SCAN_OFF_IMAGE against two independent witnesses ---------------------------------------------------------------------------------------------------
def off_image_witness_case(point, P=5):
    """tests/domain_edge_cases.state_out_of_domain on that module's magnitude points. It looks at the peer columns of EVERY group; the kernel's rule, following
    stage_peers, only at those of a group whose `prepared` mark is set. So the states it is run on exclude the unprepared groups whose peer columns hold a value
    without an image (it would flag them, the step kernel does not leave the 32-bit body for them). It also knows no negative base and no role outside 0 .. 2:
    neither occurs at these points. -> (groups compared, groups flagged)"""
    from tests import domain_edge_cases as E
    G, self_slot = E.G, 1 % P
    st = E.state_maker(point)(G, P, self_slot, E.seed_of(point, P))
    mk = E.base_maker(point)
    base = None if mk is None else mk(st)
    t = engine.Table(G, P, self_slot)
    if base is not None:
        t.set_index_base(base)
    t.load_state(st)
    got = t.scan(any=abi.SCAN_OFF_IMAGE, capacity=G)
    flagged = (got.bits & abi.SCAN_OFF_IMAGE) != 0
    b0 = np.zeros(G, np.int64) if base is None else base
    peers = np.concatenate([_rel(np.asarray(st.peers(n)).astype(np.int64), b0) for n in ("last_epoch", "next_index", "match_index")], axis=1)
    excluded = (st.repl_prepared == 0) & ((peers < 0) | (peers >= LIM)).any(axis=1)
    witness = E.state_out_of_domain(st, base)
    keep = ~excluded
    assert np.array_equal(flagged[keep], witness[keep]), (point, np.flatnonzero(flagged[keep] != witness[keep])[:8])
    assert np.array_equal(flagged, off_image(t.read_state(), b0)), point
    assert np.array_equal(got.list, np.flatnonzero(flagged)), point
    t.close()
    return int(keep.sum()), int(flagged[keep].sum())


def off_image_kernel_case(G, P, seed, bases):
    """the step kernel itself: after one dense one-round rg_submit32c of RG_EV_NONE rows the state alone says which workgroups left the 32-bit body, so
    rg_wide_body_workgroups must equal the number of 64-group blocks that hold a flagged group -> that number"""
    rng = np.random.default_rng(seed)
    t = engine.Table(G, P, 1 % P)
    if P > abi.MAX_COMPACT_CLUSTER:
        t.set_compact_any_cluster(True)
    st = random_state(G, P, rng)
    blocks = (G + 63) // 64
    hot = rng.random(blocks) < 0.4                             # the blocks that get out-of-image groups, a few each
    pick = hot[np.arange(G) // 64] & (rng.random(G) < 0.05)
    kind = rng.integers(0, 4, G)
    st.current_term[:] = np.where(pick & (kind == 0), LIM + rng.integers(0, 9, G), st.current_term)
    st.role_epoch[:] = np.where(pick & (kind == 1), LIM, st.role_epoch)
    st.elected_term[:] = np.where(pick & (kind == 2), (1 << 40), st.elected_term)
    m = st.peer_match_index.reshape(G, P - 1)
    m[:, 0] = np.where(pick & (kind == 3), LIM + 5, m[:, 0])   # (counts only where the group is prepared: the model says so, and so must the kernel)
    base = np.zeros(G, np.int64)
    if bases:
        # a base just below the group's smallest non-zero index keeps it in the image; one AT epoch.index (no image) or above it takes it out
        low = np.where(st.epoch_index > 0, st.epoch_index, 1)
        base = np.where(rng.random(G) < 0.3, low - 1, 0)
        base = np.where(hot[np.arange(G) // 64] & (rng.random(G) < 0.03), st.epoch_index + rng.integers(0, 2, G), base)
        t.set_index_base(base)
    t.load_state(st)
    got = t.scan(capacity=0)
    flagged = (got.bits & abi.SCAN_OFF_IMAGE) != 0
    assert np.array_equal(flagged, off_image(t.read_state(), t.index_base())), "the scan and the model disagree"
    want = len(np.unique(np.flatnonzero(flagged) // 64))
    assert 0 < want < blocks, (want, blocks)
    t.wide_body_workgroups(reset=True)
    t.submit32c(engine.pack32(abi.Batch(1, G), index_base=base if bases else None))
    wide = t.wide_body_workgroups()
    t.close()
    assert wide == want, "%d workgroups took the 64-bit body, the scan flags groups in %d blocks" % (wide, want)
    return want


# ---- state by list ------------------------------------------------------------------------------------------------------------------------------------------
def _everything(t):
    out = dict(state=t.read_state(), timers=t.timers_read(), base=t.index_base())
    out["ok"], out["fail"], out["recent"] = t.health_read()
    if t.option(abi.OPT_DEVICE_IN_FLIGHT):
        out["in_flight"] = t.in_flight_read()
    return out


def same_tables(a, b, where):
    same_state(a["state"], b["state"], where)
    for k in a:
        if k != "state":
            assert np.array_equal(a[k], b[k]), (where, k)


def read_list_case(G, P, seed):
    """a permutation with repeats, and the empty list"""
    rng = np.random.default_rng(seed)
    t = engine.Table(G, P, 1 % P)
    t.load_state(random_state(G, P, rng))
    whole = t.read_state()
    gids = np.concatenate([rng.permutation(G)[: G - G // 3], rng.integers(0, G, G // 3)]).astype(np.uint32)
    rng.shuffle(gids)
    assert len(np.unique(gids)) < len(gids)
    same_state(t.read_state_list(gids), rows_of(whole, gids), "G=%d" % G)
    same_state(t.read_state_list(gids[:1]), rows_of(whole, gids[:1]), "one group")
    assert t.read_state_list(np.zeros(0, np.uint32)).count == 0
    t.close()
    return len(gids)


def _busy_table(G, P, seed, in_flight):
    """state, armed timers, health statistics and in-flight counts that a load must reset for the listed groups and for no other"""
    rng = np.random.default_rng(seed)
    t = engine.Table(G, P, 1 % P)
    if in_flight:
        t.set_device_in_flight(True)
    t.load_state(random_state(G, P, rng))
    t.timers_configure(900, 300, seed)
    t.timers_arm(1000)
    n = min(G, 2048)                                           # failures for a sample of the leaders' followers: fail / recent / rejection move
    t.health_failure(rng.integers(0, G, n), rng.integers(0, P, n), rng.integers(0, 4, n), 1234)
    if in_flight:
        t.in_flight_set(rng.integers(1, 9, (G, P - 1)))
    return t


def load_list_case(G, P, k, seed, in_flight=True):
    """k scattered groups loaded by list into one table and one at a time by rg_load_state into its twin: afterwards every column of the two is identical over
    the WHOLE table — state, timers, health and in-flight counts — and differs from before in the listed groups only"""
    a, b = _busy_table(G, P, seed, in_flight), _busy_table(G, P, seed, in_flight)
    before = _everything(a)
    same_tables(before, _everything(b), "twins before")
    rng = np.random.default_rng(seed + 1)
    gids = rng.choice(G, size=k, replace=False).astype(np.uint32)
    new = random_state(k, P, rng)
    a.load_state_list(new, gids)
    for i, g in enumerate(gids):
        b.load_state(rows_of(new, [i]), first=int(g))
    after = _everything(a)
    same_tables(after, _everything(b), "G=%d k=%d" % (G, k))
    same_state(rows_of(after["state"], gids), new, "the listed groups")
    rest = np.setdiff1d(np.arange(G), gids)
    same_state(rows_of(after["state"], rest), rows_of(before["state"], rest), "the other groups")
    assert np.all(after["timers"][gids] == 0) and np.array_equal(after["timers"][rest], before["timers"][rest])
    if in_flight:
        assert not after["in_flight"][gids].any() and after["in_flight"][rest].all()
    # a load that fails validation at its LAST row leaves the table bit-identical
    bad = random_state(k, P, rng)
    bad.role[k - 1] = 7
    try:
        a.load_state_list(bad, gids)
        raise AssertionError("a role of 7 was loaded")
    except engine.EngineError as e:
        assert "rg_load_state_list: group %d role 7" % gids[k - 1] in str(e), e
    same_tables(_everything(a), after, "after a refused load")
    a.close()
    b.close()
    return k


def _refused(t, call, text):
    rc = call()
    msg = engine.lib().rg_last_error(t._h).decode()
    assert rc == -1 and text in msg, (rc, msg, text)


def list_refusals_case(G=200, P=3):
    t = engine.Table(G, P)
    L = engine.lib()
    st = random_state(4, P, np.random.default_rng(1))
    s = st.as_struct()
    whole = _everything(t)

    def gl(*g):
        a = np.array(g, np.uint32)
        return a, a.ctypes.data
    a, p = gl(1, 2, G, 3)
    _refused(t, lambda: L.rg_read_state_list(t._h, 4, p, C.byref(s)), "gid[2] = %d" % G)
    _refused(t, lambda: L.rg_load_state_list(t._h, 4, p, C.byref(s)), "gid[2] = %d" % G)
    a, p = gl(5, 9, 7, 9)
    _refused(t, lambda: L.rg_load_state_list(t._h, 4, p, C.byref(s)), "gid[1] and gid[3] both name group 9")
    big = np.zeros(G + 1, np.uint32)
    _refused(t, lambda: L.rg_read_state_list(t._h, G + 1, big.ctypes.data, C.byref(s)), "%d groups listed, the table has %d" % (G + 1, G))
    _refused(t, lambda: L.rg_load_state_list(t._h, G + 1, big.ctypes.data, C.byref(s)), "%d groups listed, the table has %d" % (G + 1, G))
    a, p = gl(0, 1, 2, 3)
    _refused(t, lambda: L.rg_read_state_list(t._h, 4, None, C.byref(s)), "gid is NULL")
    _refused(t, lambda: L.rg_read_state_list(t._h, 4, p, None), "dst or one of its columns is NULL")
    _refused(t, lambda: L.rg_load_state_list(t._h, 4, p, None), "src or one of its columns is NULL")
    for field, value, text in (("voted_for", P, "group 13 node slot out of range"), ("role", -1, "group 13 role -1")):
        bad = random_state(4, P, np.random.default_rng(2))
        getattr(bad, field)[2] = value
        bs = bad.as_struct()
        a, p = gl(11, 12, 13, 14)
        _refused(t, lambda: L.rg_load_state_list(t._h, 4, p, C.byref(bs)), "rg_load_state_list: " + text)
    bad = random_state(4, P, np.random.default_rng(3))
    bad.run_count[1], bad.run_start[4], bad.first_index[1], bad.last_index[1] = 1, 5, 6, 9
    bs = bad.as_struct()
    _refused(t, lambda: L.rg_load_state_list(t._h, 4, p, C.byref(bs)), "group 12 runs do not span [first,last]")
    assert L.rg_read_state_list(t._h, 0, None, None) == 0 and L.rg_load_state_list(t._h, 0, None, None) == 0
    same_tables(_everything(t), whole, "after the refusals")
    t.close()


# ---- refusals of rg_scan ------------------------------------------------------------------------------------------------------------------------------------
def scan_refusals_case(G=200, P=3, launches=True):
    """every refusal of the header, before any launch; launches=True: ... and the next scan equals the model"""
    t = engine.Table(G, P)
    L = engine.lib()
    summary, gids = np.zeros(abi.SCAN_SUMMARY, np.uint64), np.zeros(8, np.uint32)

    def res(**kw):
        return abi.CScanResult(**dict(dict(bits=None, list=gids.ctypes.data, list_capacity=8, summary=summary.ctypes.data), **kw))

    def qry(**kw):
        return abi.CScanQuery(**kw)
    ok_q, ok_r = qry(), res()
    for q, r, text in ((None, ok_r, "NULL query or result"), (ok_q, None, "NULL query or result"), (ok_q, res(summary=None), "summary is required"),
                       (ok_q, res(list=None), "a NULL list with a capacity of 8"), (qry(reserved=1), ok_r, "reserved is 1"),
                       (qry(any=1 << 16), ok_r, "a bit above 15"), (qry(all=1 << 31), ok_r, "a bit above 15"), (qry(none=0x10000), ok_r, "a bit above 15"),
                       (qry(backlog=-1), ok_r, "backlog -1 outside"), (qry(backlog=(1 << 62) + 1), ok_r, "backlog"), (qry(lag=-5), ok_r, "lag -5 outside"),
                       (qry(lag=(1 << 62) + 1), ok_r, "lag")):
        for memspace in (abi.MEM_HOST, abi.MEM_DEVICE):
            _refused(t, lambda: L.rg_scan(t._h, None if q is None else C.byref(q), None if r is None else C.byref(r), memspace), text)
    _refused(t, lambda: L.rg_scan(t._h, C.byref(ok_q), C.byref(ok_r), 7), "unknown memspace 7")
    assert L.rg_scan(None, C.byref(ok_q), C.byref(ok_r), abi.MEM_HOST) == -1
    if launches:
        edge = qry(backlog=1 << 62, lag=1 << 62, any=0xFFFF)     # (the ends of the ranges are inside them)
        t._check(L.rg_scan(t._h, C.byref(edge), C.byref(res(list=None, list_capacity=0)), abi.MEM_HOST))
        t.load_state(random_state(G, P, np.random.default_rng(5)))
        q = dict(any=abi.SCAN_LEADER, backlog=3, lag=4, now=9)
        check_scan(scan_host(t, q, G), model_of(t, **q), G, "after the refusals")
    t.close()
