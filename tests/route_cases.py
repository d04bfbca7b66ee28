"""Cases for rg_route32 (include/raftgpu.h, "routing a decided batch back to arrival order"): what a launch left over a batch rg_assemble32 made — outcome rows
at [round][row], persist rows under RG_F_PERSIST, the send table — back at the index of the event each cell answers, and as the three lists. Shared by
tests/test_route_gpu.py (an MI355X) and tests/devemu/emu_cases_route.py (the host emulation of the kernels, small tables).

The LAYOUT is held bit for bit against model() below, a numpy restatement of the header's contract that works from `origin`: layout_case() assembles the inputs
of assemble_cases.layout_inputs on the device, fills the outcome columns with synthetic rows (every row carries its own cell index in commit_index: a misrouted
row shows) and routes them. The DECISIONS are the oracle's: routed_tick_case() is assemble_cases.assembled_tick_case's loop (in_flight=True:
in_flight_cases.assembled_case's) with rg_route32(RG_MEM_DEVICE) queued behind tick.launch() and nothing in between; the tick's own columns are checked against the
oracle exactly as there, and the routed columns must equal a gather of those checked columns by origin, name exactly the oracle's conversions and the oracle's
sends."""
import ctypes as C
import types

import numpy as np

from rafting_amd import abi, engine
from tests import assemble_cases as A
from tests import in_flight_cases as I
from tests import sparse_rounds_cases as X
from tests.helpers import compare_states
from tests.sparse_tick_cases import assert_untouched

FILL = A.FILL
FILL32 = FILL * 0x01010101
NONE, EXPIRED = abi.ROUTE_NONE, abi.ORIGIN_EXPIRED
SENT = (abi.SEND_APPEND, abi.SEND_SNAPSHOT, abi.SEND_NEED_HOST)
LISTS = ("persist_list", "attention", "send_list")


# ---- the model: the header's contract in numpy ----------------------------------------------------------------------------------------------------------------
def model(capacity, max_rounds, n, R, m, e, gid, origin, row, persist32, send=None, followers=0):
    """the [D][C] columns of a decided batch (flat arrays) and the m and e of the assembler's run -> SimpleNamespace(cell[m], placed[m], row[m], has_persist[m],
    persist32[m], the same five with the prefix expired_ [e], persist_list, attention, send_list (all items), send_offset [followers + 1] or None)"""
    Cc, D = capacity, max_rounds
    grid = lambda a, dt: np.asarray(a, dt)[: D * Cc].reshape(D, Cc)[:R, :n].reshape(-1)      # noqa: E731
    o, rw, pw = grid(origin, np.uint32), grid(row, abi.OUT32_DT), grid(persist32, abi.PERSIST32_DT)
    at = (np.arange(R, dtype=np.uint32)[:, None] * np.uint32(Cc) + np.arange(n, dtype=np.uint32)[None, :]).reshape(-1)      # ascending
    gid = np.asarray(gid, np.uint32)
    per, att = (rw["flags"] & abi.F_PERSIST) != 0, abi.flags_status(rw["flags"]) == abi.NEED_HOST
    w = types.SimpleNamespace()

    def side(prefix, sel, idx, k):
        cell, placed, has = np.full(k, NONE, np.uint32), np.zeros(k, bool), np.zeros(k, bool)
        r_, p_ = np.zeros(k, abi.OUT32_DT), np.zeros(k, abi.PERSIST32_DT)
        cell[idx[sel]], placed[idx[sel]], r_[idx[sel]] = at[sel], True, rw[sel]
        has[idx[sel & per]], p_[idx[sel & per]] = True, pw[sel & per]
        for name, v in (("cell", cell), ("placed", placed), ("row", r_), ("has_persist", has), ("persist32", p_)):
            setattr(w, prefix + name, v)
    low = (o & np.uint32(0x7FFFFFFF)).astype(np.int64)
    side("", ((o & EXPIRED) == 0) & (low < m), low, m)
    side("expired_", ((o & EXPIRED) != 0) & (low < e), low, e)

    def items(dt, first, rows):
        out = np.zeros(len(first), dt)
        out[dt.names[0]], out["gid"] = first, gid[rows]
        return out
    w.persist_list, w.attention = items(abi.ROUTE_ITEM_DT, at[per], at[per] % Cc), items(abi.ROUTE_ITEM_DT, at[att], at[att] % Cc)
    w.send_list, w.send_offset = np.zeros(0, abi.SEND_ITEM_DT), None
    if send is not None:
        kind = np.asarray(send, abi.SEND_DT)["kind"][: followers * Cc].reshape(followers, Cc)[:, :n]
        j, i = np.nonzero(np.isin(kind, SENT))                                           # follower-major, rows ascending
        w.send_list = items(abi.SEND_ITEM_DT, i.astype(np.uint32), i)
        w.send_offset = np.concatenate([[0], np.cumsum(np.bincount(j, minlength=followers))]).astype(np.uint32)
    return w


def check_routed(got, want, m, e, where):
    """rg_route32's outputs (images over FILL bytes; engine.Assembler.route's namespace) against the model's, bit for bit, and FILL wherever the contract says NOT
    TOUCHED"""
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)      # noqa: E731
    for prefix, k in (("", m), ("expired_", e)):
        cell = getattr(got, prefix + "cell")
        if cell is None:
            continue
        assert np.array_equal(cell[:k], getattr(want, prefix + "cell")), "%s: %scell" % (where, prefix)
        assert np.all(cell[k:] == FILL32), "%s: %scell beyond the run's entries was written" % (where, prefix)
        for name, mask in (("row", "placed"), ("persist32", "has_persist")):
            img, ref, on = raw(getattr(got, prefix + name)), raw(getattr(want, prefix + name)), getattr(want, prefix + mask)
            assert np.array_equal(img[:k][on], ref[on]), "%s: %s%s" % (where, prefix, name)
            assert np.all(img[:k][~on] == FILL) and np.all(img[k:] == FILL), "%s: %s%s: an entry that is not to be written was written" % (where, prefix, name)
    sends = want.send_offset is not None
    counts = [len(want.persist_list), len(want.attention), len(want.send_list), 0]
    assert list(got.counts) == counts, (where, list(got.counts), counts)
    for name, cap in zip(LISTS, (got.persist_capacity, got.attention_capacity, got.send_capacity)):
        have, ref = getattr(got, name), getattr(want, name)
        k = min(len(ref), cap)
        assert np.array_equal(have[:k], ref[:k]), "%s: %s" % (where, name)
        assert np.all(raw(have)[k:] == FILL), "%s: %s beyond what the list holds was written" % (where, name)
    if sends:
        assert np.array_equal(got.send_offset, want.send_offset), (where, got.send_offset, want.send_offset)
    else:
        assert np.all(got.send_offset == FILL32), "%s: send_offset was written without a send table" % where


def route_device(asm, gid, count, rounds, origin, row, persist32, capacity, max_rounds, arrival_capacity, expired_capacity=None, send=None,
                 persist_capacity=None, attention_capacity=None, send_capacity=None):
    """engine.Assembler.route's twin in RG_MEM_DEVICE: every column in device memory (outputs over FILL bytes), one asynchronous run, one sync, read back"""
    t = asm.table
    Cc, D, F = int(capacity), int(max_rounds), t.cluster - 1
    up = lambda a, dt: engine.DeviceBuffer.from_host(t, np.ascontiguousarray(a, dtype=dt))      # noqa: E731
    ins = dict(gid=up(gid, np.uint32), count=up([count], np.uint32), rounds=up([rounds], np.uint32), origin=up(origin, np.uint32), row=up(row, abi.OUT32_DT),
               persist32=up(persist32, abi.PERSIST32_DT))
    if send is not None:
        ins.update(send=up(send, abi.SEND_DT), send_head=up(np.zeros(max(Cc, 1), abi.SEND_HEAD_DT), abi.SEND_HEAD_DT))
    d = abi.CDecided()
    d.capacity, d.max_rounds = Cc, D
    for k, v in ins.items():
        setattr(d, k, v.ptr)
    cap = lambda c, most: int(most if c is None else c)      # noqa: E731
    pcap, acap, scap = cap(persist_capacity, Cc * D), cap(attention_capacity, Cc * D), cap(send_capacity, F * Cc if send is not None else 0)
    shape = dict(cell=(np.uint32, arrival_capacity), row=(abi.OUT32_DT, arrival_capacity), persist32=(abi.PERSIST32_DT, arrival_capacity),
                 persist_list=(abi.ROUTE_ITEM_DT, pcap), attention=(abi.ROUTE_ITEM_DT, acap), send_list=(abi.SEND_ITEM_DT, scap), send_offset=(np.uint32, F + 1),
                 counts=(np.uint32, 4))
    if expired_capacity is not None:
        shape.update(expired_cell=(np.uint32, expired_capacity), expired_row=(abi.OUT32_DT, expired_capacity), expired_persist32=(abi.PERSIST32_DT, expired_capacity))
    outs = {k: engine.DeviceBuffer.from_host(t, np.full(max(int(n), 1) * np.dtype(dt).itemsize, FILL, np.uint8)) for k, (dt, n) in shape.items()}
    r = abi.CRouted()
    r.arrival_capacity, r.expired_capacity = int(arrival_capacity), int(expired_capacity or 0)
    r.persist_capacity, r.attention_capacity, r.send_capacity = pcap, acap, scap
    for k, v in outs.items():
        setattr(r, k, v.ptr if k not in LISTS or shape[k][1] else None)               # (a capacity of 0 comes with a NULL list)
    asm.route_device(d, r)
    t.sync()
    out = types.SimpleNamespace(expired_cell=None, expired_row=None, expired_persist32=None, persist_capacity=pcap, attention_capacity=acap, send_capacity=scap)
    for k, (dt, n) in shape.items():
        setattr(out, k, outs[k].to_host(dt, max(int(n), 1)))
    for x in list(ins.values()) + list(outs.values()):
        x.free()
    return out


def run_counts(kw):
    """the m and e the assembler reads from the inputs of one case of assemble_cases.layout_inputs"""
    m = min(len(kw["gid"]) if kw.get("count") is None else int(kw["count"]), len(kw["gid"]))
    ex = kw.get("expired")
    e = 0 if ex is None or int(ex[2]) == 0xFFFFFFFF else min(int(ex[2]), len(ex[0]))
    return m, e


def synthetic(rng, Cc, D, n, R, F):
    """outcome columns and a send table for a batch of R x n cells at [D][Cc]: every row carries its cell index in commit_index, RG_F_PERSIST on about 10 % and the
    status RG_NEED_HOST on about 2 % of the rows, kinds over all five values. What the launch would not have written — cells at or beyond R or n, send rows at or
    beyond n — carries RG_F_PERSIST, RG_NEED_HOST and RG_SEND_APPEND: a read beyond n or R shows in the lists"""
    cells = Cc * D
    row, per = np.zeros(cells, abi.OUT32_DT), np.zeros(cells, abi.PERSIST32_DT)
    row["resp_term"], row["log_from"], row["commit_index"] = rng.integers(0, 1 << 31, cells), rng.integers(-(1 << 31), 1 << 31, cells), np.arange(cells)
    flags = (rng.integers(0, 1 << 16, cells).astype(np.uint32) & ~np.uint32(abi.F_PERSIST)) | (rng.random(cells) < 0.1).astype(np.uint32) * np.uint32(abi.F_PERSIST)
    status = rng.integers(0, 8, cells).astype(np.uint32)
    status[rng.random(cells) < 0.02] = abi.NEED_HOST
    flags |= status << np.uint32(abi.F_STATUS_SHIFT)
    inside = np.zeros((D, Cc), bool)
    inside[:R, :n] = True
    flags[~inside.reshape(-1)] = abi.F_PERSIST | (abi.NEED_HOST << abi.F_STATUS_SHIFT)
    row["flags"] = flags
    for f in ("term", "voted_for", "role"):
        per[f] = rng.integers(-(1 << 31), 1 << 31, cells)
    per["role_epoch"] = rng.integers(0, 1 << 32, cells, dtype=np.uint64)
    send = np.zeros(F * Cc, abi.SEND_DT)
    for f in ("prev_index", "prev_term", "last_index"):
        send[f] = rng.integers(0, 1 << 40, F * Cc)
    kind = rng.integers(0, 5, (F, Cc)).astype(np.uint32)
    kind[:, n:] = abi.SEND_APPEND
    send["kind"], send["count"] = kind.reshape(-1), rng.integers(0, 50, F * Cc)
    return row, per, send


def layout_case(G, seed, device=False, events=None, P=3):
    """every input of assemble_cases.layout_inputs() assembled on ONE assembler, its cells given synthetic rows, routed TWICE, against the model. The list
    capacities go round from one input to the next: every possible item, 0 (with NULL lists), half of the items, a few more than the items; every other input comes
    without a send table. One more input, the whole capacity at D = 64, makes the count arrays long enough for a wider span"""
    t = engine.Table(G, P)
    F = P - 1
    cases = A.layout_inputs(G, seed, events)
    rng = np.random.default_rng(seed + 1000)
    # one input of this module's own: the whole capacity at D = 64 — the shape at which a wavefront covers more than 64 rows of a round (rg_route.hpp: route_span)
    wide = rng.integers(0, G, G).astype(np.uint32)
    wide_head, wide_abcd = A._rows(rng, G)
    cases.append(("the whole capacity at depth 64", dict(gid=wide, head=wide_head, abcd=wide_abcd, capacity=G, max_rounds=64)))
    asm = engine.Assembler(t, max(len(kw["gid"]) for _, kw in cases), max_expired=max(G // 50, 64))
    seen = dict(m0=0, R1=0, RD=0, none=0, all_deferred=0, cap0=0, below=0, above=0, no_send=0, expired=0, persist=0, attention=0)
    for c, (name, kw) in enumerate(cases):
        Cc, D = kw["capacity"], kw["max_rounds"]
        got = A.assemble_device(asm, **kw) if device else asm.assemble(fill=FILL, **kw)
        A.check_layout(got, A.model(G, **kw), Cc, D, "%s (%d groups)" % (name, G))
        n, R = got.n, got.R
        m, e = run_counts(kw)
        row, per, send = synthetic(rng, Cc, D, n, R, F)
        if c % 2:
            send = None
        want = model(Cc, D, n, R, m, e, got.gid, got.origin, row, per, send, F)
        counts = (len(want.persist_list), len(want.attention), len(want.send_list))
        caps = {0: (None,) * 3, 1: (0,) * 3, 2: tuple(k // 2 for k in counts), 3: tuple(k + 5 for k in counts)}[(c // 2) % 4]
        ecap = None if kw.get("expired") is None else len(kw["expired"][0])
        args = dict(gid=got.gid, count=n, rounds=R, origin=got.origin, row=row, persist32=per, capacity=Cc, max_rounds=D, arrival_capacity=len(kw["gid"]),
                    expired_capacity=ecap, send=send, persist_capacity=caps[0], attention_capacity=caps[1], send_capacity=caps[2])
        for again in (0, 1):
            out = route_device(asm, **args) if device else asm.route(fill=FILL, **args)
            check_routed(out, want, m, e, "%s (%d groups, %s memory, run %d)" % (name, G, "device" if device else "host", again))
        groups = np.asarray(kw["gid"][:m], np.int64)
        gone = np.setdiff1d(groups[groups < G], groups[want.placed]) if m else np.zeros(0)
        seen["m0"] += m == 0
        seen["R1"] += R == 1 and D > 1 and n > 0
        seen["RD"] += R == D and D > 1
        seen["none"] += int(np.count_nonzero(~want.placed))
        seen["all_deferred"] += len(gone)
        seen["cap0"] += caps[0] == 0 and counts[0] > 0
        seen["below"] += caps[0] is not None and 0 < caps[0] < counts[0]
        seen["above"] += caps[0] is not None and caps[0] > counts[0]
        seen["no_send"] += send is None
        seen["expired"] += int(np.count_nonzero(want.expired_placed))
        seen["persist"] += counts[0]
        seen["attention"] += counts[1]
    assert all(v > 0 for v in seen.values()), seen
    asm.close()
    t.close()
    return len(cases)


# ---- assemble -> tick -> route, in lockstep with the oracle ------------------------------------------------------------------------------------------------------
class _Columns:
    """the routed columns of a tick loop: page-locked host memory, or device memory (resident=True), FILL bytes before every run"""

    def __init__(self, table, shape, resident):
        self.table, self.shape, self.resident, self.pins, self.bufs = table, shape, resident, [], {}
        for k, (dt, n) in shape.items():
            nbytes = max(int(n), 1) * np.dtype(dt).itemsize
            if resident:
                self.bufs[k] = engine.DeviceBuffer(table, nbytes)
            else:
                a, p = engine.pinned_like(table, np.zeros(nbytes, np.uint8))
                self.bufs[k] = a
                self.pins.append(p)
        self.blank = {k: np.full(max(int(n), 1) * np.dtype(dt).itemsize, FILL, np.uint8) for k, (dt, n) in shape.items()}

    def ptr(self, k):
        return self.bufs[k].ptr if self.resident else self.bufs[k].ctypes.data

    def clear(self):
        for k, b in self.bufs.items():
            if self.resident:
                self.table._check(engine.lib().rg_copy_to_device(self.table._h, b.ptr, self.blank[k].ctypes.data, self.blank[k].nbytes))
            else:
                b[:] = FILL

    def read(self, k):
        dt, n = self.shape[k]
        return self.bufs[k].to_host(dt, max(int(n), 1)) if self.resident else np.array(self.bufs[k].view(dt)[: max(int(n), 1)], copy=True)

    def close(self):
        for b in self.bufs.values():
            if self.resident:
                b.free()
        for p in self.pins:
            p.free()


def routed_tick_case(G, seed, ticks, P=5, device_resident=False, in_flight=False, expect_all=True):
    """rg_assemble32 -> rg_tick2_launch -> rg_route32, all RG_MEM_DEVICE on the table's stream with nothing in between, tick after tick, in lockstep with the oracle.
    The tick's own columns are held to the oracle as assemble_cases.assembled_tick_case holds them (in_flight=True: a table with RG_OPT_DEVICE_IN_FLIGHT, as
    in_flight_cases.assembled_case and its model hold them). The routed columns must equal model() over those checked columns; the persist list names exactly the
    oracle's conversions of the tick, in order; the send list names exactly the (follower, row) pairs whose kind the oracle (the in-flight model) makes a send.
    Rows repaired after RG_NEED_HOST are left out of the two comparisons with the oracle (the device stopped their groups); their share is capped at 2 % of the
    listed rows, asserted. -> (rows decided, send items, send rows)"""
    gpu, orc, shadow, fz, rng, rng2 = X._tables(G, P, seed)
    if in_flight:
        gpu.set_device_in_flight(True)
    sends_model = I.Model(G, P, 2 % P) if in_flight else None
    RMAX, F = X.RMAX, P - 1
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
    # the outbound half: the tick's columns in, the routed columns out. persist_list is short on purpose (the count may exceed it); the others hold every item
    pcap = max(G // 32, 1)
    cols = _Columns(gpu, dict(cell=(np.uint32, RMAX * G), row=(abi.OUT32_DT, RMAX * G), persist32=(abi.PERSIST32_DT, RMAX * G), expired_cell=(np.uint32, G),
                              expired_row=(abi.OUT32_DT, G), expired_persist32=(abi.PERSIST32_DT, G), persist_list=(abi.ROUTE_ITEM_DT, pcap),
                              attention=(abi.ROUTE_ITEM_DT, RMAX * G), send_list=(abi.SEND_ITEM_DT, F * G), send_offset=(np.uint32, P), counts=(np.uint32, 4)),
                    device_resident)
    decided = asm.decided_for_tick(tick, origin.ctypes.data)
    routed = abi.CRouted()
    routed.arrival_capacity, routed.expired_capacity, routed.persist_capacity, routed.attention_capacity, routed.send_capacity = RMAX * G, G, pcap, RMAX * G, F * G
    for k in cols.shape:
        setattr(routed, k, cols.ptr(k))
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    seen = dict(deep=0, ragged=0, fired_rows=0, conversions=0, sends=0, no_send=0, short_list=0)
    rows = listed = left_out = send_items = send_rows = 0
    for k in range(ticks):
        if in_flight and k % I.SET_EVERY == I.SET_AT:
            sends_model.randomise(rng2)
            gpu.in_flight_set(sends_model.counts)
        t = A.lead(orc, fz, rng, G, k, fired_g, fired_e, P)
        where = "tick %d (%d rounds x %d rows)" % (k, t.R, t.n)
        before = I._snapshot(gpu) if in_flight else gpu.read_state()
        lg, lh, la, at_r, at_i = A.arrival_log(t, rng)
        m, e = len(lg), len(fired_g)
        log_gid[:m], log_head[:m], log_abcd[:m], log_count[0] = lg, lh, la, m
        if t.n and t.b32.entry_count:
            tick._put(tick.entry_terms, t.b32.entry_terms[: t.b32.entry_count])
        tick.now[:] = [X.now_of(k, r) for r in range(RMAX)]
        if t.n and not in_flight:
            hb, fl = X._traffic(rng2, t.n, P)
            tick._put(tick.heartbeat, hb)
            for j in range(F):
                tick._put(tick.in_flight, np.ascontiguousarray(fl.T[j]), at=j * G)
        origin[:] = 0xABABABAB
        cols.clear()
        asm.run_device(arr, out)
        tick.launch()
        asm.route_device(decided, routed)
        tick.wait()
        gpu.sync()
        # ---- the tick's own columns, as assembled_tick_case / in_flight_cases.assembled_case check them
        tick.n, tick.depth = int(tick.count[0]), int(tick.depth_now[0])
        assert (tick.n, tick.depth) == (t.n, t.R), (where, tick.n, tick.depth)
        assert not t.n or np.array_equal(tick._get(tick.gid, np.uint32, t.n), t.gid), where
        assert list(stats) == [m + e, 0, 0, 0], (where, list(stats))
        if t.n:
            want_origin = np.full((t.R, t.n), A.NONE, np.uint32)
            want_origin[at_r, at_i] = np.arange(m, dtype=np.uint32)
            fr = np.flatnonzero(np.isin(t.rows, fired_g))
            want_origin[0, fr] = A.EXPIRED | np.searchsorted(fired_g, t.gid[fr]).astype(np.uint32)
            assert np.array_equal(origin.reshape(RMAX, G)[: t.R, : t.n], want_origin), where
            seen["fired_rows"] += len(fr)
        # (read before any repair: what the route saw)
        t_row, t_per = tick._get(tick.row, abi.OUT32_DT, RMAX * G), tick._get(tick.persist32, abi.PERSIST32_DT, RMAX * G)
        t_send, t_gid = tick._get(tick.send, abi.SEND_DT, F * G), tick._get(tick.gid, np.uint32, G)
        ok = np.ones(t.n, dtype=bool)
        if in_flight:
            bad = I._after_tick(gpu, orc, shadow, sends_model, tick, t, where, before)
            ok[bad] = False
            eg, epg = t.expired[0], t.expired[1]
        else:
            bad = X._check_rows(gpu, shadow, t, tick.outcome32(), where, fold=True) if t.n else np.zeros(0, dtype=np.int64)
            ok[bad] = False
            eo, epo, no = t.expired
            eg, epg, ng = tick.expired()
            assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo), where
            assert np.array_equal(gpu.timers_read(), orc.timers_read()), where
            for a, c in zip(gpu.health_read(), orc.health_read()):
                assert np.array_equal(a, c), where
            if t.n:
                (hg, sg), (ho, so) = tick.sends(), orc.replicate(gid=t.gid, heartbeat=hb, in_flight=fl)
                if len(bad):
                    gpu.replicate(gid=t.gid[bad], heartbeat=hb[bad], in_flight=fl[bad])
                for f in ("term", "leader_commit", "epoch_index", "epoch_term", "role_epoch", "is_leader"):
                    assert np.array_equal(hg[f][ok], ho[f][ok]), (where, f)
                for f in ("prev_index", "prev_term", "last_index", "count", "kind"):
                    assert np.array_equal(sg[f][ok], so[f][ok]), (where, f)
                rd, ro = tick.readiness(), orc.ready(t.nows[-1], 1, 60)[t.rows]
                assert np.array_equal(rd[ok], ro[ok]), where
            after = gpu.read_state()
            compare_states(orc.read_state(), after, where)
            assert_untouched(before, after, ~t.pick, where)
        # ---- the routed columns: a gather of the checked columns by origin ...
        got = types.SimpleNamespace(persist_capacity=pcap, attention_capacity=RMAX * G, send_capacity=F * G, **{name: cols.read(name) for name in cols.shape})
        want = model(G, RMAX, t.n, t.R, m, e, t_gid, origin, t_row, t_per, t_send, F)
        check_routed(got, want, m, e, where)
        if t.n:
            assert np.array_equal(want.cell, (at_r * G + at_i).astype(np.uint32)) and want.placed.all() and want.expired_placed.all(), where
            # ... the persist list: exactly the oracle's conversions of the tick, round-major
            flags = t.want.reply["flags"].reshape(t.R, t.n)
            r_, i_ = np.nonzero(((flags & abi.F_PERSIST) != 0) & ok[None, :])
            mine = want.persist_list[ok[want.persist_list["cell"] % G]]
            assert np.array_equal(mine["cell"], (r_ * G + i_).astype(np.uint32)) and np.array_equal(mine["gid"], t.gid[i_]), (where, "persist list")
            # ... the send list: exactly the (follower, row) pairs whose kind is a send — for the oracle (the in-flight model: _after_tick held the tick's send rows to it)
            kind = t_send["kind"].reshape(F, G)[:, : t.n]
            if not in_flight:
                assert np.array_equal(kind.T[ok], so["kind"][ok]), where
            for j in range(F):
                mine = want.send_list[want.send_offset[j]: want.send_offset[j + 1]]
                mine = mine[ok[mine["row"]]]
                rows_j = np.flatnonzero(np.isin(kind[j], SENT) & ok)
                assert np.array_equal(mine["row"], rows_j) and np.array_equal(mine["gid"], t.gid[rows_j]), (where, "send list", j)
            listed_rows = want.attention["cell"] % G
            assert set(listed_rows.tolist()) <= set(bad.tolist()) or not len(listed_rows), (where, "an attention item names a row that needed no repair")
            seen["conversions"] += len(r_)
            seen["sends"] += len(want.send_list)
            seen["no_send"] += int(np.count_nonzero(~np.isin(kind, SENT)))
            seen["short_list"] += len(want.persist_list) > pcap
            send_items, send_rows = send_items + len(want.send_list), send_rows + F * t.n
        seen["deep"] += t.n > 0 and t.R >= 3
        seen["ragged"] += t.n % 64 != 0
        rows += t.R * t.n
        listed += t.n
        left_out += len(bad)
        fired_g, fired_e = eg, epg
    if expect_all:
        assert all(v > 0 for v in seen.values()), seen
    assert left_out * 50 <= listed, "%d of %d listed rows were left out of the comparisons with the oracle (cap: 2 %%)" % (left_out, listed)
    asm.close()
    tick.close()
    cols.close()
    for p in pins:
        p.free()
    for x in (gpu, orc, shadow):
        x.close()
    return rows, send_items, send_rows


def in_flight_case(G=1000, seed=77, ticks=20, P=5, device_resident=False):
    """routed_tick_case on a table with RG_OPT_DEVICE_IN_FLIGHT: the host fills no per-row column at all, and the send list is sparse — an untriggered row's sends
    are RG_SEND_NONE"""
    rows, items, of = routed_tick_case(G, seed, ticks, P=P, device_resident=device_resident, in_flight=True, expect_all=False)
    assert 0 < items < of // 2, (items, of)
    return rows


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def refusal_structs(G, D=4, m=16, e=4, P=3):
    """a correct call on host memory for the run of assemble_cases.refusal_structs -> (decided, routed, the arrays that back them)"""
    F = P - 1
    cols = dict(gid=np.arange(G, dtype=np.uint32), count=np.array([m], np.uint32), rounds=np.ones(1, np.uint32), origin=np.full(D * G, NONE, np.uint32),
                row=np.zeros(D * G, abi.OUT32_DT), persist32=np.zeros(D * G, abi.PERSIST32_DT), send_head=np.zeros(G, abi.SEND_HEAD_DT), send=np.zeros(F * G, abi.SEND_DT),
                o_cell=np.zeros(m, np.uint32), o_row=np.zeros(m, abi.OUT32_DT), o_persist32=np.zeros(m, abi.PERSIST32_DT), o_expired_cell=np.zeros(e, np.uint32),
                o_expired_row=np.zeros(e, abi.OUT32_DT), o_expired_persist32=np.zeros(e, abi.PERSIST32_DT), o_persist_list=np.zeros(8, abi.ROUTE_ITEM_DT),
                o_attention=np.zeros(8, abi.ROUTE_ITEM_DT), o_send_list=np.zeros(8, abi.SEND_ITEM_DT), o_send_offset=np.zeros(P, np.uint32), o_counts=np.zeros(4, np.uint32))
    d, r = abi.CDecided(), abi.CRouted()
    d.capacity, d.max_rounds = G, D
    for f in ("gid", "count", "rounds", "origin", "row", "persist32", "send_head", "send"):
        setattr(d, f, cols[f].ctypes.data)
    r.arrival_capacity, r.expired_capacity, r.persist_capacity, r.attention_capacity, r.send_capacity = m, e, 8, 8, 8
    for f in ("cell", "row", "persist32", "expired_cell", "expired_row", "expired_persist32", "persist_list", "attention", "send_list", "send_offset", "counts"):
        setattr(r, f, cols["o_" + f].ctypes.data)
    return d, r, cols


def refusals_case(G=64, launches=True):
    """every refusal of the header's list answers -1 with a message, before any launch. launches=False (the lane-serial emulation, whose kernels cannot run): only
    what needs no earlier run of the assembler — everything but the comparison with the last run's shape. launches=True: those too, and nothing was launched by any
    refused call: the assembler's next run and its route equal the models. (The emulation cannot tell pageable from page-locked memory: that refusal is checked on
    the GPU, tests/test_route_gpu.py.)"""
    t = engine.Table(G, 3)
    L = engine.lib()
    asm = engine.Assembler(t, 16, max_expired=4)

    def refused(text, memspace=abi.MEM_HOST, **change):
        d, r, cols = refusal_structs(G)
        for k, v in change.items():
            setattr(d if k.startswith("d_") else r, k[2:], v)
        rc = L.rg_route32(asm._h, C.byref(d), C.byref(r), memspace)
        err = L.rg_last_error(t._h)
        assert rc == -1 and text in err, (change, rc, err)

    def shape_independent():
        for col in ("gid", "count", "rounds", "origin", "row", "persist32"):
            refused(b"of the decided batch are required", **{"d_" + col: None})
        for col in ("cell", "row", "persist32", "counts", "persist_list", "attention"):
            refused(b"of the routed columns are required", **{"r_" + col: None})
        for col in ("send_offset", "send_list"):
            refused(b"a send table needs send_offset", **{"r_" + col: None})
        for col in ("send_head", "send"):
            refused(b"send_head and send, or as neither", **{"d_" + col: None})
        for col in ("expired_cell", "expired_row", "expired_persist32"):
            refused(b"all three or none", **{"r_" + col: None})
        refused(b"capacity 0 outside", d_capacity=0)
        refused(b"capacity %d outside" % (G + 1), d_capacity=G + 1)
        refused(b"max_rounds 0 outside 1 .. 64", d_max_rounds=0)
        refused(b"max_rounds 65 outside 1 .. 64", d_max_rounds=65)
        refused(b"unknown memspace", memspace=7)
        d, r, cols = refusal_structs(G)
        assert L.rg_route32(asm._h, None, C.byref(r), abi.MEM_HOST) == -1 and L.rg_route32(asm._h, C.byref(d), None, abi.MEM_HOST) == -1
        assert L.rg_route32(None, C.byref(d), C.byref(r), abi.MEM_HOST) == -1
    shape_independent()
    refused(b"has not run yet")
    if launches:
        a, b, keep = A.refusal_structs(G)
        assert L.rg_assemble32(asm._h, C.byref(a), C.byref(b), abi.MEM_HOST) == 0
        shape_independent()
        refused(b"the assembler's last run had %d and 4" % G, d_capacity=G - 1)
        refused(b"the assembler's last run had %d and 4" % G, d_max_rounds=5)
        refused(b"an arrival capacity of 15, the assembler's last run had 16", r_arrival_capacity=15)
        refused(b"an expired capacity of 5, the assembler's last run had 4", r_expired_capacity=5)
        # nothing was launched: a run and its route on the same assembler are the models'
        rng = np.random.default_rng(5)
        kw = dict(gid=np.array([9, 3, 9, 300, 1, 9, 9], np.uint32), head=np.zeros(7, abi.HEAD_DT), abcd=np.zeros(7, abi.QUAD32_DT), capacity=G, max_rounds=2,
                  expired=(np.array([3, 40], np.uint32), np.array([7, 8], np.uint32), 2))
        got = asm.assemble(fill=FILL, **kw)
        A.check_layout(got, A.model(G, **kw), G, 2, "after the refusals")
        row, per, send = synthetic(rng, G, 2, got.n, got.R, 2)
        out = asm.route(got.gid, got.n, got.R, got.origin, row, per, G, 2, 7, expired_capacity=2, send=send, fill=FILL)
        check_routed(out, model(G, 2, got.n, got.R, 7, 2, got.gid, got.origin, row, per, send, 2), 7, 2, "after the refusals")
    asm.close()
    t.close()
