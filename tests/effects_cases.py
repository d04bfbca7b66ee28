"""Cases for rg_effects32 (include/raftgpu.h, "what a launch asks the host to do, as lists"): the log writes, the commit advances and the RG_NEED_HOST cells of
the compact outcome rows a launch left, compacted on the device. Shared by tests/test_effects_gpu.py (an MI355X) and tests/devemu/emu_cases_effects.py (the host
emulation of the kernels, small sizes).

The LAYOUT is held bit for bit against model() below, a numpy restatement of the header's contract: layout_case() makes synthetic rows (every row carries its own
cell index in commit_index: a misplaced item shows; what the call must not read carries every mark) and runs the call over them, twice. The DECISIONS are the
oracle's: decisions_case() is the stream of sparse_rounds_cases (rows held to the oracle exactly as there) through one of three routes, and a consumer that reads
ONLY the three lists, and row[cell] for the cells they name, must reconstruct what the walk over every unpacked row finds."""
import ctypes as C
import types

import numpy as np

from rafting_amd import abi, engine
from tests import sparse_rounds_cases as X
from tests.helpers import compare_states

FILL = 0xAB
LISTS = ("log_list", "commit_list", "attention")
LOG = abi.F_LOG_APPEND | abi.F_LOG_TRUNC
MARKS = LOG | abi.F_COMMIT | (abi.NEED_HOST << abi.F_STATUS_SHIFT)


# ---- the model: the header's contract in numpy ----------------------------------------------------------------------------------------------------------------
def model(capacity, max_rounds, n, R, gid, row):
    """row [D * C] (abi.OUT32_DT), the n and R of the run, gid [C] or None -> SimpleNamespace(log_list, commit_list, attention): every item, in the stated order"""
    Cc, D = int(capacity), int(max_rounds)
    rw = np.asarray(row, abi.OUT32_DT)[: D * Cc].reshape(D, Cc)[:R, :n]
    gid = np.arange(Cc, dtype=np.uint32) if gid is None else np.asarray(gid, np.uint32)
    at = np.arange(R, dtype=np.uint32)[:, None] * np.uint32(Cc) + np.arange(n, dtype=np.uint32)[None, :]
    flags = rw["flags"]

    def cells(sel):                                              # (np.nonzero walks row-major: ascending cell)
        r, i = np.nonzero(sel)
        out = np.zeros(len(r), abi.ROUTE_ITEM_DT)
        out["cell"], out["gid"] = at[r, i], gid[i]
        return out
    w = types.SimpleNamespace(log_list=cells((flags & LOG) != 0), attention=cells(abi.flags_status(flags) == abi.NEED_HOST))
    com = (flags & abi.F_COMMIT) != 0
    i = np.flatnonzero(com.any(axis=0))
    last = (R - 1 - np.argmax(com[::-1, i], axis=0)) if len(i) else np.zeros(0, np.int64)
    w.commit_list = np.zeros(len(i), abi.COMMIT_ITEM_DT)
    w.commit_list["cell"], w.commit_list["gid"] = at[last, i], gid[i]
    w.commit_list["commit_index"], w.commit_list["flags"] = rw["commit_index"][last, i], flags[last, i]
    return w


def check_effects(got, want, where):
    """rg_effects32's outputs (images over FILL bytes; engine.Table.effects' namespace) against the model's, bit for bit, and FILL wherever the contract says NOT
    TOUCHED"""
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)      # noqa: E731
    counts = [len(want.log_list), len(want.commit_list), len(want.attention), 0]
    assert list(got.counts) == counts, (where, list(got.counts), counts)
    for name, cap in zip(LISTS, (got.log_capacity, got.commit_capacity, got.attention_capacity)):
        have, ref = getattr(got, name), getattr(want, name)
        k = min(len(ref), cap)
        assert np.array_equal(have[:k], ref[:k]), "%s: %s" % (where, name)
        assert np.all(raw(have)[k:] == FILL), "%s: %s beyond what the list holds was written" % (where, name)


def same_bytes(a, b, where):
    for name in LISTS + ("counts",):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), "%s: %s differs between two runs" % (where, name)


def effects_device(t, row, capacity, max_rounds, gid=None, count=None, rounds=None, log_capacity=None, commit_capacity=None, attention_capacity=None):
    """engine.Table.effects' twin in RG_MEM_DEVICE: every column in device memory (outputs over FILL bytes), one asynchronous run, one sync, read back"""
    Cc, D = int(capacity), int(max_rounds)
    up = lambda a, dt: engine.DeviceBuffer.from_host(t, np.ascontiguousarray(a, dtype=dt))      # noqa: E731
    ins = dict(row=up(row, abi.OUT32_DT))
    if gid is not None:
        ins["gid"] = up(gid, np.uint32)
    if count is not None:
        ins["count"] = up([count], np.uint32)
    if rounds is not None:
        ins["rounds"] = up([rounds], np.uint32)
    e = abi.CEffectsIn()
    e.capacity, e.max_rounds = Cc, D
    for k, v in ins.items():
        setattr(e, k, v.ptr)
    cap = lambda c, most: int(most if c is None else c)      # noqa: E731
    lcap, ccap, acap = cap(log_capacity, Cc * D), cap(commit_capacity, Cc), cap(attention_capacity, Cc * D)
    shape = dict(log_list=(abi.ROUTE_ITEM_DT, lcap), commit_list=(abi.COMMIT_ITEM_DT, ccap), attention=(abi.ROUTE_ITEM_DT, acap), counts=(np.uint32, 4))
    outs = {k: engine.DeviceBuffer.from_host(t, np.full(max(int(k_), 1) * np.dtype(dt).itemsize, FILL, np.uint8)) for k, (dt, k_) in shape.items()}
    o = abi.CEffects()
    o.log_capacity, o.commit_capacity, o.attention_capacity = lcap, ccap, acap
    for k, v in outs.items():
        setattr(o, k, v.ptr if k not in LISTS or shape[k][1] else None)                  # (a capacity of 0 comes with a NULL list)
    t.effects_device(e, o)
    t.sync()
    out = types.SimpleNamespace(log_capacity=lcap, commit_capacity=ccap, attention_capacity=acap)
    for k, (dt, k_) in shape.items():
        setattr(out, k, outs[k].to_host(dt, max(int(k_), 1)))
    for x in list(ins.values()) + list(outs.values()):
        x.free()
    return out


def synthetic(rng, Cc, D, n, R, fill):
    """rows for a batch of R x n cells at [D][Cc]: commit_index is the cell index, the other numbers are random; each of RG_F_LOG_APPEND, RG_F_LOG_TRUNC and
    RG_F_COMMIT on a share `fill` of the cells, the status RG_NEED_HOST on the same share, RG_F_WIDE_VALUES on half of them, the rest of the flags random. What the
    launch would not have written — cells at or beyond R or n — carries every mark: a read beyond n or R shows in the lists"""
    cells = Cc * D
    row = np.zeros(cells, abi.OUT32_DT)
    row["resp_term"], row["log_from"], row["commit_index"] = rng.integers(0, 1 << 31, cells), rng.integers(-(1 << 31), 1 << 31, cells), np.arange(cells, dtype=np.uint32).view(np.int32)
    flags = rng.integers(0, 1 << 16, cells).astype(np.uint32) & ~np.uint32(LOG | abi.F_COMMIT)
    for bit in (abi.F_LOG_APPEND, abi.F_LOG_TRUNC, abi.F_COMMIT):
        flags |= (rng.random(cells) < fill).astype(np.uint32) * np.uint32(bit)
    status = rng.integers(0, 8, cells).astype(np.uint32)
    status[rng.random(cells) < fill] = abi.NEED_HOST
    flags |= status << np.uint32(abi.F_STATUS_SHIFT)
    inside = np.zeros((D, Cc), bool)
    inside[:R, :n] = True
    flags[~inside.reshape(-1)] = MARKS
    row["flags"] = flags
    return row


def layout_case(Cc, D, seed, device=False):
    """one shape (C, D) on a table of C + 64 groups: fills 0, 2 %, 30 % and 100 %; n and R through the words (below C and D, clamped from above and from below,
    n = 0) and without them; gid NULL and a strictly ascending list; list capacities of every possible item, 0 (with NULL lists), half of the items, a few more
    than the items; every call made twice with identical bytes -> the number of calls"""
    G = Cc + 64
    t = engine.Table(G, 3)
    rng = np.random.default_rng(seed)
    listed = np.sort(rng.choice(G, Cc, replace=False)).astype(np.uint32)
    n1, R1 = max(Cc - 37, 1), max(D - 1, 1)
    # (fill, count word, rounds word, a gid list, the capacities)
    runs = [(0.3, None, None, False, "all"), (0.02, n1, R1, True, "none"), (1.0, n1, None, False, "half"), (0.0, None, R1, True, "more"),
            (0.3, Cc + 7, 0, True, "half"), (0.3, 0, D + 3, False, "more"), (0.02, 1, R1, True, "all"), (1.0, Cc, D, True, "more"), (0.02, None, None, True, "half")]
    seen = dict(cap0=0, below=0, above=0, short_n=0, short_R=0, empty=0)
    for c, (fill, count, rounds, with_gid, caps) in enumerate(runs):
        n, R = Cc if count is None else min(count, Cc), D if rounds is None else min(max(rounds, 1), D)
        gid = listed if with_gid else None
        row = synthetic(rng, Cc, D, n, R, fill)
        want = model(Cc, D, n, R, gid, row)
        k = (len(want.log_list), len(want.commit_list), len(want.attention))
        cap = {"all": (None,) * 3, "none": (0,) * 3, "half": tuple(x // 2 for x in k), "more": tuple(x + 5 for x in k)}[caps]
        kw = dict(gid=gid, count=count, rounds=rounds, log_capacity=cap[0], commit_capacity=cap[1], attention_capacity=cap[2])
        where = "C %d, D %d, run %d (%s memory)" % (Cc, D, c, "device" if device else "host")
        first = None
        for again in (0, 1):
            out = effects_device(t, row, Cc, D, **kw) if device else t.effects(row, Cc, D, fill=FILL, **kw)
            check_effects(out, want, "%s, call %d" % (where, again))
            if first is not None:
                same_bytes(first, out, where)
            first = out
        seen["cap0"] += caps == "none" and sum(k) > 0
        seen["below"] += caps == "half" and min(k) > 1
        seen["above"] += caps == "more" and min(k) > 0
        seen["short_n"] += 0 < n < Cc and min(k) > 0
        seen["short_R"] += R < D and min(k) > 0
        seen["empty"] += sum(k) == 0
    assert all(v > 0 for k_, v in seen.items() if k_ != "short_R" or D > 1), seen
    t.close()
    return 2 * len(runs)


# ---- real decisions: the lists against the walk over every row --------------------------------------------------------------------------------------------------
def full_walk(got, R, n, gid):
    """what a host finds by looking at every row: the loop of IngressFlusher::apply over the rg_outcome32_unpack'ed columns [R][n] -> (the log writes in order:
    (gid, round, truncate, append, log_from); {gid: the commit index its last commit advance left}; the RG_NEED_HOST cells (round, gid))"""
    flags = got.reply["flags"]
    writes, commits, attention = [], {}, []
    for at in np.flatnonzero(abi.has_logfx(flags)):
        r, i, f = int(at) // n, int(at) % n, int(flags[at])
        if f & LOG:
            writes.append((int(gid[i]), r, bool(f & abi.F_LOG_TRUNC), bool(f & abi.F_LOG_APPEND), int(got.logfx["log_from"][at])))
        if f & abi.F_COMMIT:
            commits[int(gid[i])] = int(got.logfx["commit_index"][at])
        if (f >> abi.F_STATUS_SHIFT) & 0xFF == abi.NEED_HOST:
            attention.append((r, int(gid[i])))
    return writes, commits, attention


def from_lists(fx, row, Cc, wide=None):
    """the same three answers for a consumer that reads ONLY the lists and row[cell] of the cells they name (`row` as the launch laid it out, stride Cc; wide: the
    overflow columns for a cell flagged RG_F_WIDE_VALUES)"""
    k = [min(int(c), cap) for c, cap in zip(fx.counts[:3], (fx.log_capacity, fx.commit_capacity, fx.attention_capacity))]
    assert k == [int(c) for c in fx.counts[:3]], "a list was too short for its items"
    writes, commits = [], {}
    for cell, g in fx.log_list[: k[0]].tolist():
        f = int(row["flags"][cell])
        lf = int(row["log_from"][cell]) if not f & abi.F_WIDE_VALUES else int(wide.logfx["log_from"][cell])
        writes.append((g, cell // Cc, bool(f & abi.F_LOG_TRUNC), bool(f & abi.F_LOG_APPEND), lf))
    for cell, g, ci, f in fx.commit_list[: k[1]].tolist():
        assert g not in commits and f & abi.F_COMMIT
        commits[g] = ci if not f & abi.F_WIDE_VALUES else int(wide.logfx["commit_index"][cell])
    return writes, commits, [(cell // Cc, g) for cell, g in fx.attention[: k[2]].tolist()]


def _dense(t, G):
    """the launch of sparse_rounds_cases.lead() as a dense R x G batch: the same rows at the listed groups, RG_EV_NONE everywhere else"""
    b = abi.Batch(t.R, G)
    for name in ("head", "ab", "cd"):
        getattr(b, name).reshape(t.R, G)[:, t.rows] = getattr(t.batch, name).reshape(t.R, t.n)
    b.entry_terms, b.entry_count = t.batch.entry_terms, t.batch.entry_count
    return b


def decisions_case(G, P, seed, launches, route, device_resident=False):
    """The fuzz stream of sparse_rounds_cases (launch k: fill FILLS[k % 5], depth DEPTHS[(k // 5) % 5]), its rows held to the oracle as standalone_rounds_case /
    rounds_tick_case hold them, through one route:
      "dense":  rg_submit32c on the dense R x G batch (gid NULL), rg_effects32 in host memory over its R x G rows;
      "sparse": rg_submit32c_sparse_rounds, rg_effects32 in host memory over its R x n rows with the launch's gid list;
      "tick":   a rg_tick2_create_sparse_rounds tick with rg_effects32(RG_MEM_DEVICE) queued behind rg_tick2_launch, reading the tick's own count and depth words,
                one wait at the end.
    Every launch: what from_lists() makes of the three lists equals what full_walk() finds in every row. -> (truncations, groups that committed in more than one
    round of a launch, RG_NEED_HOST cells) seen"""
    gpu, orc, shadow, fz, rng, rng2 = X._tables(G, P, seed)
    RMAX = X.RMAX
    tick = pins = None
    if route == "tick":
        tick = engine.Tick2(gpu, RMAX, entry_cap=8 * G * RMAX, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=device_resident, sparse_cap=G,
                            sparse_rounds=True)
        shape = dict(log_list=(abi.ROUTE_ITEM_DT, RMAX * G), commit_list=(abi.COMMIT_ITEM_DT, G), attention=(abi.ROUTE_ITEM_DT, RMAX * G), counts=(np.uint32, 4))
        cols, pins = {}, []
        for name, (dt, k_) in shape.items():
            cols[name], p = engine.pinned_like(gpu, np.zeros(k_, dt))
            pins.append(p)
        e, o = abi.CEffectsIn(), abi.CEffects()
        e.capacity, e.max_rounds, e.gid, e.count, e.rounds, e.row = G, RMAX, tick.rows.gid, tick.rows.count, tick.rows.rounds, tick.io.row
        o.log_capacity, o.commit_capacity, o.attention_capacity = RMAX * G, G, RMAX * G
        for name in shape:
            setattr(o, name, cols[name].ctypes.data)
    fired_g, fired_e = np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    truncs = multi = need = 0
    for k in range(launches):
        t = X.lead(orc, fz, rng, G, k, fired_g, fired_e)
        where = "%s, launch %d (%d rounds x %d rows)" % (route, k, t.R, t.n)
        fired_g, fired_e = t.expired[0], t.expired[1]
        if route != "tick" and not t.n:
            continue
        if route == "tick":
            if t.n:
                hb, fl = X._traffic(rng2, t.n, P)
                tick.refill(t.batch, t.nows, heartbeat=hb, in_flight=fl.T.reshape(-1))
            else:
                tick.refill(abi.Batch(1, 0, gid=np.zeros(0, np.uint32)), t.nows)
            for a in cols.values():
                a.view(np.uint8)[:] = FILL
            tick.launch()
            gpu.effects_device(e, o)
            tick.wait()
            fx = types.SimpleNamespace(log_capacity=RMAX * G, commit_capacity=G, attention_capacity=RMAX * G, **{name: np.array(a, copy=True) for name, a in cols.items()})
            laid, stride, wide = tick._get(tick.row, abi.OUT32_DT, RMAX * G), G, None
            raw = tick.outcome32()
            check_effects(fx, model(G, RMAX, t.n, t.R, tick._get(tick.gid, np.uint32, G), laid), where)
            if not t.n:
                eg, epg, ng = tick.expired()
                assert ng == t.expired[2] and np.array_equal(eg, t.expired[0]), where
                continue
        elif route == "dense":
            full = gpu.submit32c(_dense(t, G), fill=FILL)
            fx = gpu.effects(full.row, G, t.R, fill=FILL)
            laid, stride, wide = full.row, G, full.wide
            raw = abi.Outcome32(t.R * t.n, wide=True)
            pick = lambda a: np.ascontiguousarray(a.reshape(t.R, G)[:, t.rows]).reshape(-1)      # noqa: E731
            raw.row, raw.persist = pick(full.row), pick(full.persist)
            raw.wide.reply, raw.wide.logfx, raw.wide.persist = pick(full.wide.reply), pick(full.wide.logfx), pick(full.wide.persist)
            check_effects(fx, model(G, t.R, G, t.R, None, laid), where)
        else:
            raw = gpu.submit32c_sparse_rounds(t.batch, fill=FILL)
            fx = gpu.effects(raw.row, t.n, t.R, gid=t.gid, fill=FILL)
            laid, stride, wide = raw.row, t.n, raw.wide
            check_effects(fx, model(t.n, t.R, t.n, t.R, t.gid, laid), where)
        # the rows as the launch wrote them (before any repair), every one of them looked at ...
        got, _ = engine.unpack32(raw, t.R, t.n, t.start.role_epoch[t.rows])
        writes, commits, attention = full_walk(got, t.R, t.n, t.gid)
        # ... against the lists alone (the rows of a dense launch outside the list are RG_EV_NONE: they ask for nothing)
        assert from_lists(fx, laid, stride, wide) == (writes, commits, attention), where
        com = ((got.reply["flags"] & abi.F_COMMIT) != 0).reshape(t.R, t.n)
        truncs += sum(1 for w in writes if w[2])
        multi += int(np.count_nonzero(com.sum(axis=0) > 1))
        need += len(attention)
        # the rows against the oracle, as the sparse-rounds cases hold them
        bad = X._check_rows(gpu, shadow, t, raw, where, fold=route == "tick")
        if route == "tick":
            eg, epg, ng = tick.expired()
            assert ng == t.expired[2] and np.array_equal(eg, t.expired[0]) and np.array_equal(epg, t.expired[1]), where
            assert np.array_equal(gpu.timers_read(), orc.timers_read()), where
            orc.replicate(gid=t.gid, heartbeat=hb, in_flight=fl)
            if len(bad):
                gpu.replicate(gid=t.gid[bad], heartbeat=hb[bad], in_flight=fl[bad])
        compare_states(orc.read_state(), gpu.read_state(), where)
    if tick is not None:
        tick.close()
        for p in pins:
            p.free()
    for x in (gpu, orc, shadow):
        x.close()
    return truncs, multi, need


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def refusal_structs(G, D=4):
    """a correct call on host memory -> (rows, lists, the arrays that back them)"""
    cols = dict(gid=np.arange(G, dtype=np.uint32), count=np.array([G], np.uint32), rounds=np.array([D], np.uint32), row=np.zeros(D * G, abi.OUT32_DT),
                o_log_list=np.zeros(8, abi.ROUTE_ITEM_DT), o_commit_list=np.zeros(8, abi.COMMIT_ITEM_DT), o_attention=np.zeros(8, abi.ROUTE_ITEM_DT),
                o_counts=np.zeros(4, np.uint32))
    e, o = abi.CEffectsIn(), abi.CEffects()
    e.capacity, e.max_rounds = G, D
    for f in ("gid", "count", "rounds", "row"):
        setattr(e, f, cols[f].ctypes.data)
    o.log_capacity, o.commit_capacity, o.attention_capacity = 8, 8, 8
    for f in LISTS + ("counts",):
        setattr(o, f, cols["o_" + f].ctypes.data)
    return e, o, cols


def refusals_case(G=512, launches=True):
    """every refusal of the header's list answers -1 with a message, before any launch. launches=True (not the lane-serial emulation, whose kernels cannot run):
    the next call's result equals the model, which shows that nothing was launched by any refused call. (The emulation cannot tell pageable from page-locked
    memory: that refusal is checked on the GPU, tests/test_effects_gpu.py.)"""
    t = engine.Table(G, 3)
    L = engine.lib()

    def refused(text, memspace=abi.MEM_HOST, **change):
        e, o, cols = refusal_structs(G)
        for k, v in change.items():
            if k == "bad_gid":
                cols["gid"][v] = G
            else:
                setattr(e if k.startswith("e_") else o, k[2:], v)
        rc = L.rg_effects32(t._h, C.byref(e), C.byref(o), memspace)
        err = L.rg_last_error(t._h)
        assert rc == -1 and text in err, (change, rc, err)
    e, o, cols = refusal_structs(G)
    assert L.rg_effects32(t._h, None, C.byref(o), abi.MEM_HOST) == -1 and b"NULL rows or lists" in L.rg_last_error(t._h)
    assert L.rg_effects32(t._h, C.byref(e), None, abi.MEM_HOST) == -1 and b"NULL rows or lists" in L.rg_last_error(t._h)
    assert L.rg_effects32(None, C.byref(e), C.byref(o), abi.MEM_HOST) == -1
    refused(b"row is required", e_row=None)
    refused(b"counts is required", o_counts=None)
    refused(b"a NULL log_list with a capacity of 8", o_log_list=None)
    refused(b"a NULL commit_list with a capacity of 8", o_commit_list=None)
    refused(b"a NULL attention list with a capacity of 8", o_attention=None)
    refused(b"capacity 0 outside", e_capacity=0)
    refused(b"capacity %d outside" % (G + 1), e_capacity=G + 1)
    refused(b"max_rounds 0 outside", e_max_rounds=0)
    refused(b"max_rounds %d outside" % (1 << 24), e_max_rounds=1 << 24)
    refused(b"%d x %d cells" % (G, 1 << 23), e_max_rounds=1 << 23)                       # (512 x 2^23 = 2^32)
    refused(b"unknown memspace", memspace=7)
    refused(b"gid[5] = %d, the table has %d groups" % (G, G), bad_gid=5)
    if launches:
        rng = np.random.default_rng(5)
        n, R = G - 100, 3
        row = synthetic(rng, G, 4, n, R, 0.2)
        gid = np.arange(G, dtype=np.uint32)
        check_effects(t.effects(row, G, 4, gid=gid, count=n, rounds=R, fill=FILL), model(G, 4, n, R, gid, row), "after the refusals")
    t.close()
