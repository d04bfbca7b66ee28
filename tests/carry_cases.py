"""Cases for the carry of an assembler (include/raftgpu.h, "carrying deferred events into the next run"): rg_assembler_carry_enable / _reset / _read and
rg_route32_carry. Shared by tests/test_carry_gpu.py (an MI355X) and tests/devemu/emu_cases_carry.py (the host emulation of the kernels, small tables).

The oracle of the feature is the header's own host recipe: carry_model() concatenates the carry and the log, hands them to assemble_cases.model — today's
contract, a host that prepends the deferred rows by hand — and relabels the ids; what the run deferred, in S order, is the next carry. chain_case() drives ONE
assembler through a chain of runs (both overflows, a long segment, tickets beyond the list, an untrusted fired list, bad gids, a drain) and holds every run's
columns, both carries and the routed columns to the models, bit for bit, with FILL sentinels wherever the contract says NOT TOUCHED."""
import ctypes as C
import types

import numpy as np

from rafting_amd import abi, engine
from tests import assemble_cases as A
from tests import route_cases as R

FILL, FILL32 = A.FILL, R.FILL32
NONE, EXPIRED, CARRIED = A.NONE, A.EXPIRED, abi.ASM_CARRIED
WENT_CARRIED, SPILLED = abi.ROUTE_CARRIED, abi.ROUTE_SPILLED
LONG = 66                                                   # events of the chain's hot group: more than rg::ASM_SMALL = 64, the radix-select path


def empty_carry():
    return np.zeros(0, np.uint32), np.zeros(0, abi.HEAD_DT), np.zeros(0, abi.QUAD32_DT)


# ---- the model: today's contract with the carry prepended to the log, ids relabelled ----------------------------------------------------------------------------
def carry_model(groups, carry, gid, head, abcd, capacity, max_rounds, carry_capacity, expired=None, count=None):
    """carry = (gid, head, abcd) of the q slots the run reads -> assemble_cases.model's namespace with origin / deferred relabelled (a carried slot c is
    RG_ASM_CARRIED | c, an arrival k is k again), stats[3] = the spilled events, and: carry (the next one), q, m, e, spilled, from_carry (per slot of the next
    carry: the slot of the old carry it came from, -1 for a ticket or an arrival)"""
    cg, ch, ca = carry
    q = len(cg)
    gid = np.asarray(gid, np.uint32)
    m = min(len(gid) if count is None else int(count), len(gid))
    lg = np.concatenate([np.asarray(cg, np.uint32), gid[:m]])
    lh = np.concatenate([np.asarray(ch, abi.HEAD_DT), np.asarray(head, abi.HEAD_DT)[:m]])
    la = np.concatenate([np.asarray(ca, abi.QUAD32_DT), np.asarray(abcd, abi.QUAD32_DT)[:m]])
    w = A.model(groups, lg, lh, la, capacity, max_rounds, expired=expired)

    def relabel(ids):
        ids = np.asarray(ids, np.uint32).copy()
        log = ((ids & EXPIRED) == 0) & (ids != NONE)
        low = ids[log].astype(np.int64)
        ids[log] = np.where(low < q, CARRIED | low, low - q).astype(np.uint32)
        return ids
    raw = w.deferred
    e = 0 if expired is None or int(expired[2]) == 0xFFFFFFFF else min(int(expired[2]), len(expired[0]))
    kept = raw[:carry_capacity]
    ng, nh, na = np.zeros(len(kept), np.uint32), np.zeros(len(kept), abi.HEAD_DT), np.zeros(len(kept), abi.QUAD32_DT)
    from_carry = np.full(len(kept), -1, np.int64)
    for p, i in enumerate(kept.tolist()):
        if i & EXPIRED:
            j = i & 0x7FFFFFFF
            ng[p], nh[p] = expired[0][j], (A.TIMEOUT_HDR, expired[1][j])
        else:
            ng[p], nh[p], na[p] = lg[i], lh[i], la[i]
            from_carry[p] = i if i < q else -1
    w.origin, w.deferred = relabel(w.origin), relabel(raw)
    w.spilled = len(raw) - len(kept)
    w.stats[3] = w.spilled
    w.carry, w.from_carry, w.q, w.m, w.e = (ng, nh, na), from_carry, q, m, e
    return w


def route_model(w, capacity, max_rounds, carry_capacity, row, persist32, send=None, followers=0):
    """the routed columns of rg_route32_carry for the run carry_model() described: route_cases.model (an id with bit 30 set is routed nowhere) + the carried
    columns + the deferred entries of the three cell columns"""
    o = np.zeros(capacity * max_rounds, np.uint32)
    o.reshape(max_rounds, capacity)[: w.R, : w.n] = w.origin
    r = R.model(capacity, max_rounds, w.n, w.R, w.m, w.e, w.gid, o, row, persist32, send, followers)
    # a view of the carried ids as if they were arrivals of a log of q events
    oc = np.where((o & 0xC0000000) == CARRIED, o & np.uint32(0x3FFFFFFF), NONE).astype(np.uint32)
    c = R.model(capacity, max_rounds, w.n, w.R, w.q, 0, w.gid, oc, row, persist32)
    r.carried_cell, r.carried_placed, r.carried_row, r.carried_has_persist, r.carried_persist32 = c.cell, c.placed, c.row, c.has_persist, c.persist32
    for p, i in enumerate(w.deferred.tolist()):
        went = (WENT_CARRIED | p) if p < carry_capacity else SPILLED
        if i & EXPIRED:
            r.expired_cell[i & 0x7FFFFFFF] = went
        elif i & CARRIED:
            r.carried_cell[i & 0x3FFFFFFF] = went
        else:
            r.cell[i] = went
    return r


def check_carried(got, want, q, where):
    """the carried columns of rg_route32_carry against route_model's, FILL wherever the contract says NOT TOUCHED; the rest: route_cases.check_routed"""
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)      # noqa: E731
    assert np.array_equal(got.carried_cell[:q], want.carried_cell), "%s: the carried cell" % where
    assert np.all(got.carried_cell[q:] == FILL32), "%s: a carried cell at or beyond q was written" % where
    for name, mask in (("carried_row", "carried_placed"), ("carried_persist32", "carried_has_persist")):
        img, ref, on = raw(getattr(got, name)), raw(getattr(want, name)), getattr(want, mask)
        assert np.array_equal(img[:q][on], ref[on]), "%s: %s" % (where, name)
        assert np.all(img[:q][~on] == FILL) and np.all(img[q:] == FILL), "%s: %s: an entry that is not to be written was written" % (where, name)


def route_device(asm, gid, count, rounds, origin, row, persist32, capacity, max_rounds, arrival_capacity, expired_capacity=None, send=None, carried=True):
    """route_cases.route_device's twin for rg_route32_carry (carried=False: plain rg_route32 over the same buffers): every column in device memory over FILL bytes"""
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
    pcap, acap, scap = Cc * D, Cc * D, F * Cc if send is not None else 0
    shape = dict(cell=(np.uint32, arrival_capacity), row=(abi.OUT32_DT, arrival_capacity), persist32=(abi.PERSIST32_DT, arrival_capacity),
                 persist_list=(abi.ROUTE_ITEM_DT, pcap), attention=(abi.ROUTE_ITEM_DT, acap), send_list=(abi.SEND_ITEM_DT, scap), send_offset=(np.uint32, F + 1),
                 counts=(np.uint32, 4))
    if expired_capacity is not None:
        shape.update(expired_cell=(np.uint32, expired_capacity), expired_row=(abi.OUT32_DT, expired_capacity), expired_persist32=(abi.PERSIST32_DT, expired_capacity))
    cshape = dict(carried_cell=(np.uint32, asm.carry), carried_row=(abi.OUT32_DT, asm.carry), carried_persist32=(abi.PERSIST32_DT, asm.carry)) if carried else {}
    blank = lambda dt, n: engine.DeviceBuffer.from_host(t, np.full(max(int(n), 1) * np.dtype(dt).itemsize, FILL, np.uint8))      # noqa: E731
    outs = {k: blank(dt, n) for k, (dt, n) in list(shape.items()) + list(cshape.items())}
    r = abi.CRouted()
    r.arrival_capacity, r.expired_capacity = int(arrival_capacity), int(expired_capacity or 0)
    r.persist_capacity, r.attention_capacity, r.send_capacity = pcap, acap, scap
    for k in shape:
        setattr(r, k, outs[k].ptr if k not in R.LISTS or shape[k][1] else None)
    rc = None
    if carried:
        rc = abi.CRoutedCarry()
        rc.capacity, rc.cell, rc.row, rc.persist32 = asm.carry, outs["carried_cell"].ptr, outs["carried_row"].ptr, outs["carried_persist32"].ptr
    asm.route_device(d, r, carried=rc)
    t.sync()
    out = types.SimpleNamespace(expired_cell=None, expired_row=None, expired_persist32=None, persist_capacity=pcap, attention_capacity=acap, send_capacity=scap)
    for k, (dt, n) in list(shape.items()) + list(cshape.items()):
        setattr(out, k, outs[k].to_host(dt, max(int(n), 1)))
    for x in list(ins.values()) + list(outs.values()):
        x.free()
    return out


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------------------------------
def chain_inputs(G, seed, events=None):
    """the seeded runs of a chain on a table of G groups -> [(name, kwargs of carry_model() / Assembler.assemble() without the carry)], C = max(G // 16, 1): three
    feeding runs at D = 2 — both overflows, a hot group of LONG events (listed: its surplus is carried run after run), tickets of groups beyond the list (carried
    as rows), bad gids, a fired list marked 0xFFFFFFFF —, then empty logs at D = 8: the drain, cut to its length by chain_case"""
    rng = np.random.default_rng(seed)
    Cc = max(G // 16, 1)
    big = G if events is None else events
    hot = 1
    runs = []

    def add(name, gid, D=2, **kw):
        gid = np.asarray(gid, np.uint32)
        head, abcd = A._rows(rng, len(gid))
        runs.append((name, dict(gid=gid, head=head, abcd=abcd, capacity=Cc, max_rounds=D, **kw)))

    def fired(k, lo, hi):
        k = min(k, hi - lo)
        return np.sort(rng.choice(np.arange(lo, hi), k, replace=False)).astype(np.uint32), rng.integers(1, 1 << 20, k).astype(np.uint32)
    g = np.concatenate([rng.integers(0, max(G // 4, 2), big), np.full(LONG, hot)])[rng.permutation(big + LONG)]
    g[3::17], g[5] = G + 7, 0xFFFFFFFF
    eg, ee = fired(max(G // 50, 3), G // 2, G)                                                   # (groups beyond the list: the log's lie below G / 4)
    add("both overflows, a long segment, tickets beyond the list, bad gids", g, expired=(eg, ee, len(eg)))
    eg, ee = fired(max(G // 50, 3), 0, G)
    add("a fired list marked untrusted", rng.integers(0, max(G // 4, 2), max(big // 4, 4)), expired=(eg, ee, 0xFFFFFFFF))
    eg, ee = fired(max(G // 50, 3), 0, G)
    g = rng.integers(0, G, max(big // 8, 4))
    g[::5] = G
    add("a sparse log over all groups, fired tickets", g, expired=(eg, ee, len(eg)))
    for k in range(64):
        add("drain %d" % k, [], D=8)
    return runs


def model_chain(G, runs, carry_capacity):
    """the models of a chain from an empty carry, the drain cut where the model's carry is empty (one empty run beyond it: q = 0 in, q = 0 out) ->
    [(name, kw, model)], the greatest deferred count of a run, the greatest number of runs in a row an event was carried for"""
    carry, age = empty_carry(), np.zeros(0, np.int64)
    out, most, oldest = [], 0, 0
    for name, kw in runs:
        if name.startswith("drain") and len(carry[0]) == 0 and out[-1][0].startswith("drain") and len(out) >= 6:
            break
        w = carry_model(G, carry, carry_capacity=carry_capacity, **kw)
        age = np.where(w.from_carry >= 0, np.append(age, 0)[w.from_carry] + 1, 1)       # (-1, a ticket or an arrival: the appended 0)
        most, oldest = max(most, int(w.stats[1])), max(oldest, int(age.max()) if len(age) else 0)
        out.append((name, kw, w))
        carry = w.carry
    assert len(carry[0]) == 0, "the chain's drain is too short for this carry"
    return out, most, oldest


def _same_carry(got, want, where):
    for a, b, name in zip(got, want, ("gid", "head", "abcd")):
        assert len(a) == len(b) and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), "%s: the carry's %s" % (where, name)


def run_chain(asm, G, chain, carry_capacity, device, seed, routes=True, where=""):
    """one pass of a modelled chain through a carrying assembler whose next carry is empty -> the bytes of everything the device wrote (for the repeat)"""
    t = asm.table
    F = t.cluster - 1
    rng = np.random.default_rng(seed + 1000)
    old = empty_carry()
    seen = dict(spilled=0, carried_placed=0, carried_again=0, ticket_carried=0, went_none=0, runs=0)
    image = []
    for name, kw, w in chain:
        at = "%s%s (%d groups, carry %d, %s memory)" % (where, name, G, carry_capacity, "device" if device else "host")
        Cc, D = kw["capacity"], kw["max_rounds"]
        got = A.assemble_device(asm, **kw) if device else asm.assemble(fill=FILL, **kw)
        A.check_layout(got, w, Cc, D, at)
        _same_carry(asm.carry_read(abi.CARRY_NEXT), w.carry, at + ", the next carry")
        _same_carry(asm.carry_read(abi.CARRY_LAST), old, at + ", the last carry")
        image += [got.gid.tobytes(), got.head.tobytes(), got.abcd.tobytes(), got.origin.tobytes(), got.deferred.tobytes(), got.stats.tobytes()]
        if routes:
            row, per, send = R.synthetic(rng, Cc, D, w.n, w.R, F)
            ecap = None if kw.get("expired") is None else len(kw["expired"][0])
            args = dict(gid=got.gid, count=w.n, rounds=w.R, origin=got.origin, row=row, persist32=per, capacity=Cc, max_rounds=D, arrival_capacity=len(kw["gid"]),
                        expired_capacity=ecap, send=send)
            rw = route_model(w, Cc, D, carry_capacity, row, per, send, F)
            out = route_device(asm, **args) if device else asm.route(fill=FILL, carried=True, **args)
            R.check_routed(out, rw, w.m, w.e, at)
            check_carried(out, rw, w.q, at)
            plain = route_device(asm, carried=False, **args) if device else asm.route(fill=FILL, **args)
            assert list(plain.counts) == list(out.counts), at
            for lst in R.LISTS + ("send_offset",):
                assert np.array_equal(getattr(plain, lst), getattr(out, lst)), "%s: %s differs from plain rg_route32's" % (at, lst)
            assert not np.any((plain.cell[: w.m] & 0x80000000 != 0) & (plain.cell[: w.m] != NONE)), "%s: plain rg_route32 wrote a carry mark" % at
            image += [out.cell.tobytes(), out.carried_cell.tobytes(), out.carried_row.tobytes(), out.carried_persist32.tobytes(), out.persist_list.tobytes()]
            seen["carried_placed"] += int(np.count_nonzero(rw.carried_placed))
            seen["carried_again"] += int(np.count_nonzero((rw.carried_cell & WENT_CARRIED != 0) & (rw.carried_cell < SPILLED)))
            seen["ticket_carried"] += 0 if rw.expired_cell is None else int(np.count_nonzero((rw.expired_cell & WENT_CARRIED != 0) & (rw.expired_cell < SPILLED)))
            seen["went_none"] += int(np.count_nonzero(rw.cell == NONE))
        seen["spilled"] += w.spilled
        seen["runs"] += 1
        old = w.carry
    return image, seen


def chain_case(G, seed, device=False, events=None, P=3, routes=True):
    """the chain of chain_inputs() on ONE assembler at four carry capacities — ample, exactly the greatest deferred count of a run, one less (a spill of 1), and
    1 —, every run against the models; at the ample capacity the whole chain again after two more runs and rg_assembler_carry_reset, with identical bytes; at the
    end rg_assembler_carry_enable of 0, after which the plain outputs equal assemble_cases.model. -> runs made"""
    t = engine.Table(G, P)
    runs = chain_inputs(G, seed, events)
    most_events = max(len(kw["gid"]) for _, kw in runs)
    max_expired = max(len(kw["expired"][0]) for _, kw in runs if kw.get("expired") is not None)
    ample = sum(len(kw["gid"]) + (len(kw["expired"][0]) if kw.get("expired") is not None else 0) for _, kw in runs)
    chain, most, oldest = model_chain(G, runs, ample)
    assert len(chain) >= 6 and oldest >= 3 and most > 1, (len(chain), oldest, most)
    asm = engine.Assembler(t, most_events, max_expired=max_expired, carry=ample)
    total = 0
    first, seen = run_chain(asm, G, chain, ample, device, seed, routes)
    assert seen["spilled"] == 0 and (not routes or all(seen[k] > 0 for k in ("carried_placed", "carried_again", "ticket_carried", "went_none"))), seen
    total += seen["runs"]
    # the drain took as many runs as the model's; two more runs leave a carry behind, the reset empties it, the chain repeats byte for byte
    for name, kw, _ in chain[:2]:
        A.assemble_device(asm, **kw) if device else asm.assemble(fill=FILL, **kw)
    assert len(asm.carry_read(abi.CARRY_NEXT)[0]) > 0
    asm.carry_reset()
    assert len(asm.carry_read(abi.CARRY_NEXT)[0]) == 0
    again, _ = run_chain(asm, G, chain, ample, device, seed, routes, where="after the reset: ")
    assert again == first, "the chain after rg_assembler_carry_reset differs from the first pass"
    for cap, spills in ((most, 0), (most - 1, 1), (1, None)):
        chain_c, _, _ = model_chain(G, runs, cap)
        assert len(chain_c) >= 6
        asm.carry_enable(cap)
        _, seen = run_chain(asm, G, chain_c, cap, device, seed, routes)
        first_spill = ([int(w.spilled) for _, _, w in chain_c if w.spilled] + [0])[0]
        assert first_spill == spills if spills is not None else seen["spilled"] > 1, (cap, first_spill, seen)
        total += seen["runs"]
    asm.carry_enable(0)
    for name, kw in runs[:3]:
        A.check_layout(A.assemble_device(asm, **kw) if device else asm.assemble(fill=FILL, **kw), A.model(G, **kw), kw["capacity"], kw["max_rounds"], "carry off: " + name)
    asm.close()
    t.close()
    return total


def large_case(G=65600, events=1 << 17, seed=9, runs=3, device=True):
    """one larger chain: 2^17 events into G groups, C = G / 16, D = 2, a carry that holds all of it; `runs` runs and their routes against the models"""
    t = engine.Table(G, 3)
    rng = np.random.default_rng(seed)
    Cc = G // 16
    asm = engine.Assembler(t, events, max_expired=64, carry=3 * events)
    carry, old = empty_carry(), empty_carry()
    deferred = 0
    for k in range(runs):
        gid = rng.integers(0, G + (1 if k == 1 else 0), events).astype(np.uint32)
        head, abcd = A._rows(rng, events)
        eg = np.sort(rng.choice(G, 64, replace=False)).astype(np.uint32)
        kw = dict(gid=gid, head=head, abcd=abcd, capacity=Cc, max_rounds=2, expired=(eg, rng.integers(1, 1 << 20, 64).astype(np.uint32), 64))
        w = carry_model(G, carry, carry_capacity=3 * events, **kw)
        got = A.assemble_device(asm, deferred_capacity=4096, **kw) if device else asm.assemble(fill=FILL, deferred_capacity=4096, **kw)
        A.check_layout(got, w, Cc, 2, "large run %d" % k)
        _same_carry(asm.carry_read(abi.CARRY_NEXT), w.carry, "large run %d, the next carry" % k)
        _same_carry(asm.carry_read(abi.CARRY_LAST), old, "large run %d, the last carry" % k)
        row, per, _ = R.synthetic(rng, Cc, 2, w.n, w.R, 2)
        args = dict(gid=got.gid, count=w.n, rounds=w.R, origin=got.origin, row=row, persist32=per, capacity=Cc, max_rounds=2, arrival_capacity=events, expired_capacity=64)
        rw = route_model(w, Cc, 2, 3 * events, row, per)
        out = route_device(asm, **args) if device else asm.route(fill=FILL, carried=True, **args)
        R.check_routed(out, rw, w.m, w.e, "large run %d" % k)
        check_carried(out, rw, w.q, "large run %d" % k)
        deferred += int(w.stats[1])
        old = carry = w.carry
    assert deferred > events
    asm.close()
    t.close()
    return deferred


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def carried_struct(k):
    cols = dict(cell=np.zeros(max(k, 1), np.uint32), row=np.zeros(max(k, 1), abi.OUT32_DT), persist32=np.zeros(max(k, 1), abi.PERSIST32_DT))
    c = abi.CRoutedCarry()
    c.capacity, c.cell, c.row, c.persist32 = k, cols["cell"].ctypes.data, cols["row"].ctypes.data, cols["persist32"].ctypes.data
    return c, cols


def refusals_case(G=64, huge=True):
    """every refusal of the header's list answers -1 with a message, before any launch (none of them needs a run: the lane-serial emulation serves). huge: also
    the two refusals that need an assembler created for 2^30 events — 5 GiB of scratch that is allocated and never touched: for the emulation, whose device
    memory is the untouched heap, not for a GPU that others share"""
    t = engine.Table(G, 3)
    L = engine.lib()
    err = lambda: L.rg_last_error(t._h)      # noqa: E731
    asm = engine.Assembler(t, 16, max_expired=4)
    d, r, keep = R.refusal_structs(G)
    c, keep_c = carried_struct(8)
    n, buf = C.c_uint32(), np.zeros(64, np.uint8)
    # an assembler without a carry
    assert L.rg_route32_carry(asm._h, C.byref(d), C.byref(r), C.byref(c), abi.MEM_HOST) == -1 and b"has no carry" in err()
    assert L.rg_assembler_carry_reset(asm._h) == -1 and b"has no carry" in err()
    assert L.rg_assembler_carry_read(asm._h, abi.CARRY_NEXT, 0, C.byref(n), None, None, None) == -1 and b"has no carry" in err()
    # bit 30 marks a carried id
    assert L.rg_assembler_carry_enable(asm._h, 1 << 30) == -1 and b"below 2^30" in err()
    for events, expired in ((1 << 30, 0), (0, 1 << 30)) if huge else ():
        h = C.c_void_p()
        assert L.rg_assembler_create(t._h, events, expired, C.byref(h)) == 0, err()
        assert L.rg_assembler_carry_enable(h, 4) == -1 and b"below 2^30" in err()
        L.rg_assembler_destroy(h)
    asm.carry_enable(8)
    assert L.rg_route32_carry(asm._h, C.byref(d), C.byref(r), None, abi.MEM_HOST) == -1 and b"of the carried columns are required" in err()
    for col in ("cell", "row", "persist32"):
        c, keep_c = carried_struct(8)
        setattr(c, col, None)
        assert L.rg_route32_carry(asm._h, C.byref(d), C.byref(r), C.byref(c), abi.MEM_HOST) == -1 and b"of the carried columns are required" in err(), col
    c, keep_c = carried_struct(7)
    assert L.rg_route32_carry(asm._h, C.byref(d), C.byref(r), C.byref(c), abi.MEM_HOST) == -1 and b"a carried capacity of 7, the assembler's carry holds 8" in err()
    c, keep_c = carried_struct(8)
    d.capacity, d.max_rounds = (1 << 26) + 1, 32
    assert L.rg_route32_carry(asm._h, C.byref(d), C.byref(r), C.byref(c), abi.MEM_HOST) == -1 and b"holds at most 2^31" in err()
    d, r, keep = R.refusal_structs(G)
    assert L.rg_route32_carry(asm._h, C.byref(d), C.byref(r), C.byref(c), abi.MEM_HOST) == -1 and b"has not run yet" in err()
    assert L.rg_assembler_carry_read(asm._h, 2, 0, C.byref(n), None, None, None) == -1 and b"unknown carry 2" in err()
    assert L.rg_assembler_carry_read(asm._h, abi.CARRY_NEXT, 0, None, None, None, None) == -1 and b"count is required" in err()
    assert L.rg_assembler_carry_read(asm._h, abi.CARRY_NEXT, 4, C.byref(n), None, buf.ctypes.data, buf.ctypes.data) == -1 and b"count is required" in err()
    assert L.rg_assembler_carry_enable(None, 4) == -1 and L.rg_assembler_carry_reset(None) == -1
    # automatic index bases: a carrying assembler is refused by rg_assemble32, a plain one is not meant
    t.set_auto_index_base(1 << 20)
    a, b, keep_a = A.refusal_structs(G)
    assert L.rg_assemble32(asm._h, C.byref(a), C.byref(b), abi.MEM_HOST) == -1 and b"RG_OPT_AUTO_INDEX_BASE" in err()
    asm.close()
    t.close()


# ---- assemble -> tick -> route with a carry, against today's path fed by hand, and the oracle ---------------------------------------------------------------
PIPE_ROUNDS = 3                                             # the flood is thinned to a group's first three events of a lead() tick


def _widen(R, n, gid, head, abcd, terms):
    """a compact [R][n] batch as read back from the assembled columns -> the wide abi.Batch the oracle decides (rows with RG_HDR_SAME_TERM get their entries back;
    the others address `terms`, the entry array every launch was handed)"""
    b = abi.Batch(R, n, gid=gid)
    hdr, aux = head["hdr"].copy(), head["aux"].copy()
    ents, off = [], 0
    for i in np.flatnonzero((hdr & 0xF) == abi.EV_AE_REQ):
        c = int(hdr[i] >> 12)
        if hdr[i] & abi.HDR_SAME_TERM:
            ents.append(np.full(c, aux[i], np.int64))
            hdr[i] &= ~np.uint32(abi.HDR_SAME_TERM)
        else:
            ents.append(np.asarray(terms[int(aux[i]): int(aux[i]) + c], np.int64))
        aux[i], off = off, off + c
    b.head["hdr"], b.head["aux"] = hdr, aux
    b.ab["x"], b.ab["y"], b.cd["x"], b.cd["y"] = abcd["a"], abcd["b"], abcd["c"], abcd["d"]
    b.entry_terms = np.concatenate(ents) if ents else np.zeros(0, np.int64)
    b.entry_count = off
    return b


class _Side:
    """one table of pipeline_case with its tick recording (capacity G // 4, depth 2), assembler, arrival log and routed columns"""

    def __init__(self, table, G, log_cap, entry_cap, carry, resident):
        self.t, self.G, self.Cc, self.log_cap, self.K = table, G, max(G // 4, 1), log_cap, carry
        self.tick = engine.Tick2(table, 2, entry_cap=entry_cap, expired_cap=G, send=False, ready=False, device_resident=resident, sparse_cap=self.Cc, sparse_rounds=True)
        self.asm = engine.Assembler(table, log_cap, max_expired=G, carry=carry)
        self.pins = []
        cells = 2 * self.Cc
        self.dcap = log_cap + G + carry
        self.log_count, self.log_gid, self.log_head, self.log_abcd = self.pin(np.uint32, 1), self.pin(np.uint32, log_cap), self.pin(abi.HEAD_DT, log_cap), self.pin(abi.QUAD32_DT, log_cap)
        self.origin, self.deferred, self.stats = self.pin(np.uint32, cells), self.pin(np.uint32, self.dcap), self.pin(np.uint32, 4)
        arr = abi.CArrivals()
        arr.count, arr.capacity, arr.gid, arr.head, arr.abcd = self.log_count.ctypes.data, log_cap, self.log_gid.ctypes.data, self.log_head.ctypes.data, self.log_abcd.ctypes.data
        arr.expired_gid, arr.expired_epoch, arr.expired_count, arr.expired_capacity = self.tick.io.expired_gid, self.tick.io.expired_epoch, self.tick.io.expired_count, G
        self.arr = arr
        self.out = self.asm.for_tick(self.tick, self.origin.ctypes.data, self.deferred.ctypes.data, self.dcap, self.stats.ctypes.data)
        self.decided = self.asm.decided_for_tick(self.tick, self.origin.ctypes.data)
        self.cell, self.row, self.per, self.counts = self.pin(np.uint32, log_cap), self.pin(abi.OUT32_DT, log_cap), self.pin(abi.PERSIST32_DT, log_cap), self.pin(np.uint32, 4)
        self.xcell, self.xrow, self.xper = self.pin(np.uint32, G), self.pin(abi.OUT32_DT, G), self.pin(abi.PERSIST32_DT, G)
        r = abi.CRouted()
        r.arrival_capacity, r.cell, r.row, r.persist32, r.counts = log_cap, self.cell.ctypes.data, self.row.ctypes.data, self.per.ctypes.data, self.counts.ctypes.data
        r.expired_capacity, r.expired_cell, r.expired_row, r.expired_persist32 = G, self.xcell.ctypes.data, self.xrow.ctypes.data, self.xper.ctypes.data
        self.routed, self.carried = r, None
        if carry:
            self.ccell, self.crow, self.cper = self.pin(np.uint32, carry), self.pin(abi.OUT32_DT, carry), self.pin(abi.PERSIST32_DT, carry)
            c = abi.CRoutedCarry()
            c.capacity, c.cell, c.row, c.persist32 = carry, self.ccell.ctypes.data, self.crow.ctypes.data, self.cper.ctypes.data
            self.carried = c

    def pin(self, dtype, k):
        a, p = engine.pinned_like(self.t, np.zeros(max(k, 1), dtype=dtype))
        self.pins.append(p)
        return a

    def queue(self, gid, head, abcd, terms, terms_at, nows):
        """the host's part of a tick, then the three calls queued with nothing between them"""
        m = len(gid)
        assert m <= self.log_cap
        self.log_gid[:m], self.log_head[:m], self.log_abcd[:m], self.log_count[0] = gid, head, abcd, m
        self.tick._put(self.tick.entry_terms, terms[terms_at:], at=terms_at)
        self.tick.now[:] = nows
        self.asm.run_device(self.arr, self.out)
        self.tick.launch()
        self.asm.route_device(self.decided, self.routed, carried=self.carried)

    def read(self):
        """after the wait: n, R and the [R][n] images of the batch and of what the tick decided"""
        tk = self.tick
        n, R = int(tk.count[0]), int(tk.depth_now[0])
        tk.n, tk.depth = n, R
        grid = lambda col, dt: np.ascontiguousarray(tk._get(col, dt, 2 * self.Cc).reshape(2, self.Cc)[:R, :n]).reshape(-1)      # noqa: E731
        return types.SimpleNamespace(n=n, R=R, gid=tk._get(tk.gid, np.uint32, n), head=grid(tk.head, abi.HEAD_DT), abcd=grid(tk.abcd, abi.QUAD32_DT),
                                     row=grid(tk.row, abi.OUT32_DT), per=grid(tk.persist32, abi.PERSIST32_DT), expired=tk.expired(), stats=self.stats.copy())

    def close(self):
        self.asm.close()
        self.tick.close()
        for p in self.pins:
            p.free()


def pipeline_case(G, P, seed, ticks=25):
    """Table A: a carrying assembler and a device-resident tick, rg_assemble32 -> rg_tick2_launch -> rg_route32_carry queued with nothing between them, the host
    looks only after rg_tick2_wait. Table B: today's path — the test reads deferred[] and prepends the rows to the next log by the header's recipe. Both take the
    rows assemble_cases.lead draws (a scratch oracle leads; the flood is thinned to a group's first PIPE_ROUNDS events), into a
    tick recording of capacity G // 4 and depth 2 (the scratch oracle decides its own rows in its own order and so drifts from the tables: part of the stream is
    stale when it is decided, as a flood's is). Every tick: the five batch columns, outcome rows, table state, deadlines, health and expired columns of A and B are
    bit-identical; every arrival's answer, found by following the chain through A's routed columns, is B's answer for that event; the oracle decides the batch as
    read back and agrees on rows and state wherever the tick has no RG_NEED_HOST row (one that has reloads all three tables from the oracle: at most 1 tick in 4).
    -> (ticks that deferred, resynchronised ticks)"""
    from tests import fuzz, oracle_lib
    from tests import sparse_rounds_cases as X
    from tests.clock import origin as clock_origin
    from tests.helpers import compare_outcomes, compare_states
    self_slot = 2 % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    a, b = engine.Table(G, P, self_slot, True), engine.Table(G, P, self_slot, True)
    orc, gen = oracle_lib.OracleTable(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    for t in (a, b, orc, gen):
        t.load_state(st0)
    for t in (a, b, gen):
        t.timers_configure(900, 300, 4321)
        t.timers_arm(clock_origin())
    fz, rng = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False), np.random.default_rng(seed)
    new_cap, K = PIPE_ROUNDS * G, 16 * G
    entry_cap = 8 * G * PIPE_ROUNDS * ticks
    A_, B_ = _Side(a, G, new_cap, entry_cap, K, True), _Side(b, G, new_cap + K + G, entry_cap, 0, False)
    terms = np.zeros(entry_cap, np.int32)
    terms_n = 0
    none = np.zeros(0, np.uint32)
    uid_next = 0
    where_a = {}                                            # A's readers: uid -> ("log", k) or ("carry", slot), until the event is answered
    hand = (none, np.zeros(0, abi.HEAD_DT), np.zeros(0, abi.QUAD32_DT), np.zeros(0, np.int64))      # B's deferred rows for its next log, and their uids (-1: a ticket)
    fired_b = (none, none)
    seen = dict(deferred_ticks=0, ticket_carried=0, carried_twice=0, drain=0, resync=0, answered=0)
    for k in range(ticks):
        at = "tick %d" % k
        t = A.lead(gen, fz, rng, G, k, none, none, P)
        lg, lh, la, at_r, _ = A.arrival_log(t, rng)
        keep = at_r < PIPE_ROUNDS
        lg, lh, la = lg[keep], lh[keep].copy(), la[keep]
        ae = ((lh["hdr"] & 0xF) == abi.EV_AE_REQ) & ((lh["hdr"] & abi.HDR_SAME_TERM) == 0)      # the entry terms of a row stay where they are until it is routed
        lh["aux"][ae] += np.uint32(terms_n)
        e_n = t.b32.entry_count if t.n else 0
        assert terms_n + e_n <= entry_cap
        if e_n:
            terms[terms_n: terms_n + e_n] = t.b32.entry_terms[:e_n]
        m = len(lg)
        uids = np.arange(uid_next, uid_next + m)
        uid_next += m
        nows = [X.now_of(k, 0), X.now_of(k, 1)]
        q_in = len(A_.asm.carry_read(abi.CARRY_NEXT)[0])
        before = orc.read_state()
        for u, j in zip(uids.tolist(), range(m)):
            where_a[u] = ("log", j)
        A_.ccell[:] = FILL32
        A_.queue(lg, lh, la, terms, terms_n, nows)
        hg, hh, ha, hu = hand
        b_uids = np.concatenate([hu, uids])
        B_.queue(np.concatenate([hg, lg]), np.concatenate([hh, lh]), np.concatenate([ha, la]), terms, terms_n, nows)
        terms_n += e_n
        A_.tick.wait()
        B_.tick.wait()
        a.sync()
        b.sync()
        ra, rb = A_.read(), B_.read()
        # ---- A and B, bit for bit
        assert (ra.n, ra.R) == (rb.n, rb.R) and np.array_equal(ra.gid, rb.gid), at
        for f in ("head", "abcd", "row"):
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), (at, f)
        pf = (ra.row["flags"] & abi.F_PERSIST) != 0
        assert np.array_equal(ra.per[pf], rb.per[pf]), at
        assert list(ra.stats[:3]) == list(rb.stats[:3]) and ra.stats[3] == 0, (at, ra.stats, rb.stats)
        compare_states(b.read_state(), a.read_state(), at + ": A against B")
        assert np.array_equal(a.timers_read(), b.timers_read()), at
        for x, y in zip(a.health_read(), b.health_read()):
            assert np.array_equal(x, y), at
        assert ra.expired[2] == rb.expired[2] and np.array_equal(ra.expired[0], rb.expired[0]) and np.array_equal(ra.expired[1], rb.expired[1]), at
        # ---- the readers: A's chain against B's columns
        ans_a, ans_b = {}, {}
        for u, (kind, j) in list(where_a.items()):
            v = int(A_.cell[j] if kind == "log" else A_.ccell[j])
            if v < 0x80000000:
                row, per = (A_.row[j], A_.per[j]) if kind == "log" else (A_.crow[j], A_.cper[j])
                ans_a[u] = (v, row.tobytes(), per.tobytes() if row["flags"] & abi.F_PERSIST else b"")
                del where_a[u]
            elif v == NONE:
                del where_a[u]                               # (a bad gid: the stream has none)
                raise AssertionError("%s: event %d was routed nowhere" % (at, u))
            else:
                assert v != SPILLED and v != FILL32, (at, u, hex(v))
                seen["carried_twice"] += kind == "carry"
                where_a[u] = ("carry", v & 0x3FFFFFFF)
        for j, u in enumerate(b_uids.tolist()):
            v = int(B_.cell[j])
            if u >= 0 and v != NONE:
                ans_b[u] = (v, B_.row[j].tobytes(), B_.per[j].tobytes() if B_.row[j]["flags"] & abi.F_PERSIST else b"")
        assert ans_a == ans_b, (at, len(ans_a), len(ans_b))
        seen["answered"] += len(ans_a)
        xc = A_.xcell[: len(fired_b[0])]
        seen["ticket_carried"] += int(np.count_nonzero((xc & 0x80000000 != 0) & (xc < SPILLED)))
        # ---- B's host step: the deferred rows to the head of its next log (the header's recipe)
        d = B_.deferred[: int(rb.stats[1])].astype(np.int64)
        assert int(rb.stats[1]) <= B_.dcap
        is_x = (d & EXPIRED) != 0
        j = d & 0x7FFFFFFF
        bl_g, bl_h, bl_a = np.concatenate([hg, lg]), np.concatenate([hh, lh]), np.concatenate([ha, la])
        ng, nh, na, nu = np.zeros(len(d), np.uint32), np.zeros(len(d), abi.HEAD_DT), np.zeros(len(d), abi.QUAD32_DT), np.full(len(d), -1, np.int64)
        ng[is_x], nh["hdr"][is_x], nh["aux"][is_x] = fired_b[0][j[is_x]], A.TIMEOUT_HDR, fired_b[1][j[is_x]]
        ng[~is_x], nh[~is_x], na[~is_x], nu[~is_x] = bl_g[j[~is_x]], bl_h[j[~is_x]], bl_a[j[~is_x]], b_uids[j[~is_x]]
        hand = (ng, nh, na, nu)
        assert len(ng) <= K
        _same_carry(A_.asm.carry_read(abi.CARRY_NEXT), (ng, nh, na), at + ": A's carry against B's deferred rows")
        fired_b = (rb.expired[0], rb.expired[1])
        seen["deferred_ticks"] += int(rb.stats[1]) > 0
        seen["drain"] += m == 0 and q_in > 0
        # ---- the oracle decides the batch as read back
        if ra.n:
            want = fuzz.concat_outcomes([orc.submit(_widen(1, ra.n, ra.gid, ra.head[r * ra.n: (r + 1) * ra.n], ra.abcd[r * ra.n: (r + 1) * ra.n], terms))
                                         for r in range(ra.R)])      # (the oracle takes a list of groups a round at a time)
            got = abi.Outcome32(ra.R * ra.n, wide=False)
            got.row, got.persist = ra.row, ra.per
            got32, _ = engine.unpack32(got, ra.R, ra.n, before.role_epoch[ra.gid])
            if not np.any(got32.status == abi.NEED_HOST):
                compare_outcomes(want, got32, at + ": against the oracle")
                compare_states(orc.read_state(), a.read_state(), at + ": against the oracle")
            else:
                st = orc.read_state()
                a.load_state(st)
                b.load_state(st)
                seen["resync"] += 1
    assert seen["deferred_ticks"] * 2 > ticks and seen["ticket_carried"] > 0 and seen["carried_twice"] > 0 and seen["drain"] > 0 and seen["answered"] > 0, seen
    assert seen["resync"] * 4 <= ticks, "%d of %d ticks were resynchronised from the oracle (cap: 1 in 4)" % (seen["resync"], ticks)
    A_.close()
    B_.close()
    for t in (a, b, orc, gen):
        t.close()
    return seen["deferred_ticks"], seen["resync"]
