"""The grow-only staging buffers of the RG_MEM_HOST entry points under CHANGING shapes: one table takes a sequence of calls whose sizes rise, fall and rise
again, through every entry point that stages — rg_submit (dense, a list of groups, with and without a hint column and entry terms), rg_submit32, rg_submit32c,
rg_submit32c_sparse, rg_submit32c_sparse_rounds (with and without the overflow columns), rg_submit_async and rg_submit_async_packed (more batches than
RG_PIPELINE_DEPTH: slots are reused), rg_timers_update(32), rg_health_update(32), rg_replicate (dense, a list), rg_health_failure, rg_timers_expired_epochs and
rg_ready. Several of them share a buffer (the gid list, the heads, the reply rows, the compact outcome rows), so a buffer sized by one call serves the next.
Shared by tests/test_host_staging_gpu.py (an MI355X) and tests/devemu/emu_cases_host_staging.py (the host emulation of the kernels).

Three tables with the same seeded state move in lockstep. Table A takes everything through RG_MEM_HOST: its buffers are reused for the whole sequence. Table B
takes the same calls through RG_MEM_DEVICE, where nothing is staged (the pipelined calls have no such form: B decides their batches with rg_submit / rg_submit32
on resident columns). The oracle LEADS, round by round: fuzz.Fuzzer(allow_miss=False) draws a round, the oracle decides it and folds it into its timers and
statistics; then all rounds go to A and to B in one call each. Every outcome row, deadline, statistic, fired ticket, send row and
readiness byte of A equals B's bit for bit, and both equal the oracle's.

Where "bit for bit" needs a mask: the pipelined paths zero nothing before a launch (include/raftgpu.h: a conditional field is valid only under its flag), so
their logfx / persist columns are compared under the flags; replies are compared whole. No row answers RG_NEED_HOST (asserted: the oracle's lossless log never
does, so such a row could not be compared): lead() says how the stream stays inside the term runs the device caches."""
import ctypes as C
import os
import types

import numpy as np

from rafting_amd import abi, engine
from tests import clock, fuzz, oracle_lib
from tests.helpers import compare_outcomes, compare_states
from tests.sparse_tick_cases import subset

EMULATED = os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so")
ROUNDS = (1, 4, 1, 70)                                        # 70: above 64, the clock chunk loop of the timer and health updates runs twice


class Resident:
    """a column in the table's device memory: engine.DeviceBuffer on the card; on the emulation device memory is the heap, so a numpy array stands in"""

    def __init__(self, table, array):
        self.a = np.ascontiguousarray(array).copy()
        self.buf = None if EMULATED else engine.DeviceBuffer.from_host(table, self.a)
        self.ptr = self.a.ctypes.data if EMULATED else self.buf.ptr

    def read(self):
        if self.buf is not None and self.a.size:
            self.a = self.buf.to_host(self.a.dtype, self.a.size)
        return self.a

    def free(self):
        if self.buf is not None:
            self.buf.free()


def _resident(table, *arrays):
    return [None if a is None else Resident(table, a) for a in arrays]


def _ptr(r):
    return None if r is None else r.ptr


def _free(cols):
    for c in cols:
        if c is not None:
            c.free()


# ---- table B: the same calls through RG_MEM_DEVICE ----------------------------------------------------------------------------------------------------------
def b_submit(t, batch):
    n = batch.rounds * batch.count
    ins = _resident(t, batch.gid, batch.head, batch.ab, batch.cd, batch.entry_terms[: batch.entry_count] if batch.entry_count else None, batch.hint)
    outs = _resident(t, np.zeros(n, abi.REPLY_DT), np.zeros(n, abi.LOGFX_DT), np.zeros(n, abi.PERSIST_DT))
    cb, co = abi.CBatch(), abi.COutcome()
    cb.rounds, cb.count, cb.entry_count = batch.rounds, batch.count, batch.entry_count
    cb.gid, cb.head, cb.ab, cb.cd, cb.entry_terms, cb.hint = [_ptr(x) for x in ins]
    co.reply, co.logfx, co.persist = [x.ptr for x in outs]
    t._check(engine.lib().rg_submit(t._h, C.byref(cb), C.byref(co), abi.MEM_DEVICE))
    t.sync()
    o = abi.Outcome(0)
    o.reply, o.logfx, o.persist = [x.read() for x in outs]
    _free(ins + outs)
    return o


def _cbatch32(t, b32):
    ins = _resident(t, b32.gid, b32.head, b32.abcd, b32.entry_terms[: b32.entry_count] if b32.entry_count else None)
    cb = abi.CBatch32()
    cb.rounds, cb.count, cb.entry_count = b32.rounds, b32.count, b32.entry_count
    cb.gid, cb.head, cb.abcd, cb.entry_terms = [_ptr(x) for x in ins]
    return cb, ins


def b_submit32(t, b32):
    n = b32.rounds * b32.count
    cb, ins = _cbatch32(t, b32)
    outs = _resident(t, np.zeros(n, abi.REPLY_DT), np.zeros(n, abi.LOGFX_DT), np.zeros(n, abi.PERSIST_DT))
    co = abi.COutcome()
    co.reply, co.logfx, co.persist = [x.ptr for x in outs]
    t._check(engine.lib().rg_submit32(t._h, C.byref(cb), C.byref(co), abi.MEM_DEVICE))
    t.sync()
    o = abi.Outcome(0)
    o.reply, o.logfx, o.persist = [x.read() for x in outs]
    _free(ins + outs)
    return o


def b_submit32c(t, b32, name, wide):
    n = b32.rounds * b32.count
    cb, ins = _cbatch32(t, b32)
    outs = _resident(t, np.zeros(n, abi.OUT32_DT), np.zeros(n, abi.PERSIST32_DT))
    over = _resident(t, np.zeros(n, abi.REPLY_DT), np.zeros(n, abi.LOGFX_DT), np.zeros(n, abi.PERSIST_DT)) if wide else []
    co = abi.COutcome32()
    co.row, co.persist = [x.ptr for x in outs]
    if wide:
        co.wide.reply, co.wide.logfx, co.wide.persist = [x.ptr for x in over]
    t._check(getattr(engine.lib(), name)(t._h, C.byref(cb), C.byref(co), abi.MEM_DEVICE))
    t.sync()
    o = abi.Outcome32(n, wide=wide)
    o.row, o.persist = [x.read() for x in outs]
    if wide:
        o.wide.reply, o.wide.logfx, o.wide.persist = [x.read() for x in over]
    _free(ins + outs + over)
    return o


def b_timers_update(t, rounds, count, gid, reply, nows):
    cols = _resident(t, gid, reply)
    now = np.ascontiguousarray(nows, dtype=np.int64)
    t._check(engine.lib().rg_timers_update(t._h, rounds, count, _ptr(cols[0]), cols[1].ptr, now.ctypes.data, abi.MEM_DEVICE))
    t.sync()
    _free(cols)


def b_health_update(t, rounds, count, gid, head, reply, nows):
    cols = _resident(t, gid, head, reply)
    now = np.ascontiguousarray(nows, dtype=np.int64)
    t._check(engine.lib().rg_health_update(t._h, rounds, count, _ptr(cols[0]), cols[1].ptr, cols[2].ptr, now.ctypes.data, abi.MEM_DEVICE))
    t.sync()
    _free(cols)


def b_update32(t, rounds, head, out32, nows):
    cols = _resident(t, head, out32.row, out32.persist)
    now = np.ascontiguousarray(nows, dtype=np.int64)
    t._check(engine.lib().rg_timers_update32(t._h, rounds, cols[1].ptr, cols[2].ptr, now.ctypes.data, abi.MEM_DEVICE))
    t._check(engine.lib().rg_health_update32(t._h, rounds, cols[0].ptr, cols[1].ptr, now.ctypes.data, abi.MEM_DEVICE))
    t.sync()
    _free(cols)


def b_expired(t, now, capacity):
    cols = _resident(t, np.zeros(max(capacity, 1), np.uint32), np.zeros(max(capacity, 1), np.uint32))
    n = C.c_uint32()
    t._check(engine.lib().rg_timers_expired_epochs(t._h, now, cols[0].ptr, cols[1].ptr, capacity, C.byref(n), abi.MEM_DEVICE))
    t.sync()
    k = min(n.value, capacity)
    got = cols[0].read()[:k], cols[1].read()[:k], n.value
    _free(cols)
    return got


def b_replicate(t, gid, heartbeat, in_flight):
    """-> (head[count], send[count, F]), as engine.Table.replicate; callers pass in_flight as [count, F], the wire is follower-major"""
    F = t.cluster - 1
    count = t.groups if gid is None else len(gid)
    fl = None if in_flight is None else np.ascontiguousarray(np.asarray(in_flight, dtype=np.uint16).reshape(count, F).T).reshape(count * F)
    ins = _resident(t, gid, heartbeat, fl)
    outs = _resident(t, np.zeros(count, abi.SEND_HEAD_DT), np.zeros(count * F, abi.SEND_DT))
    t._check(engine.lib().rg_replicate(t._h, count, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), outs[0].ptr, outs[1].ptr, abi.MEM_DEVICE))
    t.sync()
    head, send = outs[0].read(), np.ascontiguousarray(outs[1].read().reshape(F, count).T)
    _free(ins + outs)
    return head, send


def b_ready(t, now, critical_point, cool_down_ms):
    col = Resident(t, np.zeros(t.groups, np.uint8))
    t._check(engine.lib().rg_ready(t._h, now, critical_point, cool_down_ms, col.ptr, abi.MEM_DEVICE))
    t.sync()
    got = col.read()
    col.free()
    return got


# ---- the oracle leads ---------------------------------------------------------------------------------------------------------------------------------------
def _without_entries(b):
    """every AppendEntries row that carries entries becomes RG_EV_NONE: the batch has no entry terms"""
    hdr = b.head["hdr"]
    drop = ((hdr & 0xF) == abi.EV_AE_REQ) & ((hdr >> 12) > 0)
    b.head[drop], b.ab[drop], b.cd[drop] = (0, 0), (0, 0), (0, 0)
    b.entry_terms, b.entry_count = np.zeros(0, np.int64), 0


def lead(x, R, rows=None, entries=True):
    """the oracle's half of one call: R rounds, dense or for the groups `rows`, decided one after the other and folded into its timers and statistics. The rounds
    are drawn from the PILOT's state: a device table that decides them one by one, ahead of A and B, so that the fuzzer sees the four term runs the device
    caches after every round (the oracle's log is lossless) and draws no lookup that leaves them"""
    x.now += 150
    nows = [x.now + 2 * r for r in range(R)]
    subs, outs = [], []
    for r in range(R):
        b = abi.Batch(1, x.G)
        x.fz.round(x.pilot.read_state(), b, 0)
        if not entries:
            _without_entries(b)
        s = b if rows is None else subset(b, rows)
        _no_need_host(types.SimpleNamespace(n=s.count, batch=s), x.pilot.submit(s), "the pilot, round %d" % r)
        oo = x.orc.submit(s, now=[nows[r]])
        x.orc.timers_update(1, s.count, oo.reply, [nows[r]], gid=s.gid)
        subs.append(s)
        outs.append(oo)
    batch = fuzz.concat_batches(subs)
    if rows is not None:
        batch.gid = np.asarray(rows, dtype=np.uint32)
    assert abi.batch_fits_32(batch) and (entries or batch.entry_count == 0)
    x.entries_seen.append(batch.entry_count)
    return types.SimpleNamespace(R=R, n=batch.count, rows=rows, batch=batch, want=fuzz.concat_outcomes(outs), nows=nows)


def _same(a, b, where):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), where


def _same_wide(a, b, where, zeroed=True):
    """two rg_outcome_t images of one batch; zeroed: both sides hold zeroes where the kernel wrote nothing, so every column is compared whole"""
    _same(a.reply, b.reply, where)
    if zeroed:
        _same(a.logfx, b.logfx, where)
        _same(a.persist, b.persist, where)
    else:
        compare_outcomes(a, b, where)


def _no_need_host(t, oa, where):
    bad = np.flatnonzero(oa.status == abi.NEED_HOST)
    assert len(bad) == 0, (where, "RG_NEED_HOST at (round, row, event kind)", [(int(i) // t.n, int(i) % t.n, int(t.batch.head["hdr"][i]) & 0xF) for i in bad[:8]])


def _checked(x, t, oa, ob, where, zeroed=True):
    """the wide rows of one call: A's against B's, and against the oracle's"""
    _no_need_host(t, oa, where)
    _same_wide(oa, ob, where, zeroed)
    compare_outcomes(t.want, oa, where)


def _fold_wide(x, t, oa, ob):
    """rg_timers_update / rg_health_update over the wide reply rows of call t (a list of groups: one round per call, as the header asks)"""
    b, n = t.batch, t.n
    if b.gid is None:
        x.A.timers_update(t.R, n, oa.reply, t.nows)
        x.A.health_update(b, oa.reply, t.nows)
        b_timers_update(x.B, t.R, n, None, ob.reply, t.nows)
        b_health_update(x.B, t.R, n, None, b.head, ob.reply, t.nows)
        return
    for r in range(t.R):
        sl = slice(r * n, (r + 1) * n)
        one = abi.Batch(1, n, gid=b.gid)
        one.head[:] = b.head[sl]
        x.A.timers_update(1, n, oa.reply[sl], t.nows[r: r + 1], gid=b.gid)
        x.A.health_update(one, oa.reply[sl], t.nows[r: r + 1])
        b_timers_update(x.B, 1, n, b.gid, ob.reply[sl], t.nows[r: r + 1])
        b_health_update(x.B, 1, n, b.gid, one.head, ob.reply[sl], t.nows[r: r + 1])


def _columns(x, where):
    """deadlines, statistics and the whole state: A, B and the oracle"""
    ta, tb = x.A.timers_read(), x.B.timers_read()
    _same(ta, tb, where)
    _same(ta, x.orc.timers_read(), where)
    for a, b, o in zip(x.A.health_read(), x.B.health_read(), x.orc.health_read()):
        _same(a, b, where)
        _same(a, o, where)
    sa = x.A.read_state()
    compare_states(sa, x.B.read_state(), where)
    compare_states(x.orc.read_state(), sa, where)


def _aside(x, k, rows):
    """the small entry points between two submissions: failures, the fired tickets, the sends (dense, or for the groups `rows`), readiness"""
    where = "step %d, beside the batch" % k
    G, P = x.G, x.P
    n = (7, 40, 0, 3)[k % 4]
    fg, fs, ff = x.rng.integers(0, G, n).astype(np.uint32), x.rng.integers(0, P, n).astype(np.uint8), x.rng.integers(0, 4, n).astype(np.uint8)
    for t in (x.A, x.B, x.orc):
        t.health_failure(fg, fs, ff, x.now + 3)
    cap = (G, 3, G, 1)[k % 4]
    ea, eb, eo = x.A.timers_expired_epochs(x.now + 400, cap), b_expired(x.B, x.now + 400, cap), x.orc.timers_expired_epochs(x.now + 400, cap)
    for a, b, o in zip(ea, eb, eo):
        assert np.array_equal(a, b) and np.array_equal(a, o), where
    x.fired += ea[2]
    gid = None if rows is None else np.asarray(rows, dtype=np.uint32)
    m = G if rows is None else len(rows)
    hb, fl = (None, None) if k % 3 == 0 else ((x.rng.random(m) < 0.5).astype(np.uint8), x.rng.integers(0, 24, (m, P - 1)).astype(np.uint16))
    (ha, sa), (hb_, sb), (ho, so) = x.A.replicate(gid, hb, fl), b_replicate(x.B, gid, hb, fl), x.orc.replicate(gid, hb, fl)
    x.pilot.replicate(gid, hb, fl)                               # (the send side prepares the leaders it meets: the pilot's state follows)
    _same(ha, hb_, where)
    _same(sa, sb, where)
    _same(ha, ho, where)
    _same(sa, so, where)
    x.sends += int(np.count_nonzero(sa["kind"] == abi.SEND_APPEND)) if m else 0
    ra, rb, ro = x.A.ready(x.now + 5, 1, 60), b_ready(x.B, x.now + 5, 1, 60), x.orc.ready(x.now + 5, 1, 60)
    _same(ra, rb, where)
    _same(ra, ro, where)
    _columns(x, where)


def _list(x, n):
    return np.sort(x.rng.choice(x.G, n, replace=False)).astype(np.int64)


# ---- the steps ----------------------------------------------------------------------------------------------------------------------------------------------
def _wide(x, k, R, rows=None, hint=False, entries=True):
    """rg_submit"""
    where = "step %d: rg_submit, %d rounds, %s" % (k, R, "dense" if rows is None else "%d listed groups" % len(rows))
    t = lead(x, R, rows, entries)
    if hint:
        t.batch.hint = np.zeros(t.R * t.n, dtype=abi.PAIR_DT)      # (a hint column no row points into: it is staged all the same)
    oa, ob = x.A.submit(t.batch), b_submit(x.B, t.batch)
    _checked(x, t, oa, ob, where)
    _fold_wide(x, t, oa, ob)
    _aside(x, k, rows)


def _compact(x, k, R, rows=None, entries=True):
    """rg_submit32"""
    where = "step %d: rg_submit32, %d rounds" % (k, R)
    t = lead(x, R, rows, entries)
    b32 = engine.pack32(t.batch)
    oa, ob = x.A.submit32(b32), b_submit32(x.B, b32)
    _checked(x, t, oa, ob, where)
    _fold_wide(x, t, oa, ob)
    _aside(x, k, rows)


def _compact_rows(x, k, R, name, rows=None, wide=True, entries=True):
    """rg_submit32c, rg_submit32c_sparse, rg_submit32c_sparse_rounds: compact outcome rows"""
    where = "step %d: %s, %d rounds, overflow columns: %s" % (k, name, R, wide)
    before = x.A.read_state().role_epoch
    t = lead(x, R, rows, entries)
    b32 = engine.pack32(t.batch)
    ra = getattr(x.A, name[3:])(b32, wide=wide)
    rb = b_submit32c(x.B, b32, name, wide)
    _same(ra.row, rb.row, where)
    _same(ra.persist, rb.persist, where)
    if wide:
        _same_wide(ra.wide, rb.wide, where)
    oa, _ = engine.unpack32(ra, t.R, t.n, before if rows is None else before[rows])
    _no_need_host(t, oa, where)
    compare_outcomes(t.want, oa, where)
    if rows is None:                                             # a dense batch: the timers and the statistics from the compact rows where they lie
        x.A.timers_update32(t.R, ra, t.nows)
        x.A.health_update32(t.batch, ra, t.nows)
        b_update32(x.B, t.R, t.batch.head, rb, t.nows)
    else:
        _fold_wide(x, t, oa, engine.unpack32(rb, t.R, t.n, before[rows])[0])
    _aside(x, k, rows)


def _pipelined(x, k, packed):
    """rg_submit_async / rg_submit_async_packed: RG_PIPELINE_DEPTH + 2 batches of 1 and 4 rounds, so that every slot is used again at another size"""
    name = "rg_submit_async_packed" if packed else "rg_submit_async"
    N = abi.PIPELINE_DEPTH + 2
    ts = [lead(x, (1, 4)[i % 2], entries=i != 2) for i in range(N)]
    held = [engine.PackedBatch(x.A, t.batch) if packed else abi.Outcome(t.R * t.n) for t in ts]
    for t, h in zip(ts, held):
        if packed:
            x.A.submit_async_packed(h)
        else:
            x.A.submit_async(t.batch, h)
    while x.A.submit_wait() is not None:
        pass
    for i, (t, h) in enumerate(zip(ts, held)):
        where = "step %d: %s, batch %d of %d" % (k, name, i, N)
        oa = h.unpack() if packed else h
        ob = b_submit32(x.B, engine.pack32(t.batch)) if packed else b_submit(x.B, t.batch)
        _checked(x, t, oa, ob, where, zeroed=False)
        _fold_wide(x, t, oa, ob)
        if packed:
            h.free()
    _aside(x, k, None)


def _empty_lists(x, k):
    """a list of no groups: every entry point returns before anything is staged, and nothing moves"""
    L, none = engine.lib(), np.zeros(0, np.uint32)
    for t in (x.A, x.B):
        before = t.read_state()
        b = abi.Batch(1, 0, gid=none)
        assert len(t.submit(b).reply) == 0
        b32 = abi.Batch32(1, 0, none, np.zeros(0, abi.HEAD_DT), np.zeros(0, abi.QUAD32_DT), np.zeros(1, np.int32), 0)
        assert len(t.submit32(b32).reply) == 0 and len(t.submit32c_sparse(b32).row) == 0 and len(t.submit32c_sparse_rounds(b32).row) == 0
        t.timers_update(1, 0, np.zeros(0, abi.REPLY_DT), [x.now], gid=none)
        t.health_update(b, np.zeros(0, abi.REPLY_DT), [x.now])
        head, send = t.replicate(gid=none)
        assert len(head) == 0 and len(send) == 0
        assert L.rg_health_failure(t._h, 0, None, None, None, x.now) == 0
        compare_states(before, t.read_state(), "step %d: empty lists" % k)
    _aside(x, k, None)


def changing_shapes_case(G, P, seed):
    """the sequence: rounds 1, 4, 1, 70; lists of 5 groups, of every group, of none, of 3; entry terms absent, present, absent — and then small again"""
    self_slot = 1 % P
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    x = types.SimpleNamespace(G=G, P=P, A=engine.Table(G, P, self_slot, True), B=engine.Table(G, P, self_slot, True),
                              orc=oracle_lib.OracleTable(G, P, self_slot, True), pilot=engine.Table(G, P, self_slot, True), fz=fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False),
                              rng=np.random.default_rng(seed), now=clock.origin(), fired=0, sends=0, entries_seen=[])
    x.pilot.load_state(st0)
    for t in (x.A, x.B, x.orc):
        t.load_state(st0)
        t.timers_configure(900, 300, 77)
        t.timers_arm(clock.origin())
    every = np.arange(G, dtype=np.int64)
    _wide(x, 0, ROUNDS[0], entries=False)
    _wide(x, 1, 1, rows=_list(x, 5), hint=True)
    _compact(x, 2, ROUNDS[1])
    _wide(x, 3, 1, rows=every, entries=False)
    _compact_rows(x, 4, ROUNDS[2], "rg_submit32c", wide=True)
    _empty_lists(x, 5)
    _compact_rows(x, 6, 1, "rg_submit32c_sparse", rows=_list(x, 3), wide=False)
    _wide(x, 7, ROUNDS[3], hint=True)
    _compact_rows(x, 8, ROUNDS[3], "rg_submit32c", wide=False, entries=False)
    _compact_rows(x, 9, ROUNDS[1], "rg_submit32c_sparse_rounds", rows=_list(x, 5), wide=True)
    _pipelined(x, 10, packed=False)
    _pipelined(x, 11, packed=True)
    _compact(x, 12, 1, rows=_list(x, 3), entries=False)
    _compact_rows(x, 13, 1, "rg_submit32c_sparse", rows=every, wide=True)
    _wide(x, 14, ROUNDS[0])
    assert x.fired > 0 and x.sends > 0, (x.fired, x.sends)
    top = x.entries_seen.index(max(x.entries_seen))
    assert x.entries_seen[top] > 0 and 0 in x.entries_seen[:top] and 0 in x.entries_seen[top:], x.entries_seen      # entry terms: none, some, none
    for t in (x.A, x.B, x.orc, x.pilot):
        t.close()
    return len(x.entries_seen)
