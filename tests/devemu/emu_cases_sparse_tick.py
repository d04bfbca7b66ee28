"""Cases for rg_submit32c_sparse and the sparse device-resident tick (rg_tick2_create_sparse) on the host emulation of the kernels. Run by
tests/test_sparse_tick_cpu.py in a subprocess; TEST INFRASTRUCTURE. The device cases need the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1: the
two-wavefront bodies with their LDS hand-over, the expiry's ballots); the refusals happen on the host before any launch and run in either mode
(`-k refuses`). The cases are those of tests/test_sparse_tick_gpu.py at small table sizes (tests/sparse_tick_cases.py), plus what only an emulation can
check safely: a row count above the capacity."""
import ctypes as C
import os

import numpy as np
import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from rafting_amd import abi, engine  # noqa: E402
from tests import fuzz, oracle_lib  # noqa: E402
from tests import clock  # noqa: E402
from tests import sparse_tick_cases as X  # noqa: E402
from tests.helpers import compare_outcomes  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the two-wavefront kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("cluster,seed", [(3, 11), (5, 12), (7, 16)])
def test_standalone_lists_of_groups_in_lockstep_with_the_oracle(cluster, seed):
    X.standalone_case(192, cluster, 12, seed)


@device
def test_standalone_lists_of_groups_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    X.standalone_case(192, 5, 8, 13)


@device
@pytest.mark.parametrize("G,seed,ticks,resident", [(256, 321, 15, False), (200, 77, 10, True)])
def test_the_sparse_tick_matches_the_oracle(G, seed, ticks, resident):
    X.sparse_tick_case(G, seed, ticks, device_resident=resident, expect_all=False)


@device
def test_the_sparse_tick_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    X.sparse_tick_case(128, 5, 10, expect_all=False)


@device
def test_every_group_listed_equals_the_dense_tick():
    X.same_as_dense_case(128, ticks=8)


@device
def test_automatic_bases_in_sparse_ticks():
    flushes, moved = X.auto_base_case(128, 16, 31)
    assert flushes > 16 and moved > 0


@device
def test_a_recording_made_before_an_option_changed_is_turned_down():
    X.stale_recording_case()


@device
def test_a_count_above_the_capacity_is_clamped():
    """*count = 100 with a capacity of 64: rows 0 .. 63 are decided like the oracle decides them, nothing at or beyond row 64 of any output column is touched
    (the columns are longer than the capacity here and carry a fill pattern; on the emulation plain heap memory stands for device memory)"""
    G, P, cap, given, FILL = 128, 5, 64, 100, 0xAB
    F = P - 1
    st0 = fuzz.random_initial_state(G, P, 2, 44)
    gpu, orc = engine.Table(G, P, 2, True), oracle_lib.OracleTable(G, P, 2, True)
    for t in (gpu, orc):
        t.load_state(st0)
        t.timers_configure(900, 300, 1)
        t.timers_arm(clock.origin())
    b = abi.Batch(1, G)
    fuzz.Fuzzer(G, P, 2, 44, allow_miss=False).round(gpu.read_state(), b, 0)
    rows = np.arange(0, given, dtype=np.int64)
    b32 = engine.pack32(X.subset(b, rows))
    gid, count, now = rows.astype(np.uint32), np.array([given], np.uint32), np.array([clock.origin() + 100], np.int64)

    def filled(dtype, n):
        a = np.zeros(n, dtype=dtype)
        a.view(np.uint8)[:] = FILL
        return a
    row, per = filled(abi.OUT32_DT, 2 * cap), filled(abi.PERSIST32_DT, 2 * cap)
    head, send, ready = filled(abi.SEND_HEAD_DT, 2 * cap), filled(abi.SEND_DT, F * cap + cap), filled(np.uint8, 2 * cap)
    exp_g, exp_e, exp_n = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.zeros(1, np.uint32)
    io = abi.CTick2Io()
    io.rounds, io.head, io.abcd, io.now = 1, b32.head.ctypes.data, b32.abcd.ctypes.data, now.ctypes.data
    io.entry_terms, io.entry_capacity = (b32.entry_terms.ctypes.data, b32.entry_count) if b32.entry_count else (None, 0)
    io.row, io.persist32 = row.ctypes.data, per.ctypes.data
    io.expired_gid, io.expired_epoch, io.expired_count, io.expired_capacity = exp_g.ctypes.data, exp_e.ctypes.data, exp_n.ctypes.data, G
    io.send_head, io.send, io.ready = head.ctypes.data, send.ctypes.data, ready.ctypes.data
    rw = abi.CTick2Rows()
    rw.gid, rw.count, rw.capacity = gid.ctypes.data, count.ctypes.data, cap
    h = C.c_void_p()
    L = engine.lib()
    gpu._check(L.rg_tick2_create_sparse(gpu._h, C.byref(io), C.byref(rw), C.byref(h)))
    gpu._check(L.rg_tick2_launch(h))
    gpu._check(L.rg_tick2_wait(h))
    for a, n in ((row, cap), (per, cap), (head, cap), (send, F * cap), (ready, cap)):
        assert np.all(a[n:].view(np.uint8) == FILL), "a row at or beyond the capacity was written"
    out = abi.Outcome32(cap, wide=False)
    out.row, out.persist = row[:cap].copy(), per[:cap].copy()
    out.persist[(out.row["flags"] & abi.F_PERSIST) == 0] = 0
    got, _ = engine.unpack32(out, 1, cap, st0.role_epoch[:cap])
    first = X.subset(b, rows[:cap])
    oo = orc.submit(first, now=[clock.origin() + 100])
    if not np.any(got.status == abi.NEED_HOST):
        compare_outcomes(oo, got, "the first `capacity` rows")
        ho, so = orc.replicate(gid=gid[:cap])
        assert np.array_equal(head[:cap]["is_leader"], ho["is_leader"]) and np.array_equal(send[:F * cap].reshape(F, cap).T["kind"], so["kind"])
        st, ref = gpu.read_state(), orc.read_state()
        assert np.array_equal(st.current_term, ref.current_term) and np.array_equal(st.role, ref.role)
    assert L.rg_tick2_destroy(h) == 0
    gpu.close()
    orc.close()


# ---- refusals: on the host, with a message, before any launch -------------------------------------------------------------------------------
def _refused(t, rc, text):
    assert rc < 0 and text in engine.lib().rg_last_error(t._h), (rc, engine.lib().rg_last_error(t._h))


def test_submit32c_sparse_refuses_what_the_header_says():
    G = 64
    t = engine.Table(G, 3)
    L = engine.lib()
    before = t.read_state()

    def call(gid, rounds=1, count=None, drop_gid=False):
        gid = np.asarray(gid, dtype=np.uint32)
        n = len(gid) if count is None else count
        rows = rounds * n
        b = abi.Batch32(rounds, n, None if drop_gid else gid, np.zeros(rows, abi.HEAD_DT), np.zeros(rows, abi.QUAD32_DT), np.zeros(1, np.int32), 0)
        cb, co = b.as_struct(), abi.Outcome32(rows, wide=False).as_struct()
        return L.rg_submit32c_sparse(t._h, C.byref(cb), C.byref(co), abi.MEM_HOST)
    _refused(t, call([1, 2, G]), b"out of range")
    _refused(t, call([1, 3, 3]), b"strictly ascending")
    _refused(t, call([5, 4]), b"strictly ascending")
    _refused(t, call([1, 2], rounds=2), b"exactly one round")
    _refused(t, call(np.arange(G + 1), count=G + 1), b"rows for")
    _refused(t, call([1, 2], drop_gid=True), b"gid is required")
    cb = abi.Batch32(1, 2, np.array([1, 2], np.uint32), np.zeros(2, abi.HEAD_DT), np.zeros(2, abi.QUAD32_DT), np.zeros(1, np.int32), 0).as_struct()
    co = abi.Outcome32(2, wide=True).as_struct()
    co.wide.logfx = None
    _refused(t, L.rg_submit32c_sparse(t._h, C.byref(cb), C.byref(co), abi.MEM_HOST), b"all three or none")
    after = t.read_state()
    for f in before.fields():
        assert np.array_equal(getattr(before, f), getattr(after, f)), f      # nothing was launched
    t.close()
    big = engine.Table(16, abi.MAX_COMPACT_CLUSTER + 1)
    cb = abi.Batch32(1, 1, np.array([1], np.uint32), np.zeros(1, abi.HEAD_DT), np.zeros(1, abi.QUAD32_DT), np.zeros(1, np.int32), 0).as_struct()
    co = abi.Outcome32(1, wide=False).as_struct()
    _refused(big, L.rg_submit32c_sparse(big._h, C.byref(cb), C.byref(co), abi.MEM_HOST), b"wide rows")
    big.close()


def test_tick2_create_sparse_refuses_what_the_header_says():
    G = 64
    t = engine.Table(G, 3)
    L = engine.lib()
    cols = dict(head=np.zeros(G, abi.HEAD_DT), abcd=np.zeros(G, abi.QUAD32_DT), now=np.zeros(2, np.int64), row=np.zeros(G, abi.OUT32_DT),
                persist32=np.zeros(G, abi.PERSIST32_DT))
    gid, count = np.arange(G, dtype=np.uint32), np.zeros(1, np.uint32)

    def create(table=t, rounds=1, capacity=G, gid_=gid, count_=count, rows=True):
        io = abi.CTick2Io()
        io.rounds = rounds
        for k, v in cols.items():
            setattr(io, k, v.ctypes.data)
        rw = abi.CTick2Rows()
        rw.gid, rw.count, rw.capacity = (None if gid_ is None else gid_.ctypes.data), (None if count_ is None else count_.ctypes.data), capacity
        h = C.c_void_p()
        rc = L.rg_tick2_create_sparse(table._h, C.byref(io), C.byref(rw) if rows else None, C.byref(h))
        assert rc == 0 or not h.value
        return rc, h
    _refused(t, create(rounds=2)[0], b"exactly one round")
    _refused(t, create(capacity=0)[0], b"capacity")
    _refused(t, create(capacity=G + 1)[0], b"capacity")
    _refused(t, create(gid_=None)[0], b"gid and count are required")
    _refused(t, create(count_=None)[0], b"gid and count are required")
    _refused(t, create(rows=False)[0], b"rows is NULL")
    rc, h = create()                                           # ... and takes what it should
    assert rc == 0 and h.value and L.rg_tick2_destroy(h) == 0
    t.close()
    big = engine.Table(16, abi.MAX_COMPACT_CLUSTER + 1)
    _refused(big, create(table=big, capacity=16)[0], b"wide rows")
    big.close()
