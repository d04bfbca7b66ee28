"""Cases for rg_submit32c_sparse_rounds and the sparse tick with a depth (rg_tick2_create_sparse_rounds) on the host emulation of the kernels. Run by
tests/test_sparse_rounds_cpu.py in a subprocess; TEST INFRASTRUCTURE. The device cases need the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1); the refusals
happen on the host before any launch and run in either mode (`-k refuses`). The cases are those of tests/test_sparse_rounds_gpu.py at small table sizes
(tests/sparse_rounds_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from rafting_amd import abi, engine  # noqa: E402
from tests import sparse_rounds_cases as X  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the two-wavefront kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("G,P,seed", [(192, 3, 11), (256, 5, 321), (192, 7, 16)])
def test_standalone_rounds_in_lockstep_with_the_oracle(G, P, seed):
    X.standalone_rounds_case(G, P, seed, 25)


@device
def test_standalone_rounds_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    X.standalone_rounds_case(128, 5, 5, 25)


@device
@pytest.mark.parametrize("G,P,seed,resident", [(256, 5, 321, False), (200, 5, 77, True), (192, 3, 11, False), (192, 7, 16, True)])
def test_the_tick_with_a_depth_matches_the_oracle(G, P, seed, resident):
    X.rounds_tick_case(G, seed, 25, P=P, device_resident=resident)


@device
def test_the_tick_with_a_depth_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    X.rounds_tick_case(128, 5, 25)


@device
def test_need_host_inside_a_launch():
    stopped, skipped = X.need_host_case(G=256)
    assert stopped > 0 and skipped > 0


@device
def test_one_round_equals_the_one_round_forms():
    X.one_round_case(192, ticks=8)


@device
@pytest.mark.parametrize("pointer", [True, False])
def test_every_group_listed_at_full_depth_equals_the_dense_tick(pointer):
    X.same_as_dense_case(128, R=4, ticks=5, depth_pointer=pointer)


@device
def test_a_depth_below_the_maximum_leaves_the_rest_untouched():
    X.partial_depth_case(192, n=70)


@device
def test_automatic_bases_across_rounds():
    flushes, moved = X.auto_base_rounds_case(128, 8, 31)
    assert flushes > 16 and moved > 0


@device
def test_a_stale_recording_is_turned_down_and_a_tick_outlives_its_table():
    X.stale_recording_case()


@device
def test_device_memory_gives_the_rows_of_host_memory():
    assert X.device_memspace_case(G=200) > 0


# ---- refusals: on the host, with a message, before any launch -------------------------------------------------------------------------------
def _refused(t, rc, text):
    assert rc < 0 and text in engine.lib().rg_last_error(t._h), (rc, engine.lib().rg_last_error(t._h))


def _unchanged(t, before):
    after = t.read_state()
    for f in before.fields():
        assert np.array_equal(getattr(before, f), getattr(after, f)), f      # nothing was launched


def test_submit32c_sparse_rounds_refuses_what_the_header_says():
    G = 64
    t = engine.Table(G, 3)
    L = engine.lib()
    before = t.read_state()

    def batch(gid, rounds=3, count=None, drop_gid=False):
        gid = np.asarray(gid, dtype=np.uint32)
        n = len(gid) if count is None else count
        rows = rounds * n
        return abi.Batch32(rounds, n, None if drop_gid else gid, np.zeros(rows, abi.HEAD_DT), np.zeros(rows, abi.QUAD32_DT), np.zeros(1, np.int32), 0), rows

    def call(*a, **kw):
        b, rows = batch(*a, **kw)
        cb, co = b.as_struct(), abi.Outcome32(max(rows, 1), wide=False).as_struct()
        return L.rg_submit32c_sparse_rounds(t._h, C.byref(cb), C.byref(co), abi.MEM_HOST)
    _refused(t, call([1, 2, G]), b"out of range")
    _refused(t, call([1, 3, 3]), b"strictly ascending")
    _refused(t, call([5, 4]), b"strictly ascending")
    _refused(t, call([1, 2], rounds=0), b"rounds must be >= 1")
    _refused(t, call(np.arange(G + 1), count=G + 1), b"rows for")
    _refused(t, call([1, 2], drop_gid=True), b"gid is required")
    b, rows = batch([1, 2])
    cb, co = b.as_struct(), abi.Outcome32(rows, wide=True).as_struct()
    co.wide.logfx = None
    _refused(t, L.rg_submit32c_sparse_rounds(t._h, C.byref(cb), C.byref(co), abi.MEM_HOST), b"all three or none")
    co = abi.Outcome32(rows, wide=False).as_struct()
    co.persist = None
    _refused(t, L.rg_submit32c_sparse_rounds(t._h, C.byref(cb), C.byref(co), abi.MEM_HOST), b"head, abcd, row and persist are required")
    _unchanged(t, before)
    # the one-round forms keep their refusal, word for word
    b1 = abi.Batch32(2, 2, np.array([1, 2], np.uint32), np.zeros(4, abi.HEAD_DT), np.zeros(4, abi.QUAD32_DT), np.zeros(1, np.int32), 0)
    cb, co = b1.as_struct(), abi.Outcome32(4, wide=False).as_struct()
    _refused(t, L.rg_submit32c_sparse(t._h, C.byref(cb), C.byref(co), abi.MEM_HOST), b"sparse batches carry exactly one round")
    # the host-side mirror of the automatic bases takes the shape, and still turns down a list that does not fit the groups
    base = np.zeros(G, np.int64)
    assert L.rg_index_base_advance32(C.byref(cb), 1 << 28, G, base.ctypes.data) == 0
    assert L.rg_index_base_advance32(C.byref(cb), 1 << 28, 2, base.ctypes.data) == -2
    t.close()
    big = engine.Table(16, abi.MAX_COMPACT_CLUSTER + 1)
    b, rows = batch([1])
    cb, co = b.as_struct(), abi.Outcome32(rows, wide=False).as_struct()
    _refused(big, L.rg_submit32c_sparse_rounds(big._h, C.byref(cb), C.byref(co), abi.MEM_HOST), b"wide rows")
    big.close()


def test_tick2_create_sparse_rounds_refuses_what_the_header_says():
    G, R = 64, 4
    t = engine.Table(G, 3)
    L = engine.lib()
    before = t.read_state()
    cols = dict(head=np.zeros(R * G, abi.HEAD_DT), abcd=np.zeros(R * G, abi.QUAD32_DT), now=np.zeros(R, np.int64), row=np.zeros(R * G, abi.OUT32_DT),
                persist32=np.zeros(R * G, abi.PERSIST32_DT))
    gid, count, depth = np.arange(G, dtype=np.uint32), np.zeros(1, np.uint32), np.ones(1, np.uint32)

    def create(table=t, rounds=R, capacity=G, gid_=gid, count_=count, depth_=depth, rows=True, drop=None):
        io = abi.CTick2Io()
        io.rounds = rounds
        for k, v in cols.items():
            setattr(io, k, None if k == drop else v.ctypes.data)
        rw = abi.CTick2Rounds()
        rw.gid, rw.count, rw.capacity = (None if gid_ is None else gid_.ctypes.data), (None if count_ is None else count_.ctypes.data), capacity
        rw.rounds = None if depth_ is None else depth_.ctypes.data
        h = C.c_void_p()
        rc = L.rg_tick2_create_sparse_rounds(table._h, C.byref(io), C.byref(rw) if rows else None, C.byref(h))
        assert rc == 0 or not h.value
        return rc, h
    _refused(t, create(rounds=0)[0], b"1 .. 64")
    _refused(t, create(rounds=65)[0], b"1 .. 64")
    _refused(t, create(capacity=0)[0], b"capacity")
    _refused(t, create(capacity=G + 1)[0], b"capacity")
    _refused(t, create(gid_=None)[0], b"gid and count are required")
    _refused(t, create(count_=None)[0], b"gid and count are required")
    _refused(t, create(rows=False)[0], b"rows is NULL")
    _refused(t, create(drop="persist32")[0], b"head, abcd, now, row and persist32 are required")
    _unchanged(t, before)
    for kw in (dict(), dict(depth_=None), dict(rounds=1)):      # ... and takes what it should, with or without a `rounds` pointer
        rc, h = create(**kw)
        assert rc == 0 and h.value and L.rg_tick2_destroy(h) == 0
    # the one-round form keeps its refusal, word for word
    io = abi.CTick2Io()
    io.rounds = 2
    for k, v in cols.items():
        setattr(io, k, v.ctypes.data)
    rw = abi.CTick2Rows()
    rw.gid, rw.count, rw.capacity = gid.ctypes.data, count.ctypes.data, G
    h = C.c_void_p()
    _refused(t, L.rg_tick2_create_sparse(t._h, C.byref(io), C.byref(rw), C.byref(h)), b"a list of groups carries exactly one round")
    t.close()
    big = engine.Table(16, abi.MAX_COMPACT_CLUSTER + 1)
    _refused(big, create(table=big, capacity=16)[0], b"wide rows")
    big.close()
