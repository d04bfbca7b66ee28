"""R rounds of a list of groups in ONE launch on an MI355X: rg_submit32c_sparse_rounds (stand-alone) and the sparse device-resident tick that reads its row count
and its depth when the graph runs (rg_tick2_create_sparse_rounds). The fuzzed cases lead with tests/oracle_lib.OracleTable round by round and hand all R rounds
to the device in one call; the case functions live in tests/sparse_rounds_cases.py (the host emulation runs them at small sizes: tests/test_sparse_rounds_cpu.py)."""
import pytest

from tests import sparse_rounds_cases as X

pytestmark = pytest.mark.gpu

# (groups, cluster, seed, launches). The device answers RG_NEED_HOST for a few rows of such streams (the oracle never does): the cases repair them like a
# host and cap their share at 2 % (tests/sparse_rounds_cases.py, module docstring)
SIZES = [(4096, 5, 321, 50), (1000, 5, 77, 50), (1024, 3, 11, 50), (1024, 7, 16, 50), (65600, 5, 5, 15)]
TICKS = [(4096, 5, 321, 50), (1000, 5, 77, 50), (1024, 3, 11, 25), (1024, 7, 16, 25), (65600, 5, 5, 15)]


@pytest.mark.parametrize("G,P,seed,launches", SIZES)
def test_standalone_rounds_in_lockstep_with_the_oracle(G, P, seed, launches):
    """launch k: fill [0, 0.01, 0.1, 0.5, 1.0][k % 5], depth [1, 2, 3, 5, 8][(k // 5) % 5], about 40 % of the rows RG_EV_NONE. Every outcome row after unpack32,
    helpers.check_out32_rows on the raw rows, whole-table state, groups outside the list bit for bit. The run has seen a depth >= 3, a row count off a multiple
    of 64, a full list and a role conversion before the last round. (65 600 groups: 1 025 workgroups, the 128-VGPR variant.)"""
    X.standalone_rounds_case(G, P, seed, launches)


@pytest.mark.parametrize("G,P,seed,launches", SIZES[:4])
def test_standalone_rounds_on_the_64_bit_body(monkeypatch, G, P, seed, launches):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    X.standalone_rounds_case(G, P, seed, 25)


@pytest.mark.parametrize("resident", [False, True], ids=["host-pinned", "device-resident"])
@pytest.mark.parametrize("G,P,seed,ticks", TICKS)
def test_the_tick_with_a_depth_matches_the_oracle(G, P, seed, ticks, resident):
    """the same stream through a tick recorded for 8 rounds, plus last tick's fired groups in every list. Every tick also: deadlines, health columns, the expired
    list with epochs and count, send heads and rows and the readiness of the listed rows. The run has also seen a tick without rows in which tickets fired,
    SEND_APPEND rows, ready 0 and ready 1."""
    X.rounds_tick_case(G, seed, ticks, P=P, device_resident=resident)


def test_need_host_inside_a_launch():
    stopped, skipped = X.need_host_case()
    assert stopped > 0 and skipped > 0


@pytest.mark.parametrize("resident", [False, True], ids=["host-pinned", "device-resident"])
def test_one_round_equals_the_one_round_forms(resident):
    X.one_round_case(4096, device_resident=resident)


@pytest.mark.parametrize("pointer", [True, False], ids=["rounds-at-the-maximum", "no-rounds-pointer"])
def test_every_group_listed_at_full_depth_equals_the_dense_tick(pointer):
    X.same_as_dense_case(4096, R=4, ticks=10, depth_pointer=pointer)


def test_a_depth_below_the_maximum_leaves_the_rest_untouched():
    X.partial_depth_case(1000, n=333)


def test_automatic_bases_across_rounds():
    flushes, moved = X.auto_base_rounds_case(1024, 12, 41)
    assert flushes > 1024 and moved > 1024 // 4


def test_a_stale_recording_refuses_and_a_tick_outlives_its_table():
    X.stale_recording_case()


def test_device_memory_gives_the_rows_of_host_memory():
    assert X.device_memspace_case() > 64


def test_a_rounds_pointer_in_pageable_memory_is_refused():
    """(the emulation cannot tell pageable from page-locked memory: this refusal is checked here)"""
    import ctypes as C

    import numpy as np

    from rafting_amd import abi, engine
    G = 64
    t = engine.Table(G, 3)
    tick = engine.Tick2(t, 2, expired_cap=G, sparse_cap=G, sparse_rounds=True)      # (its columns: device-visible all of them)
    before = t.read_state()
    pageable = np.ones(1, np.uint32)
    rw = abi.CTick2Rounds()
    rw.gid, rw.count, rw.rounds, rw.capacity = tick.rows.gid, tick.rows.count, pageable.ctypes.data, G
    h = C.c_void_p()
    rc = engine.lib().rg_tick2_create_sparse_rounds(t._h, C.byref(tick.io), C.byref(rw), C.byref(h))
    assert rc < 0 and not h.value and b"rounds is neither device memory" in engine.lib().rg_last_error(t._h)
    after = t.read_state()
    for f in before.fields():
        assert np.array_equal(getattr(before, f), getattr(after, f)), f
    tick.close()
    t.close()
