"""rg_scan and the state exchange by a list of groups on an MI355X: the class word of every group, the counts and the ascending list bit for bit against the numpy
model of the header's contract in both memspaces; RG_SCAN_OFF_IMAGE against tests/domain_edge_cases.state_out_of_domain and against the step kernel itself;
rg_load_state_list against a twin table loaded one group at a time. The case functions live in tests/scan_cases.py (the host emulation runs them at small sizes:
tests/test_scan_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import scan_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", [False, True], ids=["host-memory", "device-memory"])
@pytest.mark.parametrize("G,P", S.SIZES)
def test_the_scan_equals_the_model(G, P, device):
    """random states (all three roles, prepared and unprepared leaders, empty logs, 1 to 4 runs, pending bits, lags on both sides of the threshold), index bases,
    armed and fired timers; select-all, select-none, any, all, none and a combination; list capacities of 0, below and above the count; every input scanned twice.
    Group counts off a multiple of 64, more than 1024 wavefronts so that the prefix sum's second level runs, more than 7 nodes. Sentinel words prove every NOT
    TOUCHED clause."""
    assert S.layout_case(G, P, seed=G + P, device=device) >= 30


def test_the_scan_of_a_table_under_traffic_equals_the_model():
    assert S.live_case() > 0


@pytest.mark.parametrize("point", ["top_all", "rel_floor", "rel_top", "straddle", "rel_hole"])
def test_off_image_agrees_with_the_domain_rule_of_the_edge_cases(point):
    compared, flagged = S.off_image_witness_case(point)
    assert compared > 100 and (flagged > 0) == (point in ("straddle", "rel_hole")), (point, compared, flagged)


@pytest.mark.parametrize("bases", [False, True], ids=["no-bases", "bases"])
@pytest.mark.parametrize("G,P", [(1000, 5), (4096, 3)])
def test_off_image_names_the_workgroups_the_step_kernel_decides_in_64_bits(G, P, bases):
    assert S.off_image_kernel_case(G, P, seed=G + bases, bases=bases) > 0


@pytest.mark.parametrize("G,P", [(1000, 3), (65600, 5), (300, 9)])
def test_read_state_list_equals_the_rows_of_read_state(G, P):
    assert S.read_list_case(G, P, seed=G) == G


@pytest.mark.parametrize("G", [4096, 65600])
@pytest.mark.parametrize("k", [1, 63, 65, 1000])
def test_load_state_list_equals_a_twin_loaded_one_group_at_a_time(G, k):
    S.load_list_case(G, 5, k, seed=G + k)


def test_load_state_list_without_the_in_flight_column():
    S.load_list_case(1000, 3, 65, seed=9, in_flight=False)


def test_the_state_lists_refuse_what_the_header_says():
    S.list_refusals_case()


def test_scan_refuses_what_the_header_says():
    S.scan_refusals_case()


def test_a_pageable_pointer_is_refused_in_the_device_memspace():
    """(the emulation cannot tell pageable from page-locked memory: this refusal is checked here) — and nothing was launched: the next scan is the model's"""
    G = 300
    t = engine.Table(G, 3)
    t.load_state(S.random_state(G, 3, np.random.default_rng(4)))
    summary, gids, words = np.zeros(abi.SCAN_SUMMARY, np.uint64), np.zeros(8, np.uint32), np.zeros(G, np.uint32)
    dev = engine.DeviceBuffer(t, 4096)
    q = abi.CScanQuery()
    for kw, what in ((dict(bits=words.ctypes.data, list=dev.ptr, summary=dev.ptr), "bits"), (dict(bits=None, list=gids.ctypes.data, summary=dev.ptr), "list"),
                     (dict(bits=None, list=dev.ptr, summary=summary.ctypes.data), "summary")):
        r = abi.CScanResult(list_capacity=8, **kw)
        rc = engine.lib().rg_scan(t._h, C.byref(q), C.byref(r), abi.MEM_DEVICE)
        msg = engine.lib().rg_last_error(t._h)
        assert rc == -1 and b"neither device memory" in msg and what.encode() in msg, (rc, msg)
    dev.free()
    query = dict(any=abi.SCAN_LEADER | abi.SCAN_NO_LEADER, lag=3)
    S.check_scan(S.scan_device(t, query, G), S.model_of(t, **query), G, "after a refusal")
    t.close()
