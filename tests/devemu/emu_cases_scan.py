"""Cases for rg_scan and the state lists on the host emulation of the kernels. Run by tests/test_scan_cpu.py in a subprocess; TEST INFRASTRUCTURE. The device cases
need the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1: ballots, shuffles and barriers meet); the refusals happen on the host before any launch and run in either
mode (`-k refuses`; lane-serial: without the scan that follows them). The cases are those of tests/test_scan_gpu.py at small table sizes (tests/scan_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from tests import scan_cases as S  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("G,P", [(200, 3), (64, 2), (1000, 5), (300, 9), (257, 15)])
def test_the_scan_equals_the_model(G, P):
    """group counts on and off a multiple of 64 and of 256, every cluster size class; host memory"""
    assert S.layout_case(G, P, seed=G + P) >= 30


@device
def test_the_scan_equals_the_model_in_device_memory():
    assert S.layout_case(300, 5, seed=7, device=True) >= 30


@device
def test_the_scan_of_a_table_under_traffic_equals_the_model():
    assert S.live_case(G=192, P=3, seed=11, ticks=4) > 0


@device
@pytest.mark.parametrize("point", ["top_all", "rel_floor", "straddle", "rel_hole"])
def test_off_image_agrees_with_the_domain_rule_of_the_edge_cases(point):
    compared, flagged = S.off_image_witness_case(point)
    assert compared > 100 and (flagged > 0) == (point in ("straddle", "rel_hole"))


@device
@pytest.mark.parametrize("bases", [False, True])
def test_off_image_names_the_workgroups_the_step_kernel_decides_in_64_bits(bases):
    assert S.off_image_kernel_case(700, 5, seed=3 + bases, bases=bases) > 0


@device
def test_read_state_list_equals_the_rows_of_read_state():
    assert S.read_list_case(300, 5, seed=1) == 300
    assert S.read_list_case(70, 9, seed=2) == 70


@device
@pytest.mark.parametrize("k", [1, 63, 65, 257])
def test_load_state_list_equals_a_twin_loaded_one_group_at_a_time(k):
    S.load_list_case(600, 5, k, seed=k)


@device
def test_load_state_list_without_the_in_flight_column():
    S.load_list_case(200, 3, 65, seed=9, in_flight=False)


def test_the_state_lists_refuse_what_the_header_says():
    S.list_refusals_case()


def test_scan_refuses_what_the_header_says():
    S.scan_refusals_case(launches=WAVES)
