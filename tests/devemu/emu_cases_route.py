"""Cases for rg_route32 on the host emulation of the kernels. Run by tests/test_route_cpu.py in a subprocess; TEST INFRASTRUCTURE. The device cases need the
WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1: ballots and barriers meet); the refusals happen on the host before any launch and run in either mode (`-k refuses`;
lane-serial: without the part that needs an earlier run of the assembler). The cases are those of tests/test_route_gpu.py at small table sizes
(tests/route_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from tests import route_cases as R  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("G,seed", [(200, 3), (64, 4), (1000, 5), (4097, 6)])
def test_the_routed_layout_equals_the_model(G, seed):
    """group counts on and off a multiple of 64; every input routed twice on one assembler (host memory)"""
    assert R.layout_case(G, seed) > 20


@device
def test_the_routed_layout_equals_the_model_in_device_memory():
    assert R.layout_case(300, 7, device=True) > 20


@device
@pytest.mark.parametrize("G,P,seed,resident", [(192, 3, 11, False), (256, 5, 321, True)])
def test_routed_ticks_in_lockstep_with_the_oracle(G, P, seed, resident):
    R.routed_tick_case(G, seed, 25, P=P, device_resident=resident)


@device
def test_routed_ticks_with_device_resident_in_flight_counts():
    assert R.in_flight_case(G=192, seed=11, ticks=20, P=3) > 0


def test_route32_refuses_what_the_header_says():
    R.refusals_case(launches=WAVES)
