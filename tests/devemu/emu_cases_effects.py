"""Cases for rg_effects32 on the host emulation of the kernels. Run by tests/test_effects_cpu.py in a subprocess; TEST INFRASTRUCTURE. The device cases need the
WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1: ballots and barriers meet); the refusals happen on the host before any launch and run in either mode (`-k refuses`;
lane-serial: without the call that shows nothing was launched). The cases are those of tests/test_effects_gpu.py at the smallest sizes (tests/effects_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from tests import effects_cases as E  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("memory", ["host", "device"])
def test_the_lists_equal_the_model(memory):
    """1000 rows x 4 rounds: a row count off a multiple of 64"""
    assert E.layout_case(1000, 4, 5, device=memory == "device") == 18


@device
@pytest.mark.parametrize("route", ["dense", "sparse", "tick"])
def test_the_lists_give_what_the_full_walk_finds(route):
    """(seed 2 at 256 groups x 5 nodes, 50 launches: truncations, groups that commit twice in a launch and an RG_NEED_HOST cell, on every route — the tick's stream
    differs from the other two, its send step prepares the leaders)"""
    truncs, multi, need = E.decisions_case(256, 5, 2, 50, route)
    assert truncs > 0 and multi > 0 and need > 0, (truncs, multi, need)


def test_effects32_refuses_what_the_header_says():
    E.refusals_case(launches=WAVES)
