"""Cases for the carry of an assembler (rg_assembler_carry_* / rg_route32_carry) on the host emulation of the kernels. Run by tests/test_carry_cpu.py in a
subprocess; TEST INFRASTRUCTURE. The device cases need the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1: ballots and barriers meet); the refusals happen on the
host before any launch and run in the lane-serial mode (`-k refuses`). The cases are those of tests/test_carry_gpu.py at small table sizes
(tests/carry_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from tests import carry_cases as K  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("G,seed,memory", [(130, 3, False), (300, 4, False), (130, 5, True)])
def test_a_chain_of_carrying_runs_equals_the_model(G, seed, memory):
    """every run of the chain at four carry capacities, both carries, the routed columns; the chain again after a reset; the carry switched off"""
    assert K.chain_case(G, seed, device=memory) >= 24


@device
def test_carried_ticks_equal_ticks_fed_by_hand():
    """assemble -> tick -> rg_route32_carry with no host step, 25 ticks, against today's path fed by hand and the oracle"""
    deferred, resync = K.pipeline_case(300, 3, 21, 25)
    assert deferred > 12 and resync * 4 <= 25


def test_the_carry_refuses_what_the_header_says():
    K.refusals_case()
