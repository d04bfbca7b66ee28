"""The cases of tests/election_round_cases.py on the host emulation of the kernels. Run by tests/test_election_round_cpu.py in a subprocess; TEST INFRASTRUCTURE.
The compact-row kernel needs the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1: ballots and barriers meet). Beyond what the GPU test checks, the emulation counts
the rows that leave tier 1 for the general handlers (RG_NOTE_SLOW -> rg_emu_slow_counts): the narrow run must not send one there — every row of these
streams is decided by the election block (or by tier 1.5) itself."""
import ctypes as C
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
assert os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1", "the compact-row kernel needs the wavefront mode of the emulation"

from rafting_amd import engine  # noqa: E402
from tests import election_round_cases as E  # noqa: E402


def slow_counts():
    a, b, c = C.c_long(), C.c_long(), C.c_long()
    engine.lib().rg_emu_slow_counts(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


@pytest.mark.parametrize("route", E.ROUTES)
@pytest.mark.parametrize("P", E.CLUSTERS)
def test_election_rounds_on_the_32_bit_body(P, route):
    assert E.case(P, route, slow_counts=slow_counts) == 0


@pytest.mark.parametrize("P", E.CLUSTERS)
def test_election_rounds_on_the_64_bit_body(P):
    E.case(P, "submit32c", force_wide=True)
