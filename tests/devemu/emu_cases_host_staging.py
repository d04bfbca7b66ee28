"""Cases for the staging buffers of the RG_MEM_HOST entry points under changing shapes, on the host emulation of the kernels. Run by
tests/test_host_staging_cpu.py in a subprocess; TEST INFRASTRUCTURE. The compact-row kernels and the ballot-compacted list of fired tickets need the WAVEFRONT
mode (RG_EMU_WAVES=1, RG_SPLIT=1). The cases are those of tests/test_host_staging_gpu.py, at the same table sizes (tests/host_staging_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
assert os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1", "the kernels need the wavefront mode of the emulation"

from tests import host_staging_cases as H  # noqa: E402


@pytest.mark.parametrize("G,P,seed", [(192, 3, 11), (130, 5, 12)])
def test_staging_buffers_serve_rising_and_falling_shapes(G, P, seed):
    """192 groups of 3 nodes; 130 groups of 5: off a multiple of 64, and a second follower count"""
    assert H.changing_shapes_case(G, P, seed) >= 20
