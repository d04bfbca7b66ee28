"""The magnitude points of tests/domain_edge_cases.py on the host emulation of the kernels. Run by tests/test_domain_edge_cpu.py in a subprocess; TEST INFRASTRUCTURE.
The 32-bit body is the two-wavefront step32_kernel: it needs the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1), as in tests/devemu/emu_cases_waves.py. The cases are
those of tests/test_domain_edge_gpu.py; rg_wide_body_workgroups() counts the workgroups of the 64-bit body here as on the device, and rg_emu_fallbacks — the
emulation's own count of the same event — must agree with it."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
assert os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1", "the two-wavefront kernels need the wavefront mode of the emulation"

from tests import domain_edge_cases as D  # noqa: E402
from tests import test_gpu_parity as T  # noqa: E402


@pytest.mark.parametrize("route", D.ROUTES)
@pytest.mark.parametrize("point,cluster", D.SHAPES)
def test_magnitude_points(point, cluster, route):
    T.emu_fallbacks()
    wide = D.case(point, cluster, route)
    fb = T.emu_fallbacks()
    # (the tick case ends with one more compact launch after its count was read: at `straddle` and `rel_hole` that launch sends the second workgroup to the 64-bit body again)
    assert fb is not None and (fb == wide or (route == "tick" and fb == wide + 1)), (fb, wide)
    if point not in D.SPLIT_POINTS:
        assert fb == 0, "%d workgroups fell back to the 64-bit body" % fb


@pytest.mark.parametrize("point,cluster", D.SHAPES)
def test_magnitude_points_on_wide_rows(point, cluster):
    """step_split_kernel (the wavefront mode fixes RG_SPLIT=1)"""
    D.case(point, cluster, "wide_rows")
