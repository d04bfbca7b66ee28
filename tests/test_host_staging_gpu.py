"""The grow-only staging buffers of the RG_MEM_HOST entry points on an MI355X: one table takes a sequence of calls whose sizes rise, fall and rise again through
every entry point that stages, a second table takes the same calls through RG_MEM_DEVICE (engine.DeviceBuffer columns), the oracle leads both. The case function
lives in tests/host_staging_cases.py (the host emulation runs it at the same sizes: tests/test_host_staging_cpu.py)."""
import pytest

from tests import host_staging_cases as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("G,P,seed", [(192, 3, 11), (130, 5, 12)])
def test_staging_buffers_serve_rising_and_falling_shapes(G, P, seed):
    """192 groups of 3 nodes; 130 groups of 5: off a multiple of 64, and a second follower count"""
    assert H.changing_shapes_case(G, P, seed) >= 20
