"""Every kernel family at every cluster size, 2 .. 15 nodes, on the host emulation of the kernels. Run by tests/test_follower_sweep_cpu.py in a subprocess;
TEST INFRASTRUCTURE. The two-wavefront kernels need the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1). The cases are those of
tests/test_follower_sweep_gpu.py (tests/follower_sweep_cases.py) but for the wide-row step kernels, whose choice RG_SPLIT makes and the wavefront mode fixes."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
assert os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1", "the two-wavefront kernels need the wavefront mode of the emulation"

from tests import follower_sweep_cases as W  # noqa: E402


@pytest.mark.parametrize("route", W.ROUTES)
@pytest.mark.parametrize("cluster", W.CLUSTERS)
def test_compact_step_kernels_at_every_cluster_size(cluster, route):
    W.step_case(cluster, route)


@pytest.mark.parametrize("nodes", W.RECORDINGS)
@pytest.mark.parametrize("cluster", W.CLUSTERS)
def test_dense_tick_recordings_at_every_cluster_size(cluster, nodes):
    W.dense_tick_case(cluster, nodes)


@pytest.mark.parametrize("cluster", W.CLUSTERS)
def test_sparse_tick_at_every_cluster_size(cluster):
    W.sparse_tick_case(cluster)


@pytest.mark.parametrize("cluster", W.CLUSTERS)
def test_sparse_tick_with_rounds_at_every_cluster_size(cluster):
    W.rounds_tick_case(cluster)
