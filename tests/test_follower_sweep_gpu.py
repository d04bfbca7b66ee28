"""Every kernel family at every cluster size, 2 .. 15 nodes, on the MI355X (tests/follower_sweep_cases.py): the launch of each family picks the kernel
instantiation by the follower count, and every one of the fourteen is reached here and held bit-exactly against the CPU oracle."""
import pytest

from tests import follower_sweep_cases as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", W.ROUTES)
@pytest.mark.parametrize("cluster", W.CLUSTERS)
def test_compact_step_kernels_at_every_cluster_size(cluster, route):
    W.step_case(cluster, route)


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("cluster", W.CLUSTERS)
def test_wide_row_step_kernels_at_every_cluster_size(monkeypatch, cluster, split):
    monkeypatch.setenv("RG_SPLIT", split)                     # (read at rg_table_create: 0 = step_kernel, 1 = step_split_kernel)
    W.wide_step_case(cluster)


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
