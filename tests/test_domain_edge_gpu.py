"""The 32-bit step body at the top of its value domain and at the floor of the relative indices, on the MI355X (tests/domain_edge_cases.py): the full mixed
traffic of tests/fuzz.py with terms, indices and role epochs just below 2^30 meeting stale terms of 1 and 2, prevLogIndex 0, leaderCommit 0 and epoch 1, through
rg_submit32, rg_submit32c, rg_submit32c_sparse_rounds and one recording of the device-resident tick — every outcome row and the table bit for bit against the
CPU oracle, and rg_wide_body_workgroups() held to the count the documented rule gives (0 for every point but `straddle`: the sign-word body decided).
The compact-row kernels are the same whatever RG_SPLIT says; the wide-row route runs under both settings (step_kernel, step_split_kernel), as
tests/test_gpu_parity.py's step_kernel_variant does for its wide-row variants."""
import pytest

from tests import domain_edge_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", D.ROUTES)
@pytest.mark.parametrize("point,cluster", D.SHAPES)
def test_magnitude_points(point, cluster, route):
    D.case(point, cluster, route)


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("point,cluster", D.SHAPES)
def test_magnitude_points_on_wide_rows(monkeypatch, point, cluster, split):
    monkeypatch.setenv("RG_SPLIT", split)                     # (read at rg_table_create: 0 = step_kernel, 1 = step_split_kernel)
    D.case(point, cluster, "wide_rows")
