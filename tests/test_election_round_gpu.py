"""The election block of the 32-bit step body (rg_tier1n.hpp) on an MI355X: the hand-built streams of tests/election_round_cases.py — every sub-block of the
block alone and together, an election row right after a conversion of the same lane, at 5, 3 and 7 nodes — through rg_submit32c, rg_submit32 and the sparse
kernel variant against the oracle, on the 32-bit body (rg_wide_body_workgroups() == 0) and, as the differential, on the 64-bit body (RG_FORCE_WIDE=1)."""
import pytest

from tests import election_round_cases as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", E.ROUTES)
@pytest.mark.parametrize("P", E.CLUSTERS)
def test_election_rounds_on_the_32_bit_body(P, route):
    assert E.case(P, route) == 0


@pytest.mark.parametrize("P", E.CLUSTERS)
def test_election_rounds_on_the_64_bit_body(P):
    E.case(P, "submit32c", force_wide=True)
