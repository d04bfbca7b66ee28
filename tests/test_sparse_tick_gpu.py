"""The sparse forms of the compact-row path on an MI355X: rg_submit32c_sparse (compact rows of a LIST of groups in, compact outcome rows out) and the sparse
device-resident tick (rg_tick2_create_sparse: one recorded graph that decides only the groups that have a row, folds their flags into timers and health,
plans their leaders' sends and readiness, and lists the fired tickets of the whole table). Bit-exact against tests/oracle_lib.OracleTable; the case
functions live in tests/sparse_tick_cases.py (the host emulation runs them at small sizes: tests/test_sparse_tick_cpu.py)."""
import pytest

from tests import sparse_tick_cases as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cluster,seed", [(3, 11), (5, 12), (7, 16)])
def test_standalone_lists_of_groups_in_lockstep_with_the_oracle(cluster, seed):
    """every round a random subset of the fuzzer's dense round — fill cycling through 1.0, 0.5, 0.1, 0.01, counts off a multiple of 64 among them —:
    rows equal the oracle's after unpack32, the raw-row rules of helpers.check_out32_rows hold, groups outside the list keep their state bit for bit"""
    hist, full, _ = X.standalone_case(1024, cluster, 48, seed)
    assert full > 0


@pytest.mark.parametrize("cluster,seed", [(3, 11), (5, 12), (7, 16)])
def test_standalone_lists_of_groups_on_the_64_bit_body(monkeypatch, cluster, seed):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    X.standalone_case(1024, cluster, 24, seed)


# Share of (tick, row) pairs whose tick repaired an RG_NEED_HOST row (left out of that tick's send / readiness comparison; cap 2 %), with this selection
# rule and Fuzzer(allow_miss=False), on the oracle alone: 0 of 56 449, 0 of 13 789 and 0 of 248 328 rows.
@pytest.mark.parametrize("resident", [False, True], ids=["host-pinned", "device-resident"])
@pytest.mark.parametrize("G,seed,ticks", [(4096, 321, 40), (1000, 77, 40), (65600, 5, 10)])
def test_the_sparse_tick_matches_the_oracle(G, seed, ticks, resident):
    """tick k has fill [0, 0.01, 0.1, 0.5, 1.0][k % 5]; its list = a random subset at that fill + the groups whose ticket fired in tick k - 1. Every tick:
    outcome rows, deadlines, health, expired list + epochs + count, send heads and rows, readiness of the listed rows, whole-table state. The run has seen a
    tick without rows in which tickets fired, a full tick, a row count off a multiple of 64, a role conversion, SEND_APPEND rows, ready 0 and 1.
    (65 600 groups: 1 025 workgroups, the 128-VGPR variant.)"""
    X.sparse_tick_case(G, seed, ticks, device_resident=resident)


def test_every_group_listed_equals_the_dense_tick():
    X.same_as_dense_case(4096, ticks=20)


def test_automatic_bases_in_sparse_ticks():
    flushes, moved = X.auto_base_case(1024, 24, 41)
    assert flushes > 1024 and moved > 1024 // 4


def test_a_stale_recording_refuses():
    X.stale_recording_case()
