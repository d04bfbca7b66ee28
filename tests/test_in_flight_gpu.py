"""RG_OPT_DEVICE_IN_FLIGHT on an MI355X: the table keeps State.requestInFlight per (group, follower) and the send step of a recorded tick derives which handler sent
and how much is in flight from the tick's own rows. The case functions and the model they hold the device to live in tests/in_flight_cases.py (the host emulation
runs them at small sizes: tests/test_in_flight_cpu.py). Every test here fails on a library that refuses the option."""
import pytest

from tests import in_flight_cases as I

pytestmark = pytest.mark.gpu

# (groups, cluster, seed, ticks, number of the first tick): sparse_rounds_cases.lead()'s streams; tests/test_in_flight_cpu.py shows on the oracle and the model
# alone that each reaches every line of in_flight_cases.MUST_SEE. lead() takes its depth from the tick's number, DEPTHS[(k // 5) % 5] = 1, 2, 3, .., so the
# ten-tick run counts its ticks from 5 (depths 2 and 3): ticks 0 .. 9 reach no depth of 3 at any seed.
SIZES = [(1000, 5, 77, 25, 0), (1024, 3, 11, 25, 0), (1024, 7, 16, 25, 0), (65600, 5, 5, 10, 5)]
NINE_NODES = (1024, 9, 29, 25, 0)


def test_a_constructed_sequence_gives_the_literal_counts_and_kinds():
    I.constructed_case()


def test_counts_at_the_end_of_a_uint16_neither_wrap_nor_stick():
    I.saturation_case()


@pytest.mark.parametrize("resident", [False, True], ids=["host-pinned", "device-resident"])
@pytest.mark.parametrize("G,P,seed,ticks,first", SIZES)
def test_the_tick_in_lockstep_with_the_oracle_and_the_model(G, P, seed, ticks, first, resident):
    I.lockstep_case(G, P, seed, ticks, first=first, device_resident=resident)


def test_the_tick_in_lockstep_on_a_nine_node_table():
    G, P, seed, ticks, first = NINE_NODES
    I.lockstep_case(G, P, seed, ticks, first=first, compact_any=True)


def test_every_group_listed_at_full_depth_equals_the_dense_tick():
    I.same_as_dense_case(4096)


def test_the_dense_tick_recorded_as_step_and_tail_equals_the_sparse_tick(monkeypatch):
    """RG_TICK_NODES=2 records the dense tick as the step kernel + tick_tail_kernel (what a RG_FORCE_WIDE table's tick is, too): the tail with the option on"""
    monkeypatch.setenv("RG_TICK_NODES", "2")
    I.same_as_dense_case(1024, ticks=6)


def test_one_round_equals_the_one_round_sparse_tick():
    I.one_round_case(4096)


def test_a_tick_fed_from_the_arrival_log_needs_no_host_column():
    I.assembled_case(1000, ticks=20)


def test_refusals_happen_before_any_launch():
    I.refusals_case()


def test_the_option_off_is_the_plain_table_bit_for_bit():
    I.option_off_case()
