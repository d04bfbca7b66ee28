"""Cases for RG_OPT_DEVICE_IN_FLIGHT on the host emulation of the kernels. Run by tests/test_in_flight_cpu.py in a subprocess; TEST INFRASTRUCTURE. The device cases
need the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1); the refusals happen on the host before any launch and run in either mode (`-k refusals`). The cases are those of
tests/test_in_flight_gpu.py at small table sizes (tests/in_flight_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from tests import in_flight_cases as I  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the two-wavefront kernels need the wavefront mode of the emulation")


@device
def test_a_constructed_sequence_gives_the_literal_counts_and_kinds():
    I.constructed_case()


@device
def test_counts_at_the_end_of_a_uint16_neither_wrap_nor_stick():
    I.saturation_case()


@device
@pytest.mark.parametrize("G,P,seed,resident", [(256, 5, 321, False), (200, 5, 77, True), (192, 3, 11, False), (192, 7, 16, True)])
def test_the_tick_in_lockstep_with_the_oracle_and_the_model(G, P, seed, resident):
    """(small tables do not reach every line of MUST_SEE: tests/test_in_flight_cpu.py shows that for the sizes the MI355X runs)"""
    seen = I.lockstep_case(G, P, seed, 25, device_resident=resident, expect_all=False)
    assert seen["command"] > 0 and seen["heartbeat"] > 0 and seen["untriggered"] > 0 and seen["decrement"] > 0 and seen["deep"] > 0, seen


@device
def test_the_tick_in_lockstep_on_a_nine_node_table():
    I.lockstep_case(128, 9, 29, 15, compact_any=True, expect_all=False)


@device
def test_the_tick_in_lockstep_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    I.lockstep_case(128, 5, 5, 15, expect_all=False)


@device
def test_every_group_listed_at_full_depth_equals_the_dense_tick():
    I.same_as_dense_case(128, ticks=5)


@device
def test_the_dense_tick_recorded_as_step_and_tail(monkeypatch):
    monkeypatch.setenv("RG_TICK_NODES", "2")
    I.same_as_dense_case(128, ticks=5)


@device
def test_one_round_equals_the_one_round_sparse_tick():
    I.one_round_case(192, ticks=6)


@device
def test_a_tick_fed_from_the_arrival_log_needs_no_host_column():
    I.assembled_case(200, ticks=20)


@device
def test_the_option_off_is_the_plain_table_bit_for_bit():
    I.option_off_case(G=192, ticks=6)


def test_refusals_happen_before_any_launch():
    I.refusals_case()
