"""The clock points of tests/clock_domain_cases.py on the host emulation of the kernels. Run by tests/test_clock_domain_cpu.py in a subprocess; TEST INFRASTRUCTURE.
The cases are those of tests/test_clock_domain_gpu.py. The expiry's ballots and the two-wavefront step kernels need the WAVEFRONT mode (RG_EMU_WAVES=1,
RG_SPLIT=1): in lane-serial mode every lane has a ballot of its own."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
assert os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1", "the ballots of the expiry need the wavefront mode of the emulation"

from tests import clock  # noqa: E402
from tests import clock_domain_cases as D  # noqa: E402


@pytest.mark.parametrize("compact", [False, True], ids=["wide", "compact"])
@pytest.mark.parametrize("cluster", D.CLUSTERS)
@pytest.mark.parametrize("point", D.POINTS)
def test_the_stand_alone_calls_in_a_closed_loop(point, cluster, compact):
    D.loop_case(point, cluster, compact)


def test_two_clocks_that_differ_in_bit_32_draw_different_timeouts():
    D.low_word_case()


@pytest.mark.parametrize("name", D.TICK_CASES)
@pytest.mark.parametrize("point", D.POINTS)
def test_the_recorded_ticks(point, name):
    D.tick_case(point, name)


@pytest.mark.parametrize("origin", [D.POINTS["epoch_ms"], clock.DEFAULT], ids=["epoch_ms", "default"])
def test_directed_boundaries(origin):
    D.boundaries_case(origin)


@pytest.mark.parametrize("pending", [False, True], ids=["", "pending"])
@pytest.mark.parametrize("cluster", range(2, 16))
def test_the_quorum_of_ready_at_every_cluster_size(cluster, pending):
    D.quorum_case(cluster, pending)


@pytest.mark.parametrize("compact", [False, True], ids=["wide", "compact"])
@pytest.mark.parametrize("rounds", D.LONG_ROUNDS)
def test_more_than_64_rounds_in_one_call(rounds, compact):
    D.long_rounds_case(rounds, compact)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("epochs", [False, True], ids=["gids", "epochs"])
@pytest.mark.parametrize("G", D.EXPIRY_GROUPS)
def test_the_expiry_list_at_its_capacities(G, epochs, device):
    D.expiry_case(G, epochs, device)


def test_the_default_origin_gives_the_clocks_the_cases_always_had():
    """every clock the oracle is given by the tick cases of tests/test_gpu_parity.py, tests/sparse_tick_cases.py and tests/in_flight_cases.py at the default origin,
    by digest: recorded before the literals became expressions of tests/clock.py's origin"""
    assert D.default_origin_digest(device=True) == D.DEFAULT_DEVICE_DIGEST
