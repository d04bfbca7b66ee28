"""Every kernel that takes a clock, at the clock values real hosts pass, on the MI355X (tests/clock_domain_cases.py): the stand-alone timer, health and readiness
calls in a closed loop and the recorded ticks at System.currentTimeMillis()'s magnitude, across 2^31, across 2^32 and at the top of the clock's domain; the
deadline column's marks, deadline == now, the two thresholds of a follower's health and the quorum of Leader.isReady with literal expected values; calls of more
than 64 rounds; the expiry list at its capacities. Everything is also held bit for bit to the CPU oracle."""
import pytest

from tests import clock
from tests import clock_domain_cases as D

pytestmark = pytest.mark.gpu


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
