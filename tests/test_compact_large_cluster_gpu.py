"""RG_OPT_COMPACT_ANY_CLUSTER on the MI355X: tables of 8 .. 15 nodes through every compact entry point and every tick, bit-identical to the CPU oracle
(tests/compact_large_cluster_cases.py). Without the option — the parent of this change — every case but the two "off" ones fails: with "unknown option 3"
where a case sets it, with "wide rows" where it submits."""
import pytest

from tests import compact_large_cluster_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", K.ROUTES)
@pytest.mark.parametrize("cluster,self_slot,pre_vote,seed", K.SHAPES)
def test_fuzz_lockstep_above_seven_nodes_on_compact_rows(cluster, self_slot, pre_vote, seed, route):
    K.lockstep_case(256, 90, cluster, self_slot, pre_vote, seed, route)


@pytest.mark.parametrize("cluster", [9, 15])
def test_the_32_bit_body_decides_config_3(cluster):
    K.body32_case(65536, cluster)


@pytest.mark.parametrize("cluster", [9, 15])
def test_the_32_bit_body_decides_groups_at_two_to_the_forty(cluster):
    K.body32_case(65536, cluster, at_two_to_the_forty=True)


@pytest.mark.parametrize("route", K.ROUTES)
@pytest.mark.parametrize("self_slot", [0, 14])
def test_directed_rows_at_follower_indices_above_seven(self_slot, route):
    K.directed_case(self_slot, route)


@pytest.mark.parametrize("cluster,seed", [(9, 31), (15, 32)])
def test_lists_of_groups_equal_the_dense_launch_and_the_oracle(cluster, seed):
    K.lists_case(1000, cluster, seed)


@pytest.mark.parametrize("cluster,seed,resident", [(9, 41, False), (15, 42, True)])
def test_the_device_resident_ticks_match_the_oracle(cluster, seed, resident):
    K.ticks_case(1024 + 40, cluster, 50, seed, device_resident=resident)


@pytest.mark.parametrize("cluster,seed", [(9, 51), (15, 52)])
def test_the_other_recordings_of_the_tick_match_the_oracle(cluster, seed):
    K.tick_recordings_case(512, cluster, 16, seed)


def test_the_once_per_tick_graph_on_nine_nodes():
    K.tick_graph_case(192)


def test_the_option_is_off_by_default():
    K.option_off_by_default_case()


def test_the_option_takes_zero_and_one_only():
    K.option_values_case()


def test_a_recorded_tick_belongs_to_the_setting_it_was_made_under():
    K.option_recorded_tick_case()


def test_small_clusters_are_decided_the_same_with_the_option_on_and_off():
    K.option_small_cluster_case(384, 60)
