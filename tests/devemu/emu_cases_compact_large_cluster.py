"""Cases for RG_OPT_COMPACT_ANY_CLUSTER on the host emulation of the kernels. Run by tests/test_compact_large_cluster_cpu.py in a subprocess; TEST
INFRASTRUCTURE. The decisions need the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1); the refusals happen on the host before any launch and run in either
mode (`-k refuses`). The cases are those of tests/test_compact_large_cluster_gpu.py at small table sizes (tests/compact_large_cluster_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from tests import compact_large_cluster_cases as K  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the two-wavefront kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("route", K.ROUTES)
@pytest.mark.parametrize("cluster,self_slot,pre_vote,seed", K.SHAPES)
def test_fuzz_lockstep_above_seven_nodes_on_compact_rows(cluster, self_slot, pre_vote, seed, route):
    K.lockstep_case(64, 40, cluster, self_slot, pre_vote, seed, route)


@device
@pytest.mark.parametrize("cluster", [9, 15])
def test_the_32_bit_body_decides_config_3(cluster):
    K.body32_case(1000, cluster)


@device
@pytest.mark.parametrize("cluster", [9, 15])
def test_the_32_bit_body_decides_groups_at_two_to_the_forty(cluster):
    K.body32_case(1000, cluster, at_two_to_the_forty=True)


@device
@pytest.mark.parametrize("route", K.ROUTES)
@pytest.mark.parametrize("self_slot", [0, 14])
def test_directed_rows_at_follower_indices_above_seven(self_slot, route):
    K.directed_case(self_slot, route)


@device
@pytest.mark.parametrize("cluster,seed", [(9, 31), (15, 32)])
def test_lists_of_groups_equal_the_dense_launch_and_the_oracle(cluster, seed):
    K.lists_case(200, cluster, seed)


@device
@pytest.mark.parametrize("cluster,seed,resident", [(9, 41, False), (15, 42, True)])
def test_the_device_resident_ticks_match_the_oracle(cluster, seed, resident):
    K.ticks_case(136, cluster, 50, seed, device_resident=resident)


@device
@pytest.mark.parametrize("cluster,seed", [(9, 51), (15, 52)])
def test_the_other_recordings_of_the_tick_match_the_oracle(cluster, seed):
    K.tick_recordings_case(128, cluster, 10, seed)


@device
def test_the_once_per_tick_graph_on_nine_nodes():
    K.tick_graph_case(96, ticks=12)


@device
def test_a_recorded_tick_belongs_to_the_setting_it_was_made_under():
    K.option_recorded_tick_case()


@device
def test_small_clusters_are_decided_the_same_with_the_option_on_and_off():
    K.option_small_cluster_case(128, 30)


# ---- refusals: on the host, with a message, before any launch -------------------------------------------------------------------------------
def test_the_option_off_by_default_refuses_every_compact_entry_point():
    K.option_off_by_default_case()


def test_the_option_refuses_other_values_and_zero_restores_the_refusals():
    K.option_values_case(launch=WAVES)
