"""bench.py stages the stream in blocks of groups, one process per block, interleaved round by round: the batches must be the very rows one
ReplayGenerator + pack32 give (a group's stream depends on its global id only), with the same decision and byte counts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from rafting_amd import workload  # noqa: E402


def test_staging_in_blocks_of_groups_gives_the_batches_of_one_generator():
    for number, groups, first_gid in ((3, 4096, 0), (5, 4096, 0), (4, 3072, 2048)):
        cfg = workload.config(number, groups + first_gid)
        F = cfg.cluster - 1
        one = list(bench.stage_compact(cfg, first_gid, groups, 6, 3, 1, F))
        many = list(bench.stage_compact(cfg, first_gid, groups, 6, 3, 3, F))
        assert len(one) == len(many) == 3
        for (a, sa), (b, sb) in zip(one, many):
            assert (a.rounds, a.count, a.entry_count) == (b.rounds, b.count, b.entry_count) == (6, groups, 0)
            assert np.array_equal(a.head, b.head) and np.array_equal(a.abcd, b.abcd)
            assert sa == sb and sa[0] > 0
