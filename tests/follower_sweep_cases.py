"""Cases that reach every kernel family at EVERY cluster size, 2 .. 15 nodes (1 .. 14 followers): the launchers pick a kernel instantiation by the follower
count, and a dispatch that reached the wrong one — or none — at a size no other test runs (10, 12, 13 and 14 nodes on the compact and tick paths) would go
unseen. Shared by tests/test_follower_sweep_gpu.py (an MI355X) and tests/devemu/emu_cases_follower_sweep.py (the host emulation of the kernels).

Built from case functions that exist, inside compact_large_cluster_cases.routed(...), i.e. with RG_OPT_COMPACT_ANY_CLUSTER — which changes nothing at 7 nodes
and below (option_small_cluster_case). 130 groups everywhere: two full workgroups and a ragged one, the smallest table that has both on every kernel.
Everything is held bit-exactly against tests/oracle_lib.OracleTable by the cases themselves."""
from tests import compact_large_cluster_cases as K
from tests import sparse_rounds_cases as X
from tests import sparse_tick_cases as S
from tests import test_gpu_parity as T

CLUSTERS = tuple(range(2, 16))
ROUTES = K.ROUTES
RECORDINGS = (None, 2, 4)                                     # RG_TICK_NODES: tick_kernel; step + tick_tail_kernel; the step-by-step form with replicate_kernel
G, ROUNDS = 130, 24


def step_case(P, route):
    """step32_kernel / step32_wide_kernel, dense, wide and compact outcome rows: a lockstep fuzz through one compact route. Rows that answer RG_NEED_HOST are
    repaired as hinted WIDE rows — not decided by the kernels under test — hence the project's 2 % cap on them (compact_large_cluster_cases.lockstep_case)."""
    with K.routed(route):
        _, _, _, _, misses, gpu = T._lockstep(G, P, 1 % P, True, ROUNDS, 800 + P, allow_miss=False)
        rows = G * ROUNDS
        print("step %s cluster %d: %d of %d rows repaired through the hint protocol" % (route, P, misses, rows))
        assert misses * 50 <= rows, "%d of %d rows were repaired as wide rows (cap: 2 %%)" % (misses, rows)
        gpu.close()


def wide_step_case(P):
    """the same lockstep on wide rows — step_kernel or step_split_kernel, as RG_SPLIT says when the table is created; every row is compared after the hint
    repair, no cap"""
    with K.routed(None):
        _, _, _, _, _, gpu = T._lockstep(G, P, 1 % P, True, ROUNDS, 800 + P, allow_miss=False)
        gpu.close()


def dense_tick_case(P, nodes):
    """one recording of the dense device-resident tick, every tick held to the oracle (tick2_case asserts that tickets fired and appends were sent)"""
    with K.routed(None):
        T.tick2_case(G=G, P=P, ticks=16, seed=820 + P, nodes=nodes)


def sparse_tick_case(P):
    """tick_sparse_kernel at depth 1 and tick_expire_kernel"""
    with K.routed(None):
        S.sparse_tick_case(G, 840 + P, 20, P=P, expect_all=False)


def rounds_tick_case(P):
    """tick_sparse_kernel at run-time depths and tick_expire_kernel"""
    with K.routed(None):
        X.rounds_tick_case(G, 860 + P, 20, P=P, expect_all=False)
