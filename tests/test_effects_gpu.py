"""rg_effects32 on an MI355X: the log writes, the commit advances and the RG_NEED_HOST cells of a launch's compact outcome rows as three lists. The layout bit for
bit against the numpy model of the header's contract in both memspaces; real decisions through rg_submit32c, rg_submit32c_sparse_rounds and a sparse-rounds tick
with the call queued behind rg_tick2_launch, where the lists alone must give what a walk over every row finds. The case functions live in
tests/effects_cases.py (the host emulation runs them at the smallest sizes: tests/test_effects_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import effects_cases as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", [False, True], ids=["host-memory", "device-memory"])
@pytest.mark.parametrize("Cc,D,seed", [(1000, 4, 5), (4096, 17, 8), (65600, 1, 6), (262208, 2, 9)])
def test_the_lists_equal_the_model(Cc, D, seed, device):
    """(1000, 4): a row count off a multiple of 64. (4096, 17): 1088 wavefronts of cells, so that the prefix sum's second level runs. (65600, 1): 1025 wavefronts
    in one round, of cells and of rows. (262208, 2): more than 4096 x 64 cells and rows, the size from which a wavefront covers 128 of them (rg_effects.hpp:
    effects_span). Fills 0 .. 100 %, n and R through the device words and without them, gid NULL and a list, capacities of 0, below and above the counts, every
    call twice with identical bytes. Sentinel bytes and marked rows prove every NOT TOUCHED / not read clause."""
    assert E.layout_case(Cc, D, seed, device=device) == 18


@pytest.mark.parametrize("route", ["dense", "sparse", "tick"])
@pytest.mark.parametrize("G,P,seed,launches", [(1024, 5, 1, 50), (1024, 3, 9, 50)])
def test_the_lists_give_what_the_full_walk_finds(G, P, seed, launches, route):
    """1024 groups x 8 rounds at most, the sparse-rounds fuzz stream. The run has seen a truncation, a group committing in more than one round of a launch and an
    RG_NEED_HOST cell: the seeds are those that give one on every route (on the host emulation: 3 cells through the two submits and 2 through the tick, whose
    send step makes its stream another, for seed 1 at 5 nodes; 3 and 6 for seed 9 at 3 nodes)."""
    truncs, multi, need = E.decisions_case(G, P, seed, launches, route)
    assert truncs > 0 and multi > 0 and need > 0, (truncs, multi, need)


def test_the_lists_behind_a_device_resident_tick():
    truncs, multi, need = E.decisions_case(1024, 5, 1, 50, "tick", device_resident=True)
    assert truncs > 0 and multi > 0 and need > 0, (truncs, multi, need)


def test_the_lists_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    truncs, multi, need = E.decisions_case(1024, 5, 1, 50, "sparse")
    assert truncs > 0 and multi > 0 and need > 0, (truncs, multi, need)


def test_effects32_refuses_what_the_header_says():
    E.refusals_case()


def test_a_pageable_pointer_is_refused_in_the_device_memspace():
    """(the emulation cannot tell pageable from page-locked memory: this refusal is checked here) — and nothing was launched: the next call is the model's"""
    G = 512
    t = engine.Table(G, 3)
    e, o, cols = E.refusal_structs(G)
    rc = engine.lib().rg_effects32(t._h, C.byref(e), C.byref(o), abi.MEM_DEVICE)
    assert rc == -1 and b"neither device memory" in engine.lib().rg_last_error(t._h)
    row = E.synthetic(np.random.default_rng(3), G, 4, 400, 3, 0.2)
    E.check_effects(E.effects_device(t, row, G, 4, count=400, rounds=3), E.model(G, 4, 400, 3, None, row), "after a refusal")
    t.close()
