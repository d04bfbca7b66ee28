"""The carry of an assembler on an MI355X: deferred events kept on the device, taken first by the next run, and routed by rg_route32_carry. Chains of runs on one
assembler against the numpy models of the header's contract — today's contract with the deferred rows prepended by hand —, bit for bit, in both memspaces. The
case functions live in tests/carry_cases.py (the host emulation runs them at small sizes: tests/test_carry_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import assemble_cases as A
from tests import carry_cases as K
from tests import route_cases as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", [False, True], ids=["host-memory", "device-memory"])
@pytest.mark.parametrize("G,seed", [(130, 3), (1000, 5), (4096, 8)])
def test_a_chain_of_carrying_runs_equals_the_model(G, seed, device):
    """both overflows, a segment for the radix select whose surplus is carried, tickets of groups beyond the list carried as rows, an untrusted fired list, bad
    gids, an event carried three runs in a row, a drain as long as the model's; carries that are ample, exactly full, one slot short and of one slot; the chain
    again after a reset; the carry switched off. Every run: the batch, both carries, the routed columns with their four kinds of cell entry, sentinel bytes
    wherever nothing is to be written, the lists equal to plain rg_route32's."""
    assert K.chain_case(G, seed, device=device) >= 24


def test_a_large_chain_equals_the_model():
    assert K.large_case(G=65600, events=1 << 17, runs=3) > 1 << 17


@pytest.mark.parametrize("G,P,seed", [(1000, 3, 21), (4096, 5, 21)])
def test_carried_ticks_equal_ticks_fed_by_hand(G, P, seed):
    """rg_assemble32 -> rg_tick2_launch -> rg_route32_carry queued with nothing between them on a device-resident tick, 25 ticks, against today's path fed by hand
    through deferred[] and against the oracle; every arrival's answer followed through the chain of routed columns"""
    deferred, resync = K.pipeline_case(G, P, seed, 25)
    assert deferred > 12 and resync * 4 <= 25


def test_the_carry_refuses_what_the_header_says():
    K.refusals_case(huge=False)


def test_a_pageable_pointer_is_refused_in_the_device_memspace():
    """(the emulation cannot tell pageable from page-locked memory: this refusal is checked here) — and nothing was launched: the carry is what the run left"""
    G = 256
    t = engine.Table(G, 3)
    asm = engine.Assembler(t, 16, max_expired=4, carry=8)
    a, b, cols = A.refusal_structs(G, D=1)
    cols["gid"][:] = 5                                                  # (16 events of one group at depth 1: 15 deferred, 8 carried, 7 spilled)
    assert engine.lib().rg_assemble32(asm._h, C.byref(a), C.byref(b), abi.MEM_HOST) == 0 and cols["o_stats"].tolist() == [5, 15, 0, 7]
    before = asm.carry_read(abi.CARRY_NEXT)
    assert len(before[0]) == 8
    d, r, keep = R.refusal_structs(G, D=1)
    c, keep_c = K.carried_struct(8)
    rc = engine.lib().rg_route32_carry(asm._h, C.byref(d), C.byref(r), C.byref(c), abi.MEM_DEVICE)
    assert rc == -1 and b"neither device memory" in engine.lib().rg_last_error(t._h)
    for x, y in zip(before, asm.carry_read(abi.CARRY_NEXT)):
        assert np.array_equal(x, y)
    asm.close()
    t.close()
