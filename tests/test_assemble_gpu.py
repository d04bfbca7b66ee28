"""rg_assemble32 on an MI355X: arrival-ordered events, and the tickets a tick listed, into the columns of a sparse-rounds batch. The layout bit for bit against
the numpy model of the header's contract, up to 1 048 576 groups with 2^20 events, in both memspaces; the decisions in lockstep with the oracle through
rg_assemble32(RG_MEM_DEVICE) -> rg_tick2_launch with no host step between them. The case functions live in tests/assemble_cases.py (the host emulation runs
them at small sizes: tests/test_assemble_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import assemble_cases as A
from tests.test_sparse_rounds_gpu import TICKS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", [False, True], ids=["host-memory", "device-memory"])
@pytest.mark.parametrize("G,seed,events", [(1000, 5, None), (4096, 8, None), (65600, 6, None), (1 << 20, 7, 1 << 20)])
def test_the_layout_equals_the_model(G, seed, events, device):
    """random logs at fills 0 .. 100 % with repeats, no events with and without fired tickets, depth and capacity overflow (one and both, a short deferred list),
    gids at and above the group count, group counts off a multiple of 64, a fired list longer than its columns and one marked 0xFFFFFFFF; every input twice on
    the same assembler. Sentinel bytes show that rows >= n and rounds >= R were not touched."""
    assert A.layout_case(G, seed, device=device, events=events) > 20


@pytest.mark.parametrize("resident", [False, True], ids=["host-pinned", "device-resident"])
@pytest.mark.parametrize("G,P,seed,ticks", TICKS)
def test_assembled_ticks_in_lockstep_with_the_oracle(G, P, seed, ticks, resident):
    A.assembled_tick_case(G, seed, ticks, P=P, device_resident=resident)


def test_assembled_ticks_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    A.assembled_tick_case(1024, 5, 25)


def test_assembled_ticks_with_automatic_index_bases():
    flushes, moved = A.auto_base_case(1024, 12, 41)
    assert flushes > 1024 and moved > 1024 // 4


@pytest.mark.parametrize("G,P,seed", [(4096, 5, 321), (1000, 3, 77)])
def test_the_assembled_columns_through_the_stand_alone_call(G, P, seed):
    assert A.standalone_case(G, P, seed, 20) > 0


def test_assemble32_refuses_what_the_header_says():
    A.refusals_case()


def test_a_pageable_pointer_is_refused_in_the_device_memspace():
    """(the emulation cannot tell pageable from page-locked memory: this refusal is checked here) — and nothing was launched: the next run is the model's"""
    G = 256
    t = engine.Table(G, 3)
    asm = engine.Assembler(t, 16, max_expired=4)
    a, b, cols = A.refusal_structs(G)
    rc = engine.lib().rg_assemble32(asm._h, C.byref(a), C.byref(b), abi.MEM_DEVICE)
    assert rc == -1 and b"neither device memory" in engine.lib().rg_last_error(t._h)
    kw = dict(gid=np.array([9, 3, 9, 300, 1], np.uint32), head=np.zeros(5, abi.HEAD_DT), abcd=np.zeros(5, abi.QUAD32_DT), capacity=G, max_rounds=2)
    A.check_layout(A.assemble_device(asm, **kw), A.model(G, **kw), G, 2, "after a refusal")
    asm.close()
    t.close()
