"""rg_route32 on an MI355X: what a launch left over an assembled batch, back in arrival order and as the persist, attention and send lists. The layout bit for
bit against the numpy model of the header's contract in both memspaces; the decisions in lockstep with the oracle through rg_assemble32 -> rg_tick2_launch ->
rg_route32, all RG_MEM_DEVICE, with no host step between the three. The case functions live in tests/route_cases.py (the host emulation runs them at small sizes:
tests/test_route_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests import assemble_cases as A
from tests import route_cases as R
from tests.test_sparse_rounds_gpu import TICKS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", [False, True], ids=["host-memory", "device-memory"])
@pytest.mark.parametrize("G,seed", [(1000, 5), (4096, 8), (65600, 6)])
def test_the_routed_layout_equals_the_model(G, seed, device):
    """the inputs of the assembler's layout check (fills 0 .. 100 %, both overflows, bad gids, e = 0, the 0xFFFFFFFF mark, a fired list longer than its columns),
    synthetic rows that carry their cell index, every input routed twice; list capacities of 0, below and above the counts; group counts off a multiple of 64 and
    more than 1024 wavefronts of cells, so that the prefix sum's second level runs. Sentinel bytes prove every NOT TOUCHED clause."""
    assert R.layout_case(G, seed, device=device) > 20


@pytest.mark.parametrize("resident", [False, True], ids=["host-pinned", "device-resident"])
@pytest.mark.parametrize("G,P,seed,ticks", sorted(TICKS)[:3])
def test_routed_ticks_in_lockstep_with_the_oracle(G, P, seed, ticks, resident):
    R.routed_tick_case(G, seed, ticks, P=P, device_resident=resident)


def test_routed_ticks_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    R.routed_tick_case(1024, 5, 25)


def test_routed_ticks_with_device_resident_in_flight_counts():
    assert R.in_flight_case() > 0


def test_route32_refuses_what_the_header_says():
    R.refusals_case()


def test_a_pageable_pointer_is_refused_in_the_device_memspace():
    """(the emulation cannot tell pageable from page-locked memory: this refusal is checked here) — and nothing was launched: the next route is the model's"""
    G = 256
    t = engine.Table(G, 3)
    asm = engine.Assembler(t, 16, max_expired=4)
    kw = dict(gid=np.arange(16, dtype=np.uint32) * 7, head=np.zeros(16, abi.HEAD_DT), abcd=np.zeros(16, abi.QUAD32_DT), capacity=G, max_rounds=4,
              expired=(np.array([3, 40, 41, 50], np.uint32), np.arange(4, dtype=np.uint32) + 1, 4))
    got = A.assemble_device(asm, **kw)
    d, r, cols = R.refusal_structs(G)
    rc = engine.lib().rg_route32(asm._h, C.byref(d), C.byref(r), abi.MEM_DEVICE)
    assert rc == -1 and b"neither device memory" in engine.lib().rg_last_error(t._h)
    row, per, send = R.synthetic(np.random.default_rng(3), G, 4, got.n, got.R, 2)
    out = R.route_device(asm, got.gid, got.n, got.R, got.origin, row, per, G, 4, 16, expired_capacity=4, send=send)
    R.check_routed(out, R.model(G, 4, got.n, got.R, 16, 4, got.gid, got.origin, row, per, send, 2), 16, 4, "after a refusal")
    asm.close()
    t.close()
