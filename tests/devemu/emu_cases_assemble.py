"""Cases for rg_assemble32 on the host emulation of the kernels. Run by tests/test_assemble_cpu.py in a subprocess; TEST INFRASTRUCTURE. The device cases need
the WAVEFRONT mode (RG_EMU_WAVES=1, RG_SPLIT=1: ballots, shuffles and barriers meet); the refusals happen on the host before any launch and run in either mode
(`-k refuses`). The cases are those of tests/test_assemble_gpu.py at small table sizes (tests/assemble_cases.py)."""
import os

import pytest

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
WAVES = os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from tests import assemble_cases as A  # noqa: E402

device = pytest.mark.skipif(not WAVES, reason="the kernels need the wavefront mode of the emulation")


@device
@pytest.mark.parametrize("G,seed", [(200, 3), (64, 4), (1000, 5), (4097, 6)])
def test_the_layout_equals_the_model(G, seed):
    """group counts on and off a multiple of 64; every input twice on one assembler (host memory)"""
    assert A.layout_case(G, seed) > 20


@device
def test_the_layout_equals_the_model_in_device_memory():
    assert A.layout_case(300, 7, device=True) > 20


@device
@pytest.mark.parametrize("G,P,seed,resident", [(192, 3, 11, False), (256, 5, 321, True), (192, 7, 16, False)])
def test_assembled_ticks_in_lockstep_with_the_oracle(G, P, seed, resident):
    A.assembled_tick_case(G, seed, 25, P=P, device_resident=resident)


@device
def test_assembled_ticks_on_the_64_bit_body(monkeypatch):
    monkeypatch.setenv("RG_FORCE_WIDE", "1")
    A.assembled_tick_case(128, 5, 25)


@device
@pytest.mark.parametrize("G,launches,seed,least", [(128, 8, 31, 16), (1024, 12, 41, 1024)])
def test_assembled_ticks_with_automatic_index_bases(G, launches, seed, least):
    """(the second case is the GPU test's: enough groups and launches for a group to be wiped several times in a row)"""
    flushes, moved = A.auto_base_case(G, launches, seed)
    assert flushes > least and moved > 0


@device
def test_the_assembled_columns_through_the_stand_alone_call():
    assert A.standalone_case(192, 5, 9, 12) > 0


def test_assemble32_refuses_what_the_header_says():
    A.refusals_case()
