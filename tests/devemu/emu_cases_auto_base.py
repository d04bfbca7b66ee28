"""Cases for RG_OPT_AUTO_INDEX_BASE on the WAVEFRONT mode of the host emulation (RG_EMU_WAVES=1, RG_SPLIT=1: the two-wavefront kernels with their
LDS hand-over, the 32-bit body of the compact-row kernel included). Run by tests/test_auto_index_base_cpu.py in a subprocess; TEST INFRASTRUCTURE.
Two-round launches (this mode cannot run multi-round launches with lanes blocked after a NEED_HOST: the stream has none)."""
import os

import numpy as np

assert os.environ.get("RG_LIB", "").endswith("libraftgpu_emu.so"), "these cases are for the host emulation library only"
assert os.environ.get("RG_EMU_WAVES") == "1" and os.environ.get("RG_SPLIT") == "1"

from rafting_amd import abi, engine  # noqa: E402
from tests import auto_base_stream as S  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests.helpers import compare_outcomes, compare_states  # noqa: E402


def test_groups_carried_past_four_windows_of_2_30_stay_on_the_32_bit_body():
    """W = 2^28 on compact rows in, compact outcome rows out (rg_submit32c): every launch is packed against the host's mirror of the bases (advanced by
    rg_index_base_advance32 from the very rows it sends), decided like the oracle decides the absolute stream, leaves the table's bases equal to the
    mirror, and keeps every workgroup on the 32-bit body — until every group's epoch has moved more than 4 x 2^30 past its start."""
    G, P, self_slot = 64, 5, 1
    st0, base = S.start_state(G, P, self_slot, seed=31)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    gpu.set_index_base(base)
    gpu.set_auto_index_base(S.WINDOW)
    gpu.load_state(st0)
    orc.load_state(st0)
    gpu.wide_body_workgroups(reset=True)
    rng = np.random.default_rng(31)
    mirror = base.copy()
    launches = flushes = 0
    while np.min(orc.read_state().epoch_index - st0.epoch_index) <= 4 << 30:
        assert launches < 400, "the stream stopped carrying the groups forward"
        b, ref, cur = S.launch(orc, rng, P, self_slot)
        b32 = engine.pack32(b, index_base=mirror)
        raw = gpu.submit32c(b32, fill=0xAB)
        got, _ = engine.unpack32(raw, b.rounds, G, cur.role_epoch, index_base=mirror)      # (the rows speak the bases the launch started with)
        compare_outcomes(ref, got, "automatic bases, launch %d" % launches)
        want = S.advance(b, mirror)
        engine.advance_index_base(b32, mirror, S.WINDOW)
        assert np.array_equal(mirror, want)
        assert np.array_equal(gpu.index_base(), mirror), "launch %d" % launches
        assert gpu.wide_body_workgroups() == 0, "launch %d" % launches
        flushes += int(np.count_nonzero((b.head["hdr"] & 0xF) == abi.EV_LOG_FLUSH))
        launches += 1
    compare_states(orc.read_state(), gpu.read_state(), "automatic bases final")
    assert np.all(mirror - base > 3 << 30) and flushes > 5 * G
    gpu.close()
    orc.close()


def test_wide_rows_move_the_bases_by_the_same_rule():
    """the same stream as wide rows (rg_submit: the two-wavefront wide-row kernel, absolute a): bases equal the mirror of rg_index_base_advance"""
    G, P, self_slot = 64, 3, 0
    st0, base = S.start_state(G, P, self_slot, seed=32)
    gpu, orc = engine.Table(G, P, self_slot, True), oracle_lib.OracleTable(G, P, self_slot, True)
    gpu.set_index_base(base)
    gpu.set_auto_index_base(S.WINDOW)
    gpu.load_state(st0)
    orc.load_state(st0)
    rng = np.random.default_rng(32)
    mirror = base.copy()
    for k in range(12):
        b, ref, _ = S.launch(orc, rng, P, self_slot)
        compare_outcomes(ref, gpu.submit(b, fill=0xAB), "wide rows, launch %d" % k)
        engine.advance_index_base(b, mirror, S.WINDOW)
        assert np.array_equal(gpu.index_base(), mirror), "launch %d" % k
    assert np.any(mirror != base)
    compare_states(orc.read_state(), gpu.read_state(), "wide rows final")
    gpu.close()
    orc.close()
