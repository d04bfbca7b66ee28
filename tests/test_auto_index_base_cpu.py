"""RG_OPT_AUTO_INDEX_BASE without a GPU: the two host-side helpers (rg_index_base_advance / rg_index_base_advance32) against a numpy restatement of the
rule, their misuse answers, and the device code on the host emulation (tests/devemu/emu_cases_auto_base.py: the compact-row kernel's 32-bit body
carrying groups past four windows of 2^30 with no workgroup on the 64-bit body)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rafting_amd import abi, engine
from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)


def rule(base, gids, a_abs, window):
    """the rule, restated: every LOG_FLUSH row raises its group's base to max(base, a - W); a = 0 moves nothing (a - W <= 0 <= base)"""
    out = base.copy()
    for g, a in zip(gids, a_abs):
        out[g] = max(out[g], a - window)
    return out


def random_batch(rng, G, rounds, sparse, base, window):
    """a batch with LOG_FLUSH rows among other kinds: relative a from 0 (none) over a - W <= base up to far beyond the window"""
    count = G if not sparse else G // 3
    gid = np.sort(rng.choice(G, count, replace=False)).astype(np.uint32) if sparse else None
    b = abi.Batch(rounds, count, gid=gid)
    kinds = rng.choice([abi.EV_NONE, abi.EV_LOG_FLUSH, abi.EV_TIMEOUT, abi.EV_AE_ACK, abi.EV_CLIENT_APPEND], size=rounds * count, p=[0.2, 0.4, 0.1, 0.2, 0.1])
    b.head["hdr"] = kinds.astype(np.uint32)
    rel = rng.choice([0, 1, window - 1, window, window + 1, 3 * window, (1 << 31) - 1], size=rounds * count).astype(np.int64)
    rel = np.where(rng.random(rounds * count) < 0.5, rng.integers(0, 1 << 31, rounds * count), rel)
    g_of_row = np.tile(np.arange(count) if gid is None else gid.astype(np.int64), rounds)
    b.ab["x"] = np.where(rel == 0, 0, rel + base[g_of_row])          # absolute a
    b.ab["y"] = rng.integers(1, 9, rounds * count)
    b.cd["x"] = rng.integers(0, 1 << 40, rounds * count)             # (other kinds' fields: never read by the rule)
    return b, rel, g_of_row


def compact_of(b, rel):
    """the same rows as an abi.Batch32 whose a is relative (what a host packed against `base`)"""
    rows = b.rounds * b.count
    abcd = np.zeros(rows, dtype=abi.QUAD32_DT)
    abcd["a"] = rel.astype(np.int32)
    abcd["b"] = b.ab["y"].astype(np.int32)
    return abi.Batch32(b.rounds, b.count, b.gid, b.head.copy(), abcd, np.zeros(1, np.int32), 0)


@pytest.mark.parametrize("rounds,sparse,seed", [(1, False, 1), (1, True, 2), (6, False, 3), (64, False, 4)])
def test_helpers_apply_the_rule_like_numpy(rounds, sparse, seed):
    rng = np.random.default_rng(seed)
    G, W = 96, 1 << 28
    base = np.where(rng.random(G) < 0.3, 0, rng.integers(1, 1 << 45, G)).astype(np.int64)
    b, rel, g_of_row = random_batch(rng, G, rounds, sparse, base, W)
    flush = (b.head["hdr"] & 0xF) == abi.EV_LOG_FLUSH
    want = rule(base, g_of_row[flush], b.ab["x"][flush].astype(np.int64), W)
    assert np.any(want != base) and np.any(rel[flush] == 0) and np.any((rel[flush] > 0) & (rel[flush] <= W))      # moves, and rows that move nothing
    wide = base.copy()
    engine.advance_index_base(b, wide, W)
    assert np.array_equal(wide, want)
    comp = base.copy()
    engine.advance_index_base(compact_of(b, rel), comp, W)                      # relative a: against the array as it was on entry
    assert np.array_equal(comp, want)
    again = want.copy()                                                          # max is idempotent: the same rows once more move nothing
    engine.advance_index_base(b, again, W)
    assert np.array_equal(again, want)


def test_a_base_is_never_lowered_and_the_window_is_what_the_rule_keeps_below_the_flush():
    base = np.array([0, 1000, 5 << 30], dtype=np.int64)
    b = abi.Batch(1, 3)
    b.head["hdr"] = abi.hdr_make(abi.EV_LOG_FLUSH)
    b.ab["x"] = [(1 << 30) + 7, 1000 + 100, 4 << 30]
    engine.advance_index_base(b, base, 100)
    assert base.tolist() == [(1 << 30) + 7 - 100, 1000, 5 << 30]


def test_helpers_refuse_misuse():
    L = engine.lib()
    G = 4
    b = abi.Batch(1, G)
    b.head["hdr"] = abi.hdr_make(abi.EV_LOG_FLUSH)
    base = np.zeros(G, dtype=np.int64)
    for w in (0, -1, 1 << 30, (1 << 31) - 1):
        with pytest.raises(engine.EngineError, match="window"):
            engine.advance_index_base(b, base, w)
    cb = b.as_struct()
    import ctypes as C
    assert L.rg_index_base_advance(None, 16, G, base.ctypes.data) == -1
    assert L.rg_index_base_advance(C.byref(cb), 16, G, None) == -1
    no_ab = b.as_struct()
    no_ab.ab = None
    assert L.rg_index_base_advance(C.byref(no_ab), 16, G, base.ctypes.data) == -1
    no_head = b.as_struct()
    no_head.head = None
    assert L.rg_index_base_advance(C.byref(no_head), 16, G, base.ctypes.data) == -1
    b32 = compact_of(b, np.zeros(G, np.int64))
    c32 = b32.as_struct()
    c32.abcd = None
    assert L.rg_index_base_advance32(C.byref(c32), 16, G, base.ctypes.data) == -1
    assert L.rg_index_base_advance(C.byref(cb), 16, G + 1, base.ctypes.data) == -2      # dense: one row per group
    sp = abi.Batch(1, 2, gid=np.array([1, 9], dtype=np.uint32))
    assert L.rg_index_base_advance(C.byref(sp.as_struct()), 16, G, base.ctypes.data) == -2      # a gid beyond the groups
    with pytest.raises(engine.EngineError, match="int64"):
        engine.advance_index_base(b, [0, 0, 0, 0], 16)
    assert abi.OPT_AUTO_INDEX_BASE == 2 and abi.ABI_VERSION == 6


def test_automatic_bases_on_the_emulated_wavefronts(emulation_library):  # noqa: F811
    env = dict(os.environ, RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1", RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT)
    env.pop("RG_FAST", None)
    env.pop("RG_FORCE_WIDE", None)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(EMU, "emu_cases_auto_base.py"), "-x", "-q", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert "2 passed" in p.stdout and "failed" not in p.stdout
