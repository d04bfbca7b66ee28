"""rg_effects32 — a launch's log writes, commit advances and RG_NEED_HOST cells as lists, on the device — without a GPU: the product's kernels and C-ABI host code
on the host emulation (tests/devemu/emu_cases_effects.py, driven the way tests/test_route_cpu.py drives its cases). Wavefront mode: the cases of
tests/test_effects_gpu.py at the smallest sizes; lane-serial mode: the refusals, which happen on the host before any launch. The numpy model the layout is held
against is checked here on a hand-made input, without any library."""
import os
import subprocess
import sys

import numpy as np

from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_effects.py")


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_effects_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)


def test_effects32_refuses_misuse_before_any_launch(emulation_library):  # noqa: F811
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="0", RG_EMU_WAVES="0"), ["-k", "refuses"])


def test_the_binding_names_the_entry_point_and_its_structs():
    """(no library: the layout of the two structs and of a commit item as include/raftgpu.h declares them, on an LP64 host)"""
    import ctypes as C
    from rafting_amd import abi, engine
    assert "rg_effects32" in engine.exported_symbols()
    assert abi.COMMIT_ITEM_DT.names == ("cell", "gid", "commit_index", "flags") and abi.COMMIT_ITEM_DT.itemsize == 16
    assert C.sizeof(abi.CEffectsIn) == 40 and abi.CEffectsIn.row.offset == 32
    assert C.sizeof(abi.CEffects) == 56 and abi.CEffects.counts.offset == 48 and abi.CEffects.attention_capacity.offset == 40


def test_the_effects_model_on_a_hand_made_batch():
    """2 rows x 2 rounds, gids [3, 6]. Group 3 appends in round 0 and commits in rounds 0 AND 1: one commit item, at the round-1 cell. Group 6 truncates and
    appends in round 0 and commits there with RG_F_WIDE_VALUES (its flags arrive verbatim), and needs the host in round 1"""
    from rafting_amd import abi
    from tests import effects_cases as E
    need = abi.NEED_HOST << abi.F_STATUS_SHIFT
    row = np.zeros(4, abi.OUT32_DT)
    row["commit_index"], row["log_from"] = [10, 20, 11, 21], [5, 6, 7, 8]
    wide_commit = abi.F_LOG_TRUNC | abi.F_LOG_APPEND | abi.F_COMMIT | abi.F_WIDE_VALUES | abi.F_REPLIED
    row["flags"] = [abi.F_LOG_APPEND | abi.F_COMMIT, wide_commit, abi.F_COMMIT | abi.F_SUCCESS, need]      # cells 0, 1 (round 0), 2, 3 (round 1)
    gid = np.array([3, 6], np.uint32)
    w = E.model(2, 2, 2, 2, gid, row)
    assert w.log_list.tolist() == [(0, 3), (1, 6)] and w.attention.tolist() == [(3, 6)]
    assert w.commit_list.tolist() == [(2, 3, 11, abi.F_COMMIT | abi.F_SUCCESS), (1, 6, 20, wide_commit)]
    # one round only: group 3's commit is the round-0 one, nothing needs the host; one row only: group 6 is not read; no gid list: row i is group i
    w = E.model(2, 2, 2, 1, gid, row)
    assert w.commit_list.tolist() == [(0, 3, 10, abi.F_LOG_APPEND | abi.F_COMMIT), (1, 6, 20, wide_commit)] and len(w.attention) == 0
    w = E.model(2, 2, 1, 2, None, row)
    assert w.log_list.tolist() == [(0, 0)] and w.commit_list.tolist() == [(2, 0, 11, abi.F_COMMIT | abi.F_SUCCESS)] and len(w.attention) == 0
    # ... and the two readers agree on it: the lists alone give what a walk over every row finds
    fx = __import__("types").SimpleNamespace(log_list=w.log_list, commit_list=w.commit_list, attention=w.attention, counts=np.array([1, 1, 0, 0], np.uint32),
                                             log_capacity=4, commit_capacity=2, attention_capacity=4)
    assert E.from_lists(fx, row, 2) == ([(0, 0, False, True, 5)], {0: 11}, [])
