"""rg_assemble32 — arrival-ordered events into sparse-round batches on the device — without a GPU: the product's kernels and C-ABI host code on the host
emulation (tests/devemu/emu_cases_assemble.py, driven the way tests/test_sparse_rounds_cpu.py drives its cases). Wavefront mode: the cases of
tests/test_assemble_gpu.py at small table sizes; lane-serial mode: the refusals, which happen on the host before any launch. The numpy model the layout is
held against is checked here on a hand-made input, without any library."""
import os
import subprocess
import sys

import numpy as np

from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_assemble.py")


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_assembling_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)


def test_assemble32_refuses_misuse_before_any_launch(emulation_library):  # noqa: F811
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="0", RG_EMU_WAVES="0"), ["-k", "refuses"])


def test_the_model_on_a_hand_made_log():
    """8 groups, 2 rows, 2 rounds: fired tickets first, a bad gid, a group beyond the list, a third event of a listed group"""
    from rafting_amd import abi
    from tests import assemble_cases as A
    gid = np.array([5, 2, 9, 2, 7, 2, 5], np.uint32)
    head = np.zeros(7, abi.HEAD_DT)
    head["hdr"], head["aux"] = 100 + np.arange(7), 200 + np.arange(7)
    abcd = np.zeros(7, abi.QUAD32_DT)
    abcd["a"] = 300 + np.arange(7)
    w = A.model(8, gid, head, abcd, capacity=2, max_rounds=2, expired=(np.array([5, 6], np.uint32), np.array([41, 42], np.uint32), 2))
    assert (w.n, w.R) == (2, 2) and list(w.gid) == [2, 5]
    assert w.origin.tolist() == [[1, 0x80000000], [3, 0]]
    assert w.head["hdr"].tolist() == [[101, A.TIMEOUT_HDR], [103, 100]] and w.head["aux"].tolist() == [[201, 41], [203, 200]]
    assert w.abcd["a"].tolist() == [[301, 0], [303, 300]]
    assert w.deferred.tolist() == [0x80000001, 4, 5, 6] and w.stats.tolist() == [4, 4, 1, 0]
    empty = A.model(8, gid[:0], head[:0], abcd[:0], capacity=2, max_rounds=2)
    assert (empty.n, empty.R) == (0, 1) and empty.stats.tolist() == [0, 0, 0, 0]
