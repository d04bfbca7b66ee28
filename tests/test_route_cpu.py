"""rg_route32 — a decided batch back in arrival order and as lists, on the device — without a GPU: the product's kernels and C-ABI host code on the host
emulation (tests/devemu/emu_cases_route.py, driven the way tests/test_assemble_cpu.py drives its cases). Wavefront mode: the cases of tests/test_route_gpu.py at
small table sizes; lane-serial mode: the refusals, which happen on the host before any launch. The numpy model the layout is held against is checked here on a
hand-made input, without any library."""
import os
import subprocess
import sys

import numpy as np

from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_route.py")


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_routing_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)


def test_route32_refuses_misuse_before_any_launch(emulation_library):  # noqa: F811
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="0", RG_EMU_WAVES="0"), ["-k", "refuses"])


def test_the_route_model_on_a_hand_made_log():
    """the 8-group log of tests/test_assemble_cpu.py (2 rows, 2 rounds: gids [2, 5], origin [[1, 0x80000000], [3, 0]], m = 7, e = 2), made-up rows: cell 0 converts
    and sends to follower 0, cell 2 (capacity 2: round 1, row 0) needs the host, cell 3 converts; row 1 sends to both followers"""
    from rafting_amd import abi
    from tests import assemble_cases as A
    from tests import route_cases as R
    gid = np.array([5, 2, 9, 2, 7, 2, 5], np.uint32)
    head, abcd = np.zeros(7, abi.HEAD_DT), np.zeros(7, abi.QUAD32_DT)
    a = A.model(8, gid, head, abcd, capacity=2, max_rounds=2, expired=(np.array([5, 6], np.uint32), np.array([41, 42], np.uint32), 2))
    assert a.origin.tolist() == [[1, 0x80000000], [3, 0]]
    row, per, send = np.zeros(4, abi.OUT32_DT), np.zeros(4, abi.PERSIST32_DT), np.zeros(4, abi.SEND_DT)
    row["commit_index"], per["term"] = [0, 1, 2, 3], [70, 71, 72, 73]
    row["flags"] = [abi.F_PERSIST, 0, abi.NEED_HOST << abi.F_STATUS_SHIFT, abi.F_PERSIST | abi.F_REPLIED]
    send["kind"] = [abi.SEND_APPEND, abi.SEND_NEED_HOST, abi.SEND_GATED, abi.SEND_SNAPSHOT]        # [follower][row]
    w = R.model(2, 2, a.n, a.R, 7, 2, a.gid, a.origin.reshape(-1), row, per, send, 2)
    NONE = 0xFFFFFFFF
    assert w.cell.tolist() == [3, 0, NONE, 2, NONE, NONE, NONE] and w.expired_cell.tolist() == [1, NONE]
    assert w.row["commit_index"][[0, 1, 3]].tolist() == [3, 0, 2] and w.expired_row["commit_index"][0] == 1
    assert w.has_persist.tolist() == [True, True, False, False, False, False, False] and w.persist32["term"][:2].tolist() == [73, 70]
    assert not w.expired_has_persist.any()
    assert w.persist_list.tolist() == [(0, 2), (3, 5)] and w.attention.tolist() == [(2, 2)]
    assert w.send_list.tolist() == [(0, 2), (1, 5), (1, 5)] and w.send_offset.tolist() == [0, 2, 3]
