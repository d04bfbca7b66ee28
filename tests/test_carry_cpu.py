"""The carry of an assembler — deferred events taken into the next run on the device — without a GPU: the product's kernels and C-ABI host code on the host
emulation (tests/devemu/emu_cases_carry.py, driven the way tests/test_route_cpu.py drives its cases). Wavefront mode: the cases of tests/test_carry_gpu.py at
small table sizes; lane-serial mode: the refusals, which happen on the host before any launch. The numpy models the device is held against are pinned here on a
hand-made chain, without any library."""
import os
import subprocess
import sys

import numpy as np

from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_carry.py")


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_carrying_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)


def test_the_carry_refuses_misuse_before_any_launch(emulation_library):  # noqa: F811
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="0", RG_EMU_WAVES="0"), ["-k", "refuses"])


def test_the_library_exports_the_carry():
    from rafting_amd import abi, engine
    L = engine.lib()
    for name in ("rg_assembler_carry_enable", "rg_assembler_carry_reset", "rg_assembler_carry_read", "rg_route32_carry"):
        assert name in engine.exported_symbols() and hasattr(L, name), name
    assert (abi.ASM_CARRIED, abi.ROUTE_CARRIED, abi.ROUTE_SPILLED, abi.CARRY_NEXT, abi.CARRY_LAST) == (0x40000000, 0x80000000, 0xFFFFFFFE, 0, 1)
    header = open(os.path.join(ROOT, "include", "raftgpu.h")).read()
    for name, value in (("RG_ASM_CARRIED", "0x40000000u"), ("RG_ROUTE_CARRIED", "0x80000000u"), ("RG_ROUTE_SPILLED", "0xFFFFFFFEu"), ("RG_CARRY_NEXT", "0"), ("RG_CARRY_LAST", "1")):
        assert "#define %s" % name in header and value in header.split("#define %s" % name)[1].split("\n")[0], name


def test_the_models_on_a_hand_made_chain():
    """8 groups, C = 2, D = 2. Run 1 (a carry of 4, empty): the log of tests/test_assemble_cpu.py. Run 2 (a carry of 3): one ticket, the four carried slots, two
    arrivals — a carried slot is placed behind the ticket of its group, three are deferred again, the arrival of a group beyond the list finds no slot"""
    from rafting_amd import abi
    from tests import assemble_cases as A
    from tests import carry_cases as K
    CARRIED, WENT, SPILLED, NONE = abi.ASM_CARRIED, abi.ROUTE_CARRIED, abi.ROUTE_SPILLED, 0xFFFFFFFF

    def rows(k, base):
        head, abcd = np.zeros(k, abi.HEAD_DT), np.zeros(k, abi.QUAD32_DT)
        head["hdr"], head["aux"], abcd["a"] = base + np.arange(k), base + 100 + np.arange(k), base + 200 + np.arange(k)
        return head, abcd
    head, abcd = rows(7, 100)
    w1 = K.carry_model(8, K.empty_carry(), np.array([5, 2, 9, 2, 7, 2, 5], np.uint32), head, abcd, 2, 2, 4,
                       expired=(np.array([5, 6], np.uint32), np.array([41, 42], np.uint32), 2))
    assert (w1.n, w1.R) == (2, 2) and w1.gid.tolist() == [2, 5]
    assert w1.origin.tolist() == [[1, 0x80000000], [3, 0]]
    assert w1.deferred.tolist() == [0x80000001, 4, 5, 6] and w1.stats.tolist() == [4, 4, 1, 0]
    g, h, a = w1.carry
    assert g.tolist() == [6, 7, 2, 5]
    assert (int(h["hdr"][0]), int(h["aux"][0])) == (A.TIMEOUT_HDR, 42) and tuple(a[0]) == (0, 0, 0, 0)
    assert h["hdr"][1:].tolist() == [104, 105, 106] and a["a"][1:].tolist() == [304, 305, 306]
    head2, abcd2 = rows(2, 500)
    w2 = K.carry_model(8, w1.carry, np.array([7, 3], np.uint32), head2, abcd2, 2, 2, 3, expired=(np.array([2], np.uint32), np.array([43], np.uint32), 1))
    assert w2.gid.tolist() == [2, 3]
    assert w2.origin.tolist() == [[0x80000000, 1], [0x40000002, 0xFFFFFFFF]]
    assert w2.head["hdr"].tolist() == [[A.TIMEOUT_HDR, 501], [105, 0]] and w2.head["aux"][0, 0] == 43
    assert w2.deferred.tolist() == [0x40000000, 0x40000001, 0x40000003, 0] and w2.stats.tolist() == [3, 4, 0, 1]
    assert w2.carry[0].tolist() == [6, 7, 5] and w2.spilled == 1 and w2.from_carry.tolist() == [0, 1, 3]
    assert (int(w2.carry[1]["hdr"][0]), int(w2.carry[1]["aux"][0])) == (A.TIMEOUT_HDR, 42)
    row, per = np.zeros(4, abi.OUT32_DT), np.zeros(4, abi.PERSIST32_DT)
    row["commit_index"], per["term"], row["flags"] = [0, 1, 2, 3], [70, 71, 72, 73], [0, 0, abi.F_PERSIST, abi.F_PERSIST]
    r = K.route_model(w2, 2, 2, 3, row, per)
    assert r.cell.tolist() == [SPILLED, 1] and r.expired_cell.tolist() == [0]
    assert r.carried_cell.tolist() == [WENT | 0, WENT | 1, 2, WENT | 2]
    assert r.carried_placed.tolist() == [False, False, True, False] and r.carried_row["commit_index"][2] == 2 and r.carried_persist32["term"][2] == 72
    assert r.persist_list.tolist() == [(2, 2), (3, 3)]                                  # (the lists are plain rg_route32's: every cell of the batch, an empty one too)
    assert CARRIED | 2 == 0x40000002 and NONE not in r.carried_cell.tolist()
