"""rg_scan and the state exchange by a list of groups without a GPU: the product's kernels and C-ABI host code on the host emulation
(tests/devemu/emu_cases_scan.py, driven the way tests/test_route_cpu.py drives its cases). Wavefront mode: the cases of tests/test_scan_gpu.py at small table
sizes; lane-serial mode: the refusals, which happen on the host before any launch. The numpy model the scan is held against is checked here on a hand-made
table, without any library."""
import os
import subprocess
import sys

import numpy as np

from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_scan.py")


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_scanning_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)


def test_scan_and_the_state_lists_refuse_misuse_before_any_launch(emulation_library):  # noqa: F811
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="0", RG_EMU_WAVES="0"), ["-k", "refuse"])


def test_the_binding_names_the_new_entry_points():
    from rafting_amd import abi, engine
    for name in ("rg_scan", "rg_read_state_list", "rg_load_state_list"):
        assert name in engine.exported_symbols() and hasattr(engine.lib(), name), name
    for name in ("scan", "scan_device", "read_state_list", "load_state_list"):
        assert callable(getattr(engine.Table, name)), name
    header = open(os.path.join(ROOT, "include", "raftgpu.h")).read()
    for b, name in enumerate(abi.SCAN_BIT_NAMES):
        assert getattr(abi, "SCAN_" + name) == 1 << b and "#define RG_SCAN_%s" % name in header, name
        assert __import__("re").search(r"#define RG_SCAN_%s\s+\(1u << %d\)" % (name, b), header), name
    assert "#define RG_SCAN_SUMMARY %d" % abi.SCAN_SUMMARY in header


def test_the_scan_model_on_a_hand_made_table():
    """eight groups of a 3-node table written out by hand (thresholds: backlog 5, lag 10, now 1000), every one of the 16 bits set in at least one group and clear in
    at least one; the words, a list and the summary asserted literally"""
    from rafting_amd import abi
    from tests import scan_cases as S
    st = abi.GroupState(8, 3)
    base, deadline = np.zeros(8, np.int64), np.zeros(8, np.int64)
    # 0: a fresh group — Follower, no leader, empty log, no ticket
    # 1: a Follower of node 1 with timeoutDetected, log 1 .. 10 committed to 2 (8 behind), its ticket overdue
    st.current_leader[1], st.timeout_detected[1], st.current_term[1], st.commit_index[1], deadline[1] = 1, 1, 3, 2, 500
    st.set_log(1, 1, [(1, 3)], 10)
    # 2: a Candidate whose four run slots are full, everything committed, its ticket fired
    st.role[2], st.current_term[2], st.voted_for[2], st.commit_index[2], deadline[2] = abi.CANDIDATE, 9, 0, 40, -1
    st.set_log(2, 1, [(1, 2), (11, 4), (21, 6), (31, 8)], 40)
    # 3: a Leader that has not prepared replication, log 1 .. 20 all committed, ticket armed for 2000
    st.role[3], st.current_term[3], st.voted_for[3], st.commit_index[3], deadline[3] = abi.LEADER, 4, 0, 20, 2000
    st.set_log(3, 1, [(1, 4)], 20)
    # 4: a prepared Leader, log 1 .. 100 committed to 98; follower 0 has it all, follower 1 matches 85 (15 behind) and waits for a snapshot
    st.role[4], st.current_term[4], st.voted_for[4], st.repl_prepared[4], st.commit_index[4], deadline[4] = abi.LEADER, 5, 0, 1, 98, 2000
    st.set_log(4, 1, [(1, 5)], 100)
    st.peers("match_index")[4], st.peers("next_index")[4], st.peers("pending")[4] = [100, 85], [101, 86], [0, 1]
    # 5: a Follower of node 2 whose term has reached 2^30: off the 32-bit image; empty log, no ticket
    st.current_leader[5], st.current_term[5] = 2, 1 << 30
    # 6: a Follower of node 0 with an index base of 1000 it lies well above: epoch 1500, log 1501 .. 1600 committed to 1550; ticket due exactly now
    st.current_leader[6], st.current_term[6], st.epoch_index[6], st.epoch_term[6], st.commit_index[6], base[6], deadline[6] = 0, 2, 1500, 1, 1550, 1000, 1000
    st.set_log(6, 1501, [(1501, 2)], 1600)
    # 7: a prepared Leader whose base of 5000 IS its epoch.index — no image —, log 5001 .. 5010 committed and matched everywhere
    st.role[7], st.current_term[7], st.voted_for[7], st.repl_prepared[7], st.epoch_index[7], st.epoch_term[7], st.commit_index[7] = abi.LEADER, 6, 0, 1, 5000, 5, 5010
    base[7], deadline[7] = 5000, 3000
    st.set_log(7, 5001, [(5001, 6)], 5010)
    st.peers("match_index")[7], st.peers("next_index")[7], st.peers("last_epoch")[7] = [5010, 5010], [5011, 5011], [5000, 5000]
    m = S.model(st, base, deadline, any=abi.SCAN_OFF_IMAGE | abi.SCAN_BACKLOG, none=abi.SCAN_LEADER, backlog=5, lag=10, now=1000, capacity=2)
    assert m.bits.tolist() == [0x2029, 0x8091, 0x4042, 0x0104, 0x0604, 0x2821, 0x9081, 0x1804]
    assert m.selected.tolist() == [1, 5, 6] and m.list.tolist() == [1, 5]
    assert m.summary.tolist() == [4, 1, 3, 1, 1, 2, 1, 2, 1, 1, 1, 2, 2, 2, 1, 2, 3, 1 << 30, 50, 60, 15, 0, 0, 0]
    for b in range(16):
        assert 0 < m.summary[b] < 8, b
    everything = S.model(st, base, deadline, backlog=5, lag=10, now=1000)
    assert everything.selected.tolist() == list(range(8)) and S.model(st, base, deadline, all=0xFFFF).selected.tolist() == []
    assert S.model(st, base, deadline, all=abi.SCAN_LEADER | abi.SCAN_HAS_BASE).selected.tolist() == [7]
