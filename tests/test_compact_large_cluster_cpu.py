"""RG_OPT_COMPACT_ANY_CLUSTER — the compact formats and the ticks for tables of 8 .. 15 nodes — without a GPU: the product's device code and C-ABI host code
on the host emulation (tests/devemu/emu_cases_compact_large_cluster.py, driven the way tests/test_sparse_rounds_cpu.py drives its cases). Wavefront mode: the
cases of tests/test_compact_large_cluster_gpu.py at small table sizes; lane-serial mode: the refusals, which happen on the host before any launch."""
import os
import subprocess
import sys

from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_compact_large_cluster.py")


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_clusters_above_seven_nodes_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)


def test_the_option_refuses_misuse_before_any_launch(emulation_library):  # noqa: F811
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="0", RG_EMU_WAVES="0"), ["-k", "refuses"])
