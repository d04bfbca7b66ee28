"""The grow-only staging buffers of the RG_MEM_HOST entry points under shapes that rise, fall and rise again — without a GPU: the product's kernels and C-ABI host
code on the host emulation (tests/devemu/emu_cases_host_staging.py, driven the way tests/test_route_cpu.py drives its cases), in wavefront mode: the compact-row
kernels and the list of fired tickets need lanes that meet."""
import os
import subprocess
import sys

from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_host_staging.py")


def test_host_staging_on_emulated_wavefronts(emulation_library):  # noqa: F811
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1")
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    par = ["-n", "2"] if __import__("importlib.util").util.find_spec("xdist") else []
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + par, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]
