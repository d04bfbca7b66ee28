"""RG_OPT_DEVICE_IN_FLIGHT without a GPU. (1) The product's device code and C-ABI host code on the host emulation (tests/devemu/emu_cases_in_flight.py, driven the
way tests/test_sparse_rounds_cpu.py drives its cases): wavefront mode for the cases of tests/test_in_flight_gpu.py at small table sizes, lane-serial mode for the
refusals. (2) The oracle-and-model-only twin of the fuzzed lockstep at the sizes the MI355X runs: every stream reaches every line of in_flight_cases.MUST_SEE, so a
run on the device that passes has been through all of them."""
import os
import subprocess
import sys

import pytest

from tests import in_flight_cases as I
from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)
from tests.test_in_flight_gpu import NINE_NODES, SIZES

CASES = os.path.join(EMU, "emu_cases_in_flight.py")


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_device_resident_in_flight_counts_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)


def test_the_option_and_its_entry_points_refuse_misuse_before_any_launch(emulation_library):  # noqa: F811
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="0", RG_EMU_WAVES="0"), ["-k", "refusals"])


@pytest.mark.parametrize("G,P,seed,ticks,first", SIZES + [NINE_NODES])
def test_the_streams_of_the_gpu_lockstep_reach_every_rule(G, P, seed, ticks, first):
    seen = I.lead_only(G, P, seed, ticks, first=first)
    assert all(seen[k] > 0 for k in I.MUST_SEE), seen
