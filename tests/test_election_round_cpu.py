"""The election block of the 32-bit step body (rg_tier1n.hpp) without a GPU: the hand-built streams of tests/election_round_cases.py on the host emulation of
the kernels (tests/devemu/emu_cases_election_round.py, wavefront mode, driven the way tests/test_route_cpu.py drives its cases) — outcome rows, persist rows and
the table against the oracle on the 32-bit body and on the 64-bit one, and not one row handed to the general handlers — and, on the oracle alone, that the
streams reach what they were built to reach."""
import os
import subprocess
import sys

import pytest

from tests import election_round_cases as E
from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_election_round.py")


@pytest.mark.parametrize("P", E.CLUSTERS)
def test_the_streams_reach_every_sub_block_alone_and_together(P):
    seen = E.reach(P)
    assert all(seen.values()), {k: v for k, v in seen.items() if not v}


def test_election_rounds_on_emulated_wavefronts(emulation_library):  # noqa: F811
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1")
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + par, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]
