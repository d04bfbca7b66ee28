"""The magnitude points of tests/domain_edge_cases.py without a GPU. First what can be shown on the oracle and the stream alone (as tests/test_in_flight_cpu.py does
for its rules): every stream hits the row classes it claims to, stays inside the domain it claims to stay in, and the fuzzer's additions leave every stream drawn
before them byte for byte as it was. Then the same cases as tests/test_domain_edge_gpu.py on the host emulation of the kernels in wavefront mode
(tests/devemu/emu_cases_domain_edge.py), where the RG_NEED_HOST share is held to its cap."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from rafting_amd import abi
from tests import domain_edge_cases as D
from tests import fuzz, oracle_lib
from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_domain_edge.py")
# sha256 over the initial state (every column), twelve rounds of rows drawn from the oracle's state (head, ab, cd, entry terms) and the initial state at offset 2^40:
# 48 groups, 5 nodes, self 1, seed 4242 — recorded from the fuzzer as it was before it learnt about magnitudes
DEFAULT_STREAM = "a5bc7c53e4884138d14a05edd1cb8b8be4b11b828cf42b5ec8b4cde8497b51c7"


def test_the_default_stream_is_byte_for_byte_what_it_was():
    groups, P, seed = 48, 5, 4242
    st0 = fuzz.random_initial_state(groups, P, 1, seed)
    orc = oracle_lib.OracleTable(groups, P, 1, True)
    orc.load_state(st0)
    fz = fuzz.Fuzzer(groups, P, 1, seed, allow_miss=True)
    h = hashlib.sha256()
    for f in st0.fields():
        h.update(np.ascontiguousarray(getattr(st0, f)).tobytes())
    for _ in range(12):
        b = abi.Batch(1, groups)
        fz.round(orc.read_state(), b, 0)
        orc.submit(b)
        for a in (b.head, b.ab, b.cd, b.entry_terms[:b.entry_count]):
            h.update(np.ascontiguousarray(a).tobytes())
    st1 = fuzz.random_initial_state(groups, P, 1, seed, offset=1 << 40)
    for f in st1.fields():
        h.update(np.ascontiguousarray(getattr(st1, f)).tobytes())
    orc.close()
    assert h.hexdigest() == DEFAULT_STREAM


def test_the_offsets_move_a_state_and_nothing_else():
    """term_offset / epoch_offset: the image of the same seed with terms / role epochs moved up, zero terms left at zero, everything else untouched"""
    groups, P, seed, dt, de = 96, 5, 77, 1000, 500
    a, b = fuzz.random_initial_state(groups, P, 2, seed), fuzz.random_initial_state(groups, P, 2, seed, term_offset=dt, epoch_offset=de)
    assert np.array_equal(b.current_term, a.current_term + dt) and np.array_equal(b.role_epoch, a.role_epoch + de)
    assert np.array_equal(b.epoch_term, np.where(a.epoch_term != 0, a.epoch_term + dt, 0)) and np.any(a.epoch_term == 0) and np.any(a.epoch_term != 0)
    live = (np.arange(abi.TERM_RUNS)[None, :] < a.run_count[:, None]).reshape(-1)
    assert np.array_equal(b.run_term[live], a.run_term[live] + dt) and not b.run_term[~live].any()
    assert not b.elected_term.any() and not b.elected_epoch.any()
    for f in a.fields():
        if f not in ("current_term", "role_epoch", "epoch_term", "run_term"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    a.elected_term[:8], a.elected_epoch[:8] = 3, 2                # (a leader elected in term 3 by participant 2: both move with the rest)
    fuzz.shift_state(a, term_offset=dt, epoch_offset=de, groups=slice(0, 16))
    assert np.all(a.elected_term[:8] == 3 + dt) and np.all(a.elected_epoch[:8] == 2 + de) and not a.elected_term[8:].any() and not a.elected_epoch[8:].any()
    assert np.array_equal(a.current_term[:16], b.current_term[:16]) and np.array_equal(a.current_term[16:] + dt, b.current_term[16:])


@pytest.mark.parametrize("point,cluster", D.SHAPES)
def test_every_stream_stays_in_its_domain_and_reaches_its_row_classes(point, cluster):
    """on the oracle and the stream alone: no value at or above 2^30 where none is expected (and growth within SPAN), `straddle` out of the domain in its second
    workgroup only, and every row class the point is there for occurs"""
    L = D.lead(point, cluster)
    top = D.check_domain(L)
    seen = D.reach(L)
    print(point, cluster, top, seen)
    missing = [c for c in D.required(point) if not seen[c]]
    assert not missing, (point, cluster, missing, seen)


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_the_magnitude_points_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)
