"""The clock points of tests/clock_domain_cases.py without a GPU. First what can be shown on the oracle and the stream alone: every stand-alone loop reaches what
it is there for (tickets fire, a short buffer leaves some for the next call, readiness answers both ways under every health setting, every branch of
RaftRoutine.resetTimer is taken, every election draw lies in [now + E, now + 2E]), a cross* run has deadlines and requestSuccess values on both sides of its power
of two, the low word of a clock does not decide a draw, a call of more than 64 rounds carries a conversion across the chunk boundary; and at the default origin
the case modules give the oracle the clocks they always gave it. Then the same cases as tests/test_clock_domain_gpu.py on the host emulation of the kernels in
wavefront mode (tests/devemu/emu_cases_clock_domain.py)."""
import os
import subprocess
import sys

import pytest

from tests import clock
from tests import clock_domain_cases as D
from tests import sparse_rounds_cases as X
from tests.test_devemu_cpu import EMU, ROOT, emulation_library  # noqa: F401  (the fixture that builds the emulation library)

CASES = os.path.join(EMU, "emu_cases_clock_domain.py")


def test_the_origin_moves_every_clock_and_comes_back():
    assert clock.origin() == clock.DEFAULT == 10_000 and X.now_of(3, 2) == 10_470
    with clock.at(D.POINTS["epoch_ms"]):
        assert clock.origin() == 1_760_000_000_000 and X.now_of(3, 2) == 1_760_000_000_470
        with clock.at(1 << 62):
            assert clock.origin() == 1 << 62
        assert clock.origin() == 1_760_000_000_000
    assert clock.origin() == 10_000


def test_the_clock_points_are_inside_the_domain_to_the_last_draw():
    last = max(D.POINTS.values()) + D.TICK_MS * D.TICKS + 2 * D.E_MS + D.HB_MS
    assert min(D.POINTS.values()) >= 1 and max(D.POINTS.values()) == D.NOW_MAX and last < D.INT64_MAX
    for point, k in D.CROSSES.items():
        assert D.POINTS[point] < 1 << k < D.POINTS[point] + D.TICK_MS * (D.TICKS - 1)


def test_the_default_origin_gives_the_oracle_the_clocks_it_always_got():
    assert D.default_origin_digest(device=False) == D.DEFAULT_LEAD_DIGEST


@pytest.mark.parametrize("cluster", D.CLUSTERS)
@pytest.mark.parametrize("point", D.POINTS)
def test_every_loop_reaches_what_it_is_there_for(point, cluster):
    st = D.lead(point, cluster)
    print(point, cluster, st.fired_rounds, st.fired, st.late, st.branches, st.bites)
    D.check_reach(point, cluster, st)


def test_the_low_word_of_a_clock_does_not_decide_a_draw():
    D.low_word_case(device=False)


@pytest.mark.parametrize("rounds", [r for r in D.LONG_ROUNDS if r > D.CHUNK])
def test_a_long_call_carries_a_conversion_across_its_chunks(rounds):
    L = D.long_lead()
    hit = D.long_reach(L, rounds)
    print(rounds, hit)
    assert hit


def _run(env, extra):
    env = dict(os.environ, RG_ALLOW_HOST_EMULATION="1", PYTHONPATH=ROOT, **env)
    for k in ("RG_FAST", "RG_FORCE_WIDE", "RG_TICK_NODES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-x", "-q", "-p", "no:cacheprovider"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-3000:]
    assert " passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_the_clock_points_on_emulated_wavefronts(emulation_library):  # noqa: F811
    par = ["-n", "4"] if __import__("importlib.util").util.find_spec("xdist") else []
    _run(dict(RG_LIB=emulation_library, RG_SPLIT="1", RG_EMU_WAVES="1"), par)
