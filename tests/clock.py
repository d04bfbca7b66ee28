"""The clock origin of the shared case modules. Every `now` of tests/test_gpu_parity.py's tick cases, tests/sparse_tick_cases.py, tests/sparse_rounds_cases.py,
tests/in_flight_cases.py, tests/assemble_cases.py and tests/devemu/emu_cases_sparse_tick.py is origin() + a small offset: 10_000 by default — the streams the
suite has always run — and, under `with clock.at(point):`, a clock of the magnitude real hosts pass (System.currentTimeMillis() is about 2^40.7) or one that
crosses 2^31 or 2^32 within the run (tests/clock_domain_cases.py). Clocks only enter the timer and health columns, never the fuzzer's draws, so the rows of a
stream do not depend on the origin; the fired tickets do (the election draw hashes `now`), which is why a case is recorded from the oracle at ITS origin."""
import contextlib

DEFAULT = 10_000
_origin = [DEFAULT]


def origin():
    return _origin[-1]


@contextlib.contextmanager
def at(value):
    """every clock of the case modules starts at `value` inside the block"""
    _origin.append(int(value))
    try:
        yield int(value)
    finally:
        _origin.pop()
