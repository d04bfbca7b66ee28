"""What rg_scan and the state lists cost, at 65 536 and 1 048 576 groups x 5 nodes, on one build: (a) a device-memory rg_scan — `runs` scans queued back to back
on the table's stream inside ONE rg_timing_begin / rg_timing_end region (an event pair) after a warm-up, with the bits column and a list that holds every selected
group —; (b) what it replaces: rg_read_state of the whole table plus the numpy model of tests/scan_cases.py, wall clock, best of three; (c) read_state_list of
1 000 scattered gids against 1 000 single-group rg_read_state calls, wall clock, best of three. `layout_bytes` is what the class kernel reads BY LAYOUT — 160 bytes a
group (nine 16-byte columns, the timer, the base) and 32 per follower of a group whose `prepared` mark is set — plus the 4-byte class word it writes: a layout
estimate, not a counter reading; `share_of_peak` sets it against 8 TB/s over the measured time of the whole scan (its four launches). One JSON line per size,
appended to --out. Needs an MI355X: there is no CPU reading of a device time.
    python tools/scan_cost.py [--runs 50] [--out profiles/scan_cost.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rafting_amd import abi, engine  # noqa: E402
from tests import scan_cases as S  # noqa: E402

P, LISTED, PEAK = 5, 1000, 8e12


def best(fn, times=3):
    out = []
    for _ in range(times):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def point(G, runs, rng):
    t = engine.Table(G, P, 1)
    st = S.random_state(G, P, rng)
    t.load_state(st)
    t.timers_configure(900, 300, 7)
    t.timers_arm(1000)
    q = dict(any=abi.SCAN_NO_LEADER | abi.SCAN_TIMEOUT_DETECTED | abi.SCAN_PENDING_INSTALL | abi.SCAN_LAGGING | abi.SCAN_RUNS_FULL, backlog=12, lag=10, now=1500)
    bits, gids, summary = engine.DeviceBuffer(t, 4 * G), engine.DeviceBuffer(t, 4 * G), engine.DeviceBuffer(t, 8 * abi.SCAN_SUMMARY)
    cq, cr = abi.CScanQuery(reserved=0, **q), abi.CScanResult(bits=bits.ptr, list=gids.ptr, list_capacity=G, summary=summary.ptr)
    for _ in range(5):
        t.scan_device(cq, cr)
    t.sync()
    t.timing_begin()
    for _ in range(runs):
        t.scan_device(cq, cr)
    scan_us = t.timing_end() * 1e3 / runs
    t.sync()
    selected = int(summary.to_host(np.uint64, abi.SCAN_SUMMARY)[abi.SCAN_SELECTED])
    want = S.model_of(t, **q)
    assert selected == len(want.selected) and np.array_equal(gids.to_host(np.uint32, G)[:selected], want.selected)
    prepared = int(np.count_nonzero(st.repl_prepared))
    layout = G * 160 + prepared * (P - 1) * 32 + G * 4
    host_s = best(lambda: S.model_of(t, **q))
    read_s = best(lambda: t.read_state())
    listed = rng.choice(G, LISTED, replace=False).astype(np.uint32)
    by_list_s = best(lambda: t.read_state_list(listed))
    one_by_one_s = best(lambda: [t.read_state(int(g), 1) for g in listed])
    for b in (bits, gids, summary):
        b.free()
    t.close()
    return {"groups": G, "cluster": P, "runs": runs, "scan_us": scan_us, "selected": selected, "prepared_leaders": prepared, "layout_bytes": layout,
            "share_of_peak": layout / (scan_us * 1e-6) / PEAK, "read_state_ms": read_s * 1e3, "read_state_plus_model_ms": host_s * 1e3,
            "listed": LISTED, "read_state_list_ms": by_list_s * 1e3, "single_group_reads_ms": one_by_one_s * 1e3, "library_sha16": engine.library_sha16()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_cost.jsonl"))
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("scan_cost: no GPU — a device time cannot be read on a CPU")
    assert args.runs >= 20
    rng = np.random.default_rng(2026)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for G in (65536, 1048576):
            line = json.dumps(point(G, args.runs, rng))
            print(line)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
