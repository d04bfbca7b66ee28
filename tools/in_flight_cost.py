"""What RG_OPT_DEVICE_IN_FLIGHT costs the tick: device microseconds per QUEUED tick (ticks launched back to back on the table's stream inside one rg_timing_begin /
rg_timing_end region after a warm-up — the quantity bench.py --full reports as device_us_per_resident_tick) of the sparse tick with a depth at 65 536 groups x 5
nodes, every column device-resident, at fills 1 %, 10 % and 100 % and depths 1 and 4, config 3's stream (rafting_amd/workload.py), three ways:
    (a) --parent-lib: a libraftgpu.so built from the PARENT commit, host columns (heartbeat random, nothing in flight);
    (b) this tree, the option off, the same columns — must equal (a) within the spread that alternating runs of (a) against (a) show on the same box;
    (c) this tree, the option on, no host column.
One library per process: the tool starts a fresh child per (variant, repetition), (a) (a) (b) (c) in turn, --reps times, so every variant sees the same drift.
A reading depends on its place in the turn (the first child after another library's ran 3 - 5 % slower than the second of the same library when the order was
fixed), so the turn is rotated by one place per repetition: with --reps a multiple of 4 every variant stands in every place equally often ("order": "rotated").
One JSON line per (fill, depth), appended to --out: the medians, every sample, the (a)-against-(a) spread, (b) and (c) against (a). Needs an MI355X.
    python tools/in_flight_cost.py --parent-lib /path/to/parent/libraftgpu.so [--reps 8] [--ticks 40] [--out profiles/in_flight_cost.jsonl]
Without --parent-lib only (b) and (c) are taken and (c) is quoted against (b)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G, P, RMAX = 65536, 5, 4
POINTS = [(fill, depth) for fill in (0.01, 0.1, 1.0) for depth in (1, 4)]


def child(option_on, ticks):
    """every point with the library this process has loaded -> one JSON line on stdout"""
    import numpy as np

    from rafting_amd import abi, engine, workload
    cfg = workload.config(3, G)
    out = {}
    for fill, depth in POINTS:
        gen = workload.ReplayGenerator(cfg)
        t = engine.Table(G, P, cfg.self_slot, cfg.pre_vote)
        if option_on:
            t.set_device_in_flight(True)
        t.load_state(gen.initial_state())
        t.timers_configure(900, 300, 1)
        t.timers_arm(0)
        tick = engine.Tick2(t, RMAX, entry_cap=8 * G * RMAX, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=True, sparse_cap=G, sparse_rounds=True)
        rng = np.random.default_rng(7)
        rows = np.arange(G) if fill >= 1.0 else np.sort(rng.choice(G, max(int(round(fill * G)), 1), replace=False))
        n = len(rows)
        triggered = 0
        for k in range(6):                                 # five warm-up ticks on fresh rows, the sixth is the one that is queued `ticks` times
            b = gen.next_batch(depth)
            sub = abi.Batch(depth, n, gid=rows.astype(np.uint32))
            sub.head[:] = b.head.reshape(depth, G)[:, rows].reshape(-1)
            sub.ab[:], sub.cd[:] = b.ab.reshape(depth, G)[:, rows].reshape(-1), b.cd.reshape(depth, G)[:, rows].reshape(-1)
            sub.entry_terms, sub.entry_count = b.entry_terms, b.entry_count
            now = [300 * (k + 1) + r for r in range(depth)]
            if option_on:
                tick.refill(sub, now)
            else:
                tick.refill(sub, now, heartbeat=(rng.random(n) < 0.5).astype(np.uint8))
            if k < 5:
                tick.launch()
                tick.wait()
        t.sync()
        t.timing_begin()
        for _ in range(ticks):
            tick.launch()
        ms = t.timing_end()
        tick.wait()
        if option_on:
            triggered = int(np.count_nonzero(tick.sends()[0]["reserved"] & abi.SENT_TRIGGERED))
        out["%g/%d" % (fill, depth)] = {"us": ms * 1e3 / ticks, "rows": n, "triggered_rows_last_tick": triggered}
        tick.close()
        t.close()
    print(json.dumps({"points": out, "library_sha16": engine.library_sha16()}))


def run_child(lib, option_on, ticks):
    env = dict(os.environ)
    env.pop("RG_LIB", None)
    if lib:
        env["RG_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--ticks", str(ticks)] + (["--on"] if option_on else []), env=env, capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        sys.exit("in_flight_cost: the child failed (%d)\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "in_flight_cost.jsonl"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--on", action="store_true")
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("in_flight_cost: no GPU — a device time cannot be read on a CPU")
    if args.child:
        return child(args.on, args.ticks)
    order = ([("a", args.parent_lib, False), ("a2", args.parent_lib, False)] if args.parent_lib else []) + [("b", None, False), ("c", None, True)]
    got = {name: [] for name, _, _ in order}
    for rep in range(args.reps):
        for name, lib, on in order[rep % len(order):] + order[:rep % len(order)]:
            got[name].append(run_child(lib, on, args.ticks))
            print("in_flight_cost: repetition %d of %d, (%s) done" % (rep + 1, args.reps, name), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for fill, depth in POINTS:
            key = "%g/%d" % (fill, depth)
            us = {name: [r["points"][key]["us"] for r in runs] for name, runs in got.items()}
            med = {name: statistics.median(v) for name, v in us.items()}
            line = {"groups": G, "cluster": P, "fill": fill, "depth": depth, "rows": got["b"][0]["points"][key]["rows"], "queued_ticks": args.ticks, "reps": args.reps, "order": "rotated",
                    "b_option_off_us": med["b"], "c_option_on_us": med["c"], "samples_us": us,
                    "c_triggered_rows_last_tick": got["c"][0]["points"][key]["triggered_rows_last_tick"],
                    "library_sha16": got["b"][0]["library_sha16"]}
            if args.parent_lib:
                base = statistics.median(us["a"] + us["a2"])
                line.update({"a_parent_us": base, "parent_library_sha16": got["a"][0]["library_sha16"],
                             "a_vs_a_spread": max(abs(x - y) for x, y in zip(us["a"], us["a2"])) / base,
                             "a_vs_a_median_gap": abs(med["a"] - med["a2"]) / base,
                             "b_vs_a": med["b"] / base - 1.0, "c_vs_a": med["c"] / base - 1.0})
                line["b_within_spread"] = abs(line["b_vs_a"]) <= line["a_vs_a_spread"]
            else:
                line["c_vs_b"] = med["c"] / med["b"] - 1.0
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
