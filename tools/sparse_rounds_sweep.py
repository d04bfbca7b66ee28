#!/usr/bin/env python3
"""What a tick of DEPTH R costs a host that waits for it, for a list of groups — three ways to get R rounds decided. Needs an MI355X.

    python tools/sparse_rounds_sweep.py --parent-lib PATH/libraftgpu.so [--groups 65536] [--ticks 1010] [--out profiles/sparse_rounds_sweep.jsonl]

  a  R back-to-back launches of the ONE-ROUND sparse tick (rg_tick2_create_sparse), one wait after the last: what a host had before
     rg_tick2_create_sparse_rounds. Run on --parent-lib (a build of the parent commit's library; it needs only that API).
  b  ONE launch of the sparse tick with a depth (rg_tick2_create_sparse_rounds, recorded for 8 rounds, *rounds = R). This build.
  c  ONE launch of the dense R-round tick (rg_tick2_create, recorded for R rounds), for scale. Run on --parent-lib.
Every point: 65 536 groups x 5 nodes, every column device-resident, capacity = groups, a seeded random list at fill 1 %, 10 %, 50 %, depth 1, 2, 4, 8; rows
from bench.py's tick stream (config 3's replay generator); per tick the host refills (not timed), then launch(es) + wait are timed with perf_counter, as
bench.py's tick_latency leg does; the first ten ticks are warm-up; p50, max and mean of the rest. Every leg is a fresh process; the legs alternate
a b c a b on one box, so that the spread between the two runs of a leg is in the file. One JSON line per (leg run, fill, depth)."""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FILLS = (0.01, 0.10, 0.50)
DEPTHS = (1, 2, 4, 8)
RMAX = 8
POOL = 4                                   # distinct refills per point, cycled


def leg(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("sparse_rounds_sweep: no GPU — a latency cannot be read on a CPU")
    from rafting_amd import abi, engine, workload
    G = args.groups
    cfg = workload.config(3, G)
    rng = np.random.default_rng(2024)
    for fill in FILLS:
        rows = np.sort(rng.choice(G, int(round(fill * G)), replace=False))
        gid = rows.astype(np.uint32)
        n = len(rows)
        for R in DEPTHS:
            gen = workload.ReplayGenerator(cfg)
            st0 = gen.initial_state()
            dense = [gen.next_batch(R) for _ in range(POOL)]
            cap = max(b.entry_count for b in dense) + 64
            t = engine.Table(G, cfg.cluster, cfg.self_slot, cfg.pre_vote)
            t.load_state(st0)
            t.timers_configure(900, 300, 1)
            t.timers_arm(0)
            kw = dict(entry_cap=cap, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=True)

            def listed(b, rounds):
                s = abi.Batch(rounds, n, gid=gid)
                for name in ("head", "ab", "cd"):
                    getattr(s, name)[:] = getattr(b, name).reshape(R, G)[:rounds, rows].reshape(-1)
                s.entry_terms, s.entry_count = b.entry_terms, b.entry_count
                return engine.pack32(s)
            if args.leg == "a":
                tk, launches = engine.Tick2(t, 1, sparse_cap=G, **kw), R
                pool = [listed(b, 1) for b in dense]
                clocks = lambda i: [300 * (i + 1)]                                         # noqa: E731
            elif args.leg == "b":
                tk, launches = engine.Tick2(t, RMAX, sparse_cap=G, sparse_rounds=True, **kw), 1
                pool = [listed(b, R) for b in dense]
                clocks = lambda i: [300 * (i + 1) + r for r in range(R)]                   # noqa: E731
            else:
                tk, launches = engine.Tick2(t, R, **kw), 1
                pool = [engine.pack32(b) for b in dense]
                clocks = lambda i: [300 * (i + 1) + r for r in range(R)]                   # noqa: E731
            us = []
            gc.collect()
            gc.disable()
            try:
                for i in range(args.ticks):
                    tk.refill(pool[i % POOL], clocks(i))
                    t0 = time.perf_counter()
                    for _ in range(launches):
                        tk.launch()
                    tk.wait()
                    dt = time.perf_counter() - t0
                    if i >= 10:
                        us.append(dt * 1e6)
            finally:
                gc.enable()
            us = np.sort(np.asarray(us))
            print("SPARSE_ROUNDS_SWEEP " + json.dumps(dict(
                leg=args.leg, fill=fill, rows=n, rounds=R, launches_per_tick=launches, p50_us=float(us[len(us) // 2]), max_us=float(us[-1]), mean_us=float(us.mean()),
                ticks=len(us), groups=G, cluster=cfg.cluster, library_sha16=engine.library_sha16())), flush=True)
            tk.close()
            t.close()


def child(args, which, lib, run):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("RG_LIB", None)
    if lib:
        env["RG_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--groups", str(args.groups), "--ticks", str(args.ticks)],
                       env=env, capture_output=True, text=True, timeout=1100)
    lines = [json.loads(ln[len("SPARSE_ROUNDS_SWEEP "):]) for ln in p.stdout.splitlines() if ln.startswith("SPARSE_ROUNDS_SWEEP ")]
    if p.returncode != 0 or len(lines) != len(FILLS) * len(DEPTHS):
        sys.exit("sparse_rounds_sweep: leg %s failed (%d): %s" % (which, p.returncode, (p.stdout + p.stderr)[-2000:]))
    return [dict(ln, run=run, build="parent" if lib else "this") for ln in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=1010, help="ticks per point; the first ten are warm-up")
    ap.add_argument("--parent-lib", default=None, help="a build of libraftgpu.so from the parent commit: legs a and c run on it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_rounds_sweep.jsonl"))
    ap.add_argument("--leg", default=None, choices=("a", "b", "c"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    if not os.path.exists("/dev/kfd"):
        sys.exit("sparse_rounds_sweep: no GPU — a latency cannot be read on a CPU")
    if not args.parent_lib:
        sys.exit("sparse_rounds_sweep: --parent-lib is required (legs a and c are the parent commit's)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for run, (which, lib) in enumerate((("a", args.parent_lib), ("b", None), ("c", args.parent_lib), ("a", args.parent_lib), ("b", None))):
            for ln in child(args, which, lib, run):
                f.write(json.dumps(ln) + "\n")
                f.flush()
                print(json.dumps(ln), flush=True)


if __name__ == "__main__":
    main()
