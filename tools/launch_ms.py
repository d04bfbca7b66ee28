"""Milliseconds per launch of one kernel body on a replayed stream, by HIP events over a region of launches — for same-box A/Bs of two builds of the library on
the legs bench.py's plain line does not time: another cluster size (the 7-node variants of the compact kernels at more than 65 536 groups: the
128-VGPR ones), the 64-bit body on compact rows (RG_FORCE_WIDE=1), wide rows (rg::step_split_kernel / rg::step_kernel). Uses only the interfaces of
ABI 5, so the same file runs against an older tree. Prints one JSON line.
    python tools/launch_ms.py [--config 3] [--cluster 7] [--groups 131072] [--rounds 64] [--launches 20] [--body compact|int64|wide]"""
import argparse
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rafting_amd import engine, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--cluster", type=int, default=None)
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--body", choices=("compact", "int64", "wide"), default="compact")
    args = ap.parse_args()
    cfg = workload.config(args.config, args.groups)
    if args.cluster:
        cfg = dataclasses.replace(cfg, cluster=args.cluster, name=cfg.name + " [cluster=%d]" % args.cluster)
    if args.body == "int64":
        os.environ["RG_FORCE_WIDE"] = "1"                      # read by rg_table_create
    gen = workload.ReplayGenerator(cfg)
    t = engine.Table(cfg.groups, cfg.cluster, cfg.self_slot, cfg.pre_vote)
    t.load_state(gen.initial_state())
    dbs = []
    for _ in range(args.launches + 2):
        b = gen.next_batch(args.rounds)
        dbs.append(engine.DeviceBatch(t, b) if args.body == "wide" else engine.DeviceBatch32(t, engine.pack32(b), compact=True, wide=False))
    for i in range(2):
        t.submit_device(dbs[i])
    t.sync()
    t.wide_body_workgroups(reset=True)
    t.timing_begin()
    for i in range(2, len(dbs)):
        t.submit_device(dbs[i])
    ms = t.timing_end()
    t.sync()
    print(json.dumps({"config": cfg.name, "body": args.body, "groups": cfg.groups, "cluster": cfg.cluster, "rounds": args.rounds, "launches": args.launches,
                      "ms_per_launch": ms / args.launches, "int64_body_workgroups": t.wide_body_workgroups(),
                      "kernel": t.step_kernel() if args.body == "wide" else ("rg::step32_wide_kernel" if args.body == "int64" else "rg::step32_kernel")}))
    for db in dbs:
        db.free()
    t.close()


if __name__ == "__main__":
    main()
