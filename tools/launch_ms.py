"""Milliseconds per launch of one kernel body on a replayed stream, by HIP events over a region of launches — for same-box A/Bs of two builds of the library on
the legs bench.py's plain line does not time: another cluster size (the 7-node variants of the compact kernels at more than 65 536 groups: the
128-VGPR ones), the 64-bit body on compact rows (RG_FORCE_WIDE=1), wide rows (rg::step_split_kernel / rg::step_kernel). Uses only the interfaces of
ABI 5, so the same file runs against an older tree. Prints one JSON line.
    python tools/launch_ms.py [--config 3] [--cluster 7] [--groups 131072] [--rounds 64] [--launches 20] [--body compact|int64|wide] [--against BODY [--pairs 3]]
--against times a second body on the same staged stream in the same process, the two legs in turn (clusters above 7 nodes: the table of a compact-row leg gets
RG_OPT_COMPACT_ANY_CLUSTER)."""
import argparse
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rafting_amd import abi, engine, workload  # noqa: E402


def make_table(cfg, body):
    """a table for one body of the step kernel: compact = the 32-bit body on compact rows, int64 = its 64-bit body (RG_FORCE_WIDE=1, read by rg_table_create), wide = wide rows"""
    saved = os.environ.get("RG_FORCE_WIDE")
    if body == "int64":
        os.environ["RG_FORCE_WIDE"] = "1"
    else:
        os.environ.pop("RG_FORCE_WIDE", None)
    try:
        t = engine.Table(cfg.groups, cfg.cluster, cfg.self_slot, cfg.pre_vote)
    finally:
        if saved is None:
            os.environ.pop("RG_FORCE_WIDE", None)
        else:
            os.environ["RG_FORCE_WIDE"] = saved
    if cfg.cluster > abi.MAX_COMPACT_CLUSTER and body != "wide":
        t.set_compact_any_cluster(True)                        # (RG_OPT_COMPACT_ANY_CLUSTER: the compact formats above 7 nodes)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--cluster", type=int, default=None)
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--body", choices=("compact", "int64", "wide"), default="compact")
    ap.add_argument("--against", choices=("compact", "int64", "wide"), default=None,
                    help="a second body on the SAME staged stream, the two timed in turn --pairs times in this process (one line per leg and pair)")
    ap.add_argument("--pairs", type=int, default=3)
    args = ap.parse_args()
    cfg = workload.config(args.config, args.groups)
    if args.cluster:
        cfg = dataclasses.replace(cfg, cluster=args.cluster, name=cfg.name + " [cluster=%d]" % args.cluster)
    gen = workload.ReplayGenerator(cfg)
    st0 = gen.initial_state()
    batches = [gen.next_batch(args.rounds) for _ in range(args.launches + 2)]
    legs = []
    for body in [args.body] + ([args.against] if args.against else []):
        t = make_table(cfg, body)
        legs.append((body, t, [engine.DeviceBatch(t, b) if body == "wide" else engine.DeviceBatch32(t, engine.pack32(b), compact=True, wide=False) for b in batches]))
    del batches
    for pair in range(args.pairs if args.against else 1):
        for body, t, dbs in legs:
            t.load_state(st0)                                  # (every timed region replays the stream from its start)
            for i in range(2):
                t.submit_device(dbs[i])
            t.sync()
            t.wide_body_workgroups(reset=True)
            t.timing_begin()
            for i in range(2, len(dbs)):
                t.submit_device(dbs[i])
            ms = t.timing_end()
            t.sync()
            print(json.dumps({"config": cfg.name, "body": body, "groups": cfg.groups, "cluster": cfg.cluster, "rounds": args.rounds, "launches": args.launches,
                              "ms_per_launch": ms / args.launches, "int64_body_workgroups": t.wide_body_workgroups(), "pair": pair,
                              "kernel": t.step_kernel() if body == "wide" else ("rg::step32_wide_kernel" if body == "int64" else "rg::step32_kernel")}), flush=True)
    for _, t, dbs in legs:
        for db in dbs:
            db.free()
        t.close()


if __name__ == "__main__":
    main()
