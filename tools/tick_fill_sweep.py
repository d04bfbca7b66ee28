#!/usr/bin/env python3
"""What the recorded tick costs on the device as a function of its FILL — the share of the table's groups that have a row — for the sparse tick
(rg_tick2_create_sparse), next to the dense tick (rg_tick2_create) on the same table size. Needs an MI355X: there is no CPU reading of a device time.

    python tools/tick_fill_sweep.py [--groups 65536] [--ticks 2000] [--parent-lib PATH/libraftgpu.so] [--out profiles/tick_fill_sweep.json]

State and rows are those of bench.py's tick leg (config 3's replay stream, single-round batches); every column is device-resident; the lists are seeded
random subsets of the groups. Per recording the two readings bench.py takes of the dense tick:
    device_us       --ticks replays queued back to back on the table's stream inside ONE timing_begin / timing_end region, after warm-up: what the device
                    spends per tick
    idle_stream_us  one event pair around one replay on an idle stream: what a host that waits for every tick sees (contains its own submission path)
and `layout_bytes_per_tick`, which is NOT measured: rows x the bytes the columns' layouts give a row, + 8 bytes per group of the table for the expiry.
--parent-lib: the dense tick is ALSO read from that build of the library (the parent commit's), alternating parent / this build three times, each leg a
fresh process — this change edits files the dense tick is compiled from, and the spread of the parent's three readings is the yardstick."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FILLS = (1.0, 0.5, 0.25, 0.10, 0.05, 0.01)
CLUSTER = 5


def row_bytes(F):
    """bytes a listed row moves, from the layouts: the five 16-byte state records read and written, the 24-byte event row and its 4-byte gid, the 16-byte
    outcome row, the 48-byte send head and F 32-byte send rows, heartbeat + F in-flight counts + readiness, deadline and timer epoch read and written.
    Not counted (conditional): persist32 rows, term runs and follower records of leaders, the health statistics an ack touches."""
    return 2 * 5 * 16 + 24 + 4 + 16 + 48 + 32 * F + 1 + 2 * F + 1 + 2 * (8 + 4)


def readings(table, tick, refills, queued):
    """bench.py's two readings of a recorded tick: idle-stream time over the refills after the tenth, queued-tick device time over `queued` replays"""
    t_idle = 0.0
    for i, refill in enumerate(refills):
        refill(i)
        if i == 10:
            table.sync()
        if i < 10:
            tick.launch()
            tick.wait()
        else:
            table.timing_begin()
            tick.launch()
            t_idle += table.timing_end()
    refills[0](len(refills))
    table.sync()
    table.timing_begin()
    for _ in range(queued):
        tick.launch()
    t_q = table.timing_end()
    tick.wait()
    return {"device_us": t_q * 1e3 / queued, "idle_stream_us": t_idle * 1e3 / max(len(refills) - 10, 1), "queued_ticks": queued}


def leg(args):
    """one process: the dense tick, and (--leg sweep) the sparse tick at every fill"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("tick_fill_sweep: no GPU — a device time cannot be read on a CPU")
    from rafting_amd import abi, engine, workload
    G, F = args.groups, CLUSTER - 1
    cfg = workload.config(3, G)
    gen = workload.ReplayGenerator(cfg)
    st0 = gen.initial_state()
    batches = [gen.next_batch(1) for _ in range(40)]
    cap = max(b.entry_count for b in batches) + 64
    out = {"library_sha16": engine.library_sha16(), "groups": G, "cluster": cfg.cluster}

    def table():
        t = engine.Table(G, cfg.cluster, cfg.self_slot, cfg.pre_vote)
        t.load_state(st0)
        t.timers_configure(900, 300, 1)
        t.timers_arm(0)
        return t
    kw = dict(entry_cap=cap, expired_cap=G, critical_point=1, cool_down_ms=60, device_resident=True)
    t = table()
    tk = engine.Tick2(t, 1, **kw)
    packed = [engine.pack32(b) for b in batches]
    out["dense"] = dict(readings(t, tk, [lambda i, p=p: tk.refill(p, [300 * (i + 1)]) for p in packed], args.ticks),
                        layout_bytes_per_tick=G * (row_bytes(F) - 4))
    tk.close()
    t.close()
    if args.leg == "sweep":
        out["sparse"] = []
        rng = np.random.default_rng(2024)
        for fill in FILLS:
            t = table()
            tk = engine.Tick2(t, 1, sparse_cap=G, **kw)
            subs = []
            for b in batches:
                rows = np.arange(G) if fill >= 1.0 else np.sort(rng.choice(G, int(round(fill * G)), replace=False))
                s = abi.Batch(1, len(rows), gid=rows.astype(np.uint32))
                s.head[:], s.ab[:], s.cd[:] = b.head[rows], b.ab[rows], b.cd[rows]
                s.entry_terms, s.entry_count = b.entry_terms, b.entry_count
                subs.append(engine.pack32(s))
            n = subs[0].count
            r = readings(t, tk, [lambda i, p=p: tk.refill(p, [300 * (i + 1)]) for p in subs], args.ticks)
            out["sparse"].append(dict(r, fill=fill, rows=n, layout_bytes_per_tick=n * row_bytes(F) + 8 * G, int64_body_workgroups=t.wide_body_workgroups()))
            tk.close()
            t.close()
    print("TICK_FILL_SWEEP " + json.dumps(out))


def child(args, which, lib=None):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("RG_LIB", None)
    if lib:
        env["RG_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--groups", str(args.groups), "--ticks", str(args.ticks)],
                       env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("TICK_FILL_SWEEP ")]
    if p.returncode != 0 or not lines:
        sys.exit("tick_fill_sweep: leg %s failed (%d): %s" % (which, p.returncode, (p.stdout + p.stderr)[-2000:]))
    return json.loads(lines[0][len("TICK_FILL_SWEEP "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=2000, help="queued replays per device_us reading")
    ap.add_argument("--parent-lib", default=None, help="a build of libraftgpu.so from the parent commit: its dense tick, alternated with this build's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tick_fill_sweep.json"))
    ap.add_argument("--leg", default=None, choices=("dense", "sweep"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    if not os.path.exists("/dev/kfd"):
        sys.exit("tick_fill_sweep: no GPU — a device time cannot be read on a CPU")
    doc = {"what": "recorded tick, every column device-resident; device_us = queued-tick device time, idle_stream_us = one replay on an idle stream, "
                   "layout_bytes_per_tick = computed from shapes (not measured)", "fills": list(FILLS)}
    if args.parent_lib:
        ab = {"parent": [], "new": []}
        for _ in range(3):
            ab["parent"].append(child(args, "dense", args.parent_lib)["dense"])
            ab["new"].append(child(args, "dense")["dense"])
        spread = lambda xs: max(x["device_us"] for x in xs) - min(x["device_us"] for x in xs)   # noqa: E731
        doc["dense_tick_parent_vs_new"] = dict(ab, parent_spread_device_us=spread(ab["parent"]), new_spread_device_us=spread(ab["new"]))
    doc.update(child(args, "sweep"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
