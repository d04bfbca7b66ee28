"""What rg_assemble32(RG_MEM_DEVICE) costs on the device: an arrival log of m events — m = 1 %, 10 % and 100 % of the table's groups, spread over m / 2 distinct
groups of depth 1 .. 3 (seeded, shuffled: arrival order) — assembled into a [3][groups] batch at 65 536 and 1 048 576 groups, with and without a second source
of fired tickets (1 % of the groups). Every column is device-resident; `runs` runs are queued back to back on the table's stream inside ONE rg_timing_begin /
rg_timing_end region after a warm-up, so the reading is what the device spends per run (ten launches), not what a host that waits for each run sees. One JSON
line per point, appended to --out. Needs an MI355X: there is no CPU reading of a device time.
    python tools/assemble_cost.py [--runs 200] [--out profiles/assemble_cost.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rafting_amd import abi, engine  # noqa: E402

DEPTH = 3


def point(t, asm, G, share, with_expired, runs, rng):
    m = max(int(round(share * G)), 1)
    groups = rng.choice(G, max(m // 2, 1), replace=False)
    gid = np.repeat(groups, rng.integers(1, DEPTH + 1, len(groups)))
    gid = np.resize(gid, m)[rng.permutation(m)].astype(np.uint32)
    head, abcd = np.zeros(m, abi.HEAD_DT), np.zeros(m, abi.QUAD32_DT)
    head["hdr"], abcd["a"] = abi.hdr_make(abi.EV_IS_REQ), np.arange(m)
    e = max(G // 100, 1) if with_expired else 0
    up = lambda a: engine.DeviceBuffer.from_host(t, a)      # noqa: E731
    bufs = [up(np.array([m], np.uint32)), up(gid), up(head), up(abcd)]
    a = abi.CArrivals()
    a.count, a.capacity, a.gid, a.head, a.abcd = bufs[0].ptr, m, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr
    if e:
        bufs += [up(np.sort(rng.choice(G, e, replace=False)).astype(np.uint32)), up(np.ones(e, np.uint32)), up(np.array([e], np.uint32))]
        a.expired_gid, a.expired_epoch, a.expired_count, a.expired_capacity = bufs[4].ptr, bufs[5].ptr, bufs[6].ptr, e
    outs = dict(gid=up(np.zeros(G, np.uint32)), count=up(np.zeros(1, np.uint32)), rounds=up(np.zeros(1, np.uint32)), head=up(np.zeros(DEPTH * G, abi.HEAD_DT)),
                abcd=up(np.zeros(DEPTH * G, abi.QUAD32_DT)), origin=up(np.zeros(DEPTH * G, np.uint32)), deferred=up(np.zeros(m + e, np.uint32)),
                stats=up(np.zeros(4, np.uint32)))
    b = abi.CAssembled()
    b.capacity, b.max_rounds, b.deferred_capacity = G, DEPTH, m + e
    for k, v in outs.items():
        setattr(b, k, v.ptr)
    for _ in range(3):
        asm.run_device(a, b)
    t.sync()
    t.timing_begin()
    for _ in range(runs):
        asm.run_device(a, b)
    ms = t.timing_end()
    t.sync()
    stats = outs["stats"].to_host(np.uint32, 4)
    res = {"groups": G, "events": m, "share": share, "expired_entries": e, "depth_mix": "1..%d" % DEPTH, "capacity": G, "max_rounds": DEPTH, "runs": runs,
           "us_per_run": ms * 1e3 / runs, "events_per_s": (m + e) * runs / (ms * 1e-3), "rows": int(outs["count"].to_host(np.uint32, 1)[0]),
           "rounds": int(outs["rounds"].to_host(np.uint32, 1)[0]), "placed": int(stats[0]), "deferred": int(stats[1]), "library_sha16": engine.library_sha16()}
    for x in bufs + list(outs.values()):
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "assemble_cost.jsonl"))
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("assemble_cost: no GPU — a device time cannot be read on a CPU")
    rng = np.random.default_rng(2025)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for G in (65536, 1048576):
            t = engine.Table(G, 5)
            asm = engine.Assembler(t, G, max_expired=max(G // 100, 1))
            for share in (0.01, 0.1, 1.0):
                for with_expired in (False, True):
                    line = json.dumps(point(t, asm, G, share, with_expired, args.runs, rng))
                    print(line)
                    f.write(line + "\n")
                    f.flush()
            asm.close()
            t.close()


if __name__ == "__main__":
    main()
