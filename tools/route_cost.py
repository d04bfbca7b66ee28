"""What rg_route32(RG_MEM_DEVICE) costs on the device, at the points of tools/assemble_cost.py: an arrival log of m events — m = 1 %, 10 % and 100 % of the
table's groups, spread over m / 2 distinct groups of depth 1 .. 3 — assembled into a [3][groups] batch at 65 536 and 1 048 576 groups, with and without a second
source of fired tickets (1 % of the groups). The batch is assembled once; its cells get outcome rows with RG_F_PERSIST on 10 % and RG_NEED_HOST on 1 % of them and a
send table (4 followers) in which a fifth of the rows send to every follower. Every column is device-resident; `runs` routes are queued back to back on the table's
stream inside ONE rg_timing_begin / rg_timing_end region after a warm-up, so the reading is what the device spends per run (eight launches), not what a host that
waits for each run sees. `bytes_per_run` is the logical traffic of a run: what its kernels load and store, counted per element (the per-wavefront count arrays
of the shape's span included), not per cache line. One JSON line per point, appended to --out. Needs an MI355X: there is no CPU reading of a device time.
    python tools/route_cost.py [--runs 200] [--out profiles/route_cost.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rafting_amd import abi, engine  # noqa: E402

DEPTH, P = 3, 5
SENT = (abi.SEND_APPEND, abi.SEND_SNAPSHOT, abi.SEND_NEED_HOST)


def point(t, asm, G, share, with_expired, runs, rng):
    F = P - 1
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
    cells = DEPTH * G
    row, send = np.zeros(cells, abi.OUT32_DT), np.zeros(F * G, abi.SEND_DT)
    row["commit_index"] = np.arange(cells)
    row["flags"] = (rng.random(cells) < 0.1) * np.uint32(abi.F_PERSIST) | ((rng.random(cells) < 0.01) * np.uint32(abi.NEED_HOST) << np.uint32(abi.F_STATUS_SHIFT))
    send["kind"] = np.tile((rng.random(G) < 0.2) * np.uint32(abi.SEND_APPEND), F)
    cols = dict(gid=up(np.zeros(G, np.uint32)), count=up(np.zeros(1, np.uint32)), rounds=up(np.zeros(1, np.uint32)), head=up(np.zeros(cells, abi.HEAD_DT)),
                abcd=up(np.zeros(cells, abi.QUAD32_DT)), origin=up(np.zeros(cells, np.uint32)), deferred=up(np.zeros(m + e, np.uint32)), stats=up(np.zeros(4, np.uint32)),
                row=up(row), persist32=up(np.zeros(cells, abi.PERSIST32_DT)), send_head=up(np.zeros(G, abi.SEND_HEAD_DT)), send=up(send))
    b = abi.CAssembled()
    b.capacity, b.max_rounds, b.deferred_capacity = G, DEPTH, m + e
    for k in ("gid", "count", "rounds", "head", "abcd", "origin", "deferred", "stats"):
        setattr(b, k, cols[k].ptr)
    asm.run_device(a, b)
    d = abi.CDecided()
    d.capacity, d.max_rounds = G, DEPTH
    for k in ("gid", "count", "rounds", "origin", "row", "persist32", "send_head", "send"):
        setattr(d, k, cols[k].ptr)
    outs = dict(cell=up(np.zeros(m, np.uint32)), row=up(np.zeros(m, abi.OUT32_DT)), persist32=up(np.zeros(m, abi.PERSIST32_DT)),
                persist_list=up(np.zeros(cells, abi.ROUTE_ITEM_DT)), attention=up(np.zeros(cells, abi.ROUTE_ITEM_DT)), send_list=up(np.zeros(F * G, abi.SEND_ITEM_DT)),
                send_offset=up(np.zeros(P, np.uint32)), counts=up(np.zeros(4, np.uint32)))
    if e:
        outs.update(expired_cell=up(np.zeros(e, np.uint32)), expired_row=up(np.zeros(e, abi.OUT32_DT)), expired_persist32=up(np.zeros(e, abi.PERSIST32_DT)))
    r = abi.CRouted()
    r.arrival_capacity, r.expired_capacity, r.persist_capacity, r.attention_capacity, r.send_capacity = m, e, cells, cells, F * G
    for k, v in outs.items():
        setattr(r, k, v.ptr)
    for _ in range(3):
        asm.route_device(d, r)
    t.sync()
    t.timing_begin()
    for _ in range(runs):
        asm.route_device(d, r)
    ms = t.timing_end()
    t.sync()
    n, R = int(cols["count"].to_host(np.uint32, 1)[0]), int(cols["rounds"].to_host(np.uint32, 1)[0])
    counts = outs["counts"].to_host(np.uint32, 4)
    placed = int(np.count_nonzero(outs["cell"].to_host(np.uint32, m) != abi.ROUTE_NONE)) + (int(np.count_nonzero(outs["expired_cell"].to_host(np.uint32, e) != abi.ROUTE_NONE)) if e else 0)
    routed_persist = int(np.count_nonzero((row["flags"].reshape(DEPTH, G)[:R, :n] & abi.F_PERSIST)[cols["origin"].to_host(np.uint32, cells).reshape(DEPTH, G)[:R, :n] != abi.ORIGIN_NONE]))
    span = 64                                                                  # rg_route.hpp: route_span — a count word per wavefront, a wavefront per `span` rows
    while span < 4096 and max(DEPTH, F) * ((G + 4 * span - 1) // (4 * span)) * 4 > 4096:
        span *= 2
    waves, send_waves = DEPTH * ((G + 4 * span - 1) // (4 * span)) * 4, F * ((G + 4 * span - 1) // (4 * span)) * 4
    moved = ((m + e) * 4                                                        # the fill
             + R * n * (4 + 16) + placed * (4 + 16) + routed_persist * 32 + waves * 8      # the scatter and its counts
             + 2 * waves * 12                                                   # the two prefix sums (two reads and a write per word)
             + R * n * 4 + (int(counts[0]) + int(counts[1])) * (4 + 8) + waves * 8         # the emit
             + 2 * F * n * 4 + send_waves * (4 + 12 + 4) + int(counts[2]) * (4 + 8))       # the send list
    res = {"groups": G, "events": m, "share": share, "expired_entries": e, "depth_mix": "1..%d" % DEPTH, "capacity": G, "max_rounds": DEPTH, "cluster": P, "runs": runs,
           "span": span, "us_per_run": ms * 1e3 / runs, "bytes_per_run": int(moved), "rows": n, "rounds": R, "placed": placed, "persist_items": int(counts[0]),
           "attention_items": int(counts[1]), "send_items": int(counts[2]), "library_sha16": engine.library_sha16()}
    for x in bufs + list(cols.values()) + list(outs.values()):
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "route_cost.jsonl"))
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("route_cost: no GPU — a device time cannot be read on a CPU")
    rng = np.random.default_rng(2025)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for G in (65536, 1048576):
            t = engine.Table(G, P)
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
