"""What the carry of an assembler costs on the device, in the form and at the points of tools/assemble_cost.py: 65 536 and 1 048 576 groups, an arrival log of
groups / 2 events at capacity = groups, max_rounds = 2, every column device-resident, `runs` runs queued back to back on the table's stream inside ONE
rg_timing_begin / rg_timing_end region after a warm-up. Per point, microseconds per run of rg_assemble32 and of rg_route32_carry in three situations —
    empty      the carry on, nothing ever deferred: every group of the log has one event
    1 %, 10 %  that share of the log's events is deferred per run, in STEADY STATE: d hot groups get max_rounds events per run and have one in the carry, so
               every run reads d carried slots, places them and one of each hot group's arrivals, and defers d again (one priming run with a third event per hot
               group starts it)
— and, beside each, the plain calls in the same process on a second assembler of the same table: rg_assemble32 over the log the header's host recipe would have
built (the d carried rows prepended by hand: the same batch) and rg_route32. One JSON line per point, appended to --out. Needs an MI355X.
    python tools/carry_cost.py [--runs 200] [--out profiles/carry_cost.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rafting_amd import abi, engine  # noqa: E402

DEPTH, P = 2, 5


def timed(t, runs, call):
    for _ in range(3):
        call()
    t.sync()
    t.timing_begin()
    for _ in range(runs):
        call()
    ms = t.timing_end()
    t.sync()
    return ms * 1e3 / runs


def point(t, G, share, runs, rng):
    m = G // 2
    d = int(round(share * m))
    order = rng.permutation(G)
    hot, cold = order[:d], order[d: d + m - DEPTH * d]
    log = np.concatenate([np.repeat(hot, DEPTH), cold])
    log = log[rng.permutation(len(log))]
    gid = np.concatenate([log, hot]).astype(np.uint32)                   # [m] the steady log, [m, m + d) the third events of the priming run
    by_hand = np.concatenate([hot, log]).astype(np.uint32)               # the plain assembler's log: the d carried rows first
    head, abcd = np.zeros(m + d, abi.HEAD_DT), np.zeros(m + d, abi.QUAD32_DT)
    head["hdr"], abcd["a"] = abi.hdr_make(abi.EV_IS_REQ), np.arange(m + d)
    cells, F = DEPTH * G, P - 1
    up = lambda a: engine.DeviceBuffer.from_host(t, a)      # noqa: E731
    bufs = dict(prime=up(np.array([m + d], np.uint32)), steady=up(np.array([m], np.uint32)), gid=up(gid), by_hand=up(by_hand), head=up(head), abcd=up(abcd))
    row = np.zeros(cells, abi.OUT32_DT)
    row["commit_index"] = np.arange(cells)
    row["flags"] = (rng.random(cells) < 0.1) * np.uint32(abi.F_PERSIST)
    cols = dict(gid=up(np.zeros(G, np.uint32)), count=up(np.zeros(1, np.uint32)), rounds=up(np.zeros(1, np.uint32)), head=up(np.zeros(cells, abi.HEAD_DT)),
                abcd=up(np.zeros(cells, abi.QUAD32_DT)), origin=up(np.zeros(cells, np.uint32)), deferred=up(np.zeros(m + d, np.uint32)), stats=up(np.zeros(4, np.uint32)),
                row=up(row), persist32=up(np.zeros(cells, abi.PERSIST32_DT)))
    outs = dict(cell=up(np.zeros(m + d, np.uint32)), row=up(np.zeros(m + d, abi.OUT32_DT)), persist32=up(np.zeros(m + d, abi.PERSIST32_DT)),
                persist_list=up(np.zeros(cells, abi.ROUTE_ITEM_DT)), attention=up(np.zeros(cells, abi.ROUTE_ITEM_DT)), counts=up(np.zeros(4, np.uint32)))
    K = max(G // 8, 1)
    couts = dict(cell=up(np.zeros(K, np.uint32)), row=up(np.zeros(K, abi.OUT32_DT)), persist32=up(np.zeros(K, abi.PERSIST32_DT)))

    def arrivals(count, log_gid):
        a = abi.CArrivals()
        a.count, a.capacity, a.gid, a.head, a.abcd = bufs[count].ptr, m + d, bufs[log_gid].ptr, bufs["head"].ptr, bufs["abcd"].ptr
        return a
    b = abi.CAssembled()
    b.capacity, b.max_rounds, b.deferred_capacity = G, DEPTH, m + d
    for k in ("gid", "count", "rounds", "head", "abcd", "origin", "deferred", "stats"):
        setattr(b, k, cols[k].ptr)
    dd = abi.CDecided()
    dd.capacity, dd.max_rounds = G, DEPTH
    for k in ("gid", "count", "rounds", "origin", "row", "persist32"):
        setattr(dd, k, cols[k].ptr)
    r = abi.CRouted()
    r.arrival_capacity, r.persist_capacity, r.attention_capacity = m + d, cells, cells
    for k, v in outs.items():
        setattr(r, k, v.ptr)
    rc = abi.CRoutedCarry()
    rc.capacity, rc.cell, rc.row, rc.persist32 = K, couts["cell"].ptr, couts["row"].ptr, couts["persist32"].ptr
    res = {"groups": G, "events": m, "deferred_share": share, "capacity": G, "max_rounds": DEPTH, "carry_capacity": K, "runs": runs, "library_sha16": engine.library_sha16()}
    # the carrying assembler: one priming run, then the steady log
    asm = engine.Assembler(t, m + d, carry=K)
    asm.run_device(arrivals("prime", "gid"), b)
    steady = arrivals("steady", "gid")
    res["carry_assemble_us"] = timed(t, runs, lambda: asm.run_device(steady, b))
    stats = cols["stats"].to_host(np.uint32, 4)
    res.update(carried_slots_read=len(asm.carry_read(abi.CARRY_LAST)[0]), deferred=int(stats[1]), spilled=int(stats[3]), placed=int(stats[0]))
    assert res["carried_slots_read"] == d and res["deferred"] == d and res["spilled"] == 0, res
    res["carry_route_us"] = timed(t, runs, lambda: asm.route_device(dd, r, carried=rc))
    asm.close()
    # the plain calls beside it: the same batch from a log with the carried rows prepended by hand
    plain = engine.Assembler(t, m + d)
    hand = arrivals("prime", "by_hand")
    res["plain_assemble_us"] = timed(t, runs, lambda: plain.run_device(hand, b))
    assert int(cols["stats"].to_host(np.uint32, 4)[1]) == d
    res["plain_route_us"] = timed(t, runs, lambda: plain.route_device(dd, r))
    plain.close()
    for x in list(bufs.values()) + list(cols.values()) + list(outs.values()) + list(couts.values()):
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "carry_cost.jsonl"))
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("carry_cost: no GPU — a device time cannot be read on a CPU")
    rng = np.random.default_rng(2025)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for G in (65536, 1048576):
            t = engine.Table(G, P)
            for share in (0.0, 0.01, 0.1):
                line = json.dumps(point(t, G, share, args.runs, rng))
                print(line)
                f.write(line + "\n")
                f.flush()
            t.close()


if __name__ == "__main__":
    main()
