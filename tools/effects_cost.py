"""What rg_effects32(RG_MEM_DEVICE) costs behind a launch, against what a host pays today for the same answer, at two shapes:
  bench:  65 536 groups x 5 nodes x 64 rounds, the rows rg_submit32c leaves of bench.py's config-3 stream (dense: gid NULL, C = 65 536, D = 64);
  sparse: 1 % of 1 048 576 groups x 5 nodes, depth 4, the rows rg_submit32c_sparse_rounds leaves of the same mix (config 4) for a list of groups (C = n, D = 4).
The launch runs once; its rows stay in device memory. Then three legs ALTERNATE, `reps` times:
  device   `runs` calls queued back to back on the table's stream inside ONE rg_timing_begin / rg_timing_end region: what the device spends per call (five launches);
  lists    one call, one wait, then the counts and the written items of the three lists copied down: what a host waits for before its threads can act (wall clock);
  host     what a host does for the same answer without the call: rg_copy_to_host of every row into page-locked memory, then one single-threaded numpy pass over
           the flags for the three selections (the log writes in cell order, the last commit of every group, the RG_NEED_HOST cells) (wall clock).
The floor is one pass over `row` — D x C x 16 bytes — at the figure rg_copy_bandwidth gives on the same table. The call reads the flags of the rows in TWO passes
(count, emit), each over the cell domain and the row domain (rg_effects.hpp): four reads of the rows per call; the floor is quoted for one. Medians over the
repetitions, with the smallest and largest reading beside them. One JSON line per shape, appended to --out. Needs an MI355X: there is no CPU reading of a device time.
    python tools/effects_cost.py [--runs 100] [--reps 7] [--out profiles/effects_cost.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rafting_amd import abi, engine, workload  # noqa: E402

LOG = abi.F_LOG_APPEND | abi.F_LOG_TRUNC


def host_scan(row, Cc, D):
    """the three answers from every row, single-threaded numpy -> their item counts"""
    flags = row["flags"]
    log = np.flatnonzero(flags & LOG)
    attention = np.flatnonzero((flags >> abi.F_STATUS_SHIFT) & 0xFF == abi.NEED_HOST)
    com = ((flags & abi.F_COMMIT) != 0).reshape(D, Cc)
    groups = np.flatnonzero(com.any(axis=0))
    last = D - 1 - np.argmax(com[::-1, groups], axis=0)
    commit_index = row["commit_index"].reshape(D, Cc)[last, groups]
    return len(log), len(commit_index), len(attention)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def measure(name, t, row_buf, Cc, D, gid_buf, runs, reps, gbps):
    """row_buf: the launch's rows [D][Cc] in device memory; gid_buf: its gid list there, or None"""
    L = engine.lib()
    cells = Cc * D
    up = lambda a: engine.DeviceBuffer.from_host(t, a)      # noqa: E731
    outs = dict(log_list=up(np.zeros(cells, abi.ROUTE_ITEM_DT)), commit_list=up(np.zeros(Cc, abi.COMMIT_ITEM_DT)), attention=up(np.zeros(cells, abi.ROUTE_ITEM_DT)),
                counts=up(np.zeros(4, np.uint32)))
    e, o = abi.CEffectsIn(), abi.CEffects()
    e.capacity, e.max_rounds, e.gid, e.row = Cc, D, (gid_buf.ptr if gid_buf else None), row_buf.ptr
    o.log_capacity, o.commit_capacity, o.attention_capacity = cells, Cc, cells
    for k, v in outs.items():
        setattr(o, k, v.ptr)
    down, pin = engine.pinned_like(t, np.zeros(cells, abi.OUT32_DT))
    lists = {k: engine.pinned_like(t, np.zeros(n, dt)) for k, (dt, n) in dict(log_list=(abi.ROUTE_ITEM_DT, cells), commit_list=(abi.COMMIT_ITEM_DT, Cc),
                                                                             attention=(abi.ROUTE_ITEM_DT, cells), counts=(np.uint32, 4)).items()}
    for _ in range(3):                                          # warm-up: the scratch of the shape, the code objects
        t.effects_device(e, o)
    t.sync()
    host_scan(down, Cc, D)
    device_us, lists_us, host_copy_us, host_scan_us = [], [], [], []
    counts = found = None
    for _ in range(reps):
        t.timing_begin()
        for _ in range(runs):
            t.effects_device(e, o)
        device_us.append(t.timing_end() * 1e3 / runs)
        t0 = time.perf_counter()
        t.effects_device(e, o)
        t.sync()
        t._check(L.rg_copy_to_host(t._h, lists["counts"][0].ctypes.data, outs["counts"].ptr, 16))
        counts = [int(c) for c in lists["counts"][0]]
        for k, c in zip(("log_list", "commit_list", "attention"), counts):
            if c:
                t._check(L.rg_copy_to_host(t._h, lists[k][0].ctypes.data, outs[k].ptr, c * lists[k][0].dtype.itemsize))
        lists_us.append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        t._check(L.rg_copy_to_host(t._h, down.ctypes.data, row_buf.ptr, down.nbytes))
        t1 = time.perf_counter()
        found = host_scan(down, Cc, D)
        t2 = time.perf_counter()
        host_copy_us.append((t1 - t0) * 1e6)
        host_scan_us.append((t2 - t1) * 1e6)
    assert list(found) == counts[:3], (found, counts)            # the two ways give the same answer
    host_us = [a + b for a, b in zip(host_copy_us, host_scan_us)]
    floor_us = cells * 16 / (gbps * 1e9) * 1e6
    res = {"shape": name, "capacity": Cc, "max_rounds": D, "cells": cells, "row_bytes": cells * 16, "gid_list": gid_buf is not None, "runs": runs, "reps": reps,
           "log_items": counts[0], "commit_items": counts[1], "attention_items": counts[2],
           "device_us_per_call": spread(device_us), "call_wait_and_lists_down_us": spread(lists_us), "host_copy_rows_us": spread(host_copy_us),
           "host_numpy_scan_us": spread(host_scan_us), "host_total_us": spread(host_us), "copy_bandwidth_gbps": gbps, "floor_one_pass_us": floor_us,
           "passes_over_row_per_call": 4, "device_over_floor": spread(device_us)["median"] / floor_us,
           "host_over_device": spread(host_us)["median"] / spread(device_us)["median"], "host_over_lists_down": spread(host_us)["median"] / spread(lists_us)["median"],
           "library_sha16": engine.library_sha16()}
    pin.free()
    for a, p in lists.values():
        p.free()
    for x in outs.values():
        x.free()
    return res


def bench_shape(runs, reps):
    cfg = workload.config(3)
    gen = workload.ReplayGenerator(cfg)
    t = engine.Table(cfg.groups, cfg.cluster, cfg.self_slot, cfg.pre_vote)
    t.load_state(gen.initial_state())
    db = engine.DeviceBatch32(t, gen.next_batch(64), compact=True, wide=False)
    t.submit_device(db)
    t.sync()
    gbps = t.copy_bandwidth()
    res = measure("bench: 65536 x 5 nodes x 64 rounds, config 3, dense", t, db.row32, cfg.groups, 64, None, runs, reps, gbps)
    db.free()
    t.close()
    return res


def sparse_shape(runs, reps, D=4):
    cfg = workload.config(4)
    gen = workload.ReplayGenerator(cfg)
    t = engine.Table(cfg.groups, cfg.cluster, cfg.self_slot, cfg.pre_vote)
    t.load_state(gen.initial_state())
    dense = gen.next_batch(D)
    G = cfg.groups
    rows = np.flatnonzero(np.random.default_rng(2025).random(G) < 0.01)
    n = len(rows)
    sub = abi.Batch(D, n, gid=rows.astype(np.uint32))
    for name in ("head", "ab", "cd"):
        getattr(sub, name)[:] = getattr(dense, name).reshape(D, G)[:, rows].reshape(-1)
    sub.entry_terms, sub.entry_count = dense.entry_terms, dense.entry_count
    db = engine.DeviceBatch32(t, sub, compact=True, wide=False)
    t._check(engine.lib().rg_submit32c_sparse_rounds(t._h, C.byref(db.c_batch), C.byref(db.c_out), abi.MEM_DEVICE))
    t.sync()
    gbps = t.copy_bandwidth()
    res = measure("sparse: 1 %% of 1048576 x 5 nodes, depth %d, config 4, a list of groups" % D, t, db.row32, n, D, db.gid, runs, reps, gbps)
    db.free()
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "effects_cost.jsonl"))
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("effects_cost: no GPU — a device time cannot be read on a CPU")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for shape in (bench_shape, sparse_shape):
            line = json.dumps(shape(args.runs, args.reps))
            print(line)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
