"""What RG_OPT_AUTO_INDEX_BASE costs a launch: config 3's mix for long-lived groups (every log compacted at 2^40; bench.py's long-lived leg) with LOG_FLUSH
rows put on about 1 % of the groups of every launch, timed over 20 launches with the option on (W = 2^28) and, on the same absolute rows, with the option
off (host-set bases). The bases start a window and a little more below the epochs (2^40 - 2^28 - 1000), so the first flush of a group MOVES its base in the
option's leg (to 2^40 - 2^28: a base write in that launch, rows relative to the moved base from the next launch on, as a host's mirror packs them); each leg
packs the rows against its own bases. The flush rows compact the group at its current epoch (RaftLog.flush(epoch.index, epoch.term)) in place of the group's
row of the launch's last round — the rows that follow for that group were generated without the replaced one, so those ~1 % of groups take the slow paths
more often, in both legs alike. Prints one JSON line: ms per launch, 64-bit-body workgroups and bases moved of each leg.
    python tools/auto_base_cost.py [--groups 65536] [--rounds 64] [--launches 20]"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rafting_amd import abi, engine, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--share", type=float, default=0.01)
    args = ap.parse_args()
    OFF, W = 1 << 40, 1 << 28
    cfg = dataclasses.replace(workload.config(3, args.groups), index_base=OFF, name="config3 at 2^40 with LOG_FLUSH rows")
    gen = workload.ReplayGenerator(cfg)
    st0 = gen.initial_state()
    base = np.full(args.groups, OFF - W - 1000, dtype=np.int64)
    rng = np.random.default_rng(5)
    batches, flush_rows = [], 0
    for _ in range(args.launches + 2):
        b = gen.next_batch(args.rounds)
        pick = np.flatnonzero(rng.random(args.groups) < args.share)
        rows = (args.rounds - 1) * args.groups + pick        # the group's row of the launch's last round (config 3 has no idle rounds) becomes the flush
        b.head["hdr"][rows] = abi.hdr_make(abi.EV_LOG_FLUSH)
        b.head["aux"][rows] = 0
        b.ab["x"][rows], b.ab["y"][rows] = st0.epoch_index[pick], st0.epoch_term[pick]
        b.cd["x"][rows], b.cd["y"][rows] = 0, 0
        flush_rows += len(pick)
        batches.append(b)
    out = {"config": cfg.name, "groups": args.groups, "rounds": args.rounds, "launches": args.launches, "window": W,
           "flush_rows_per_launch": flush_rows / (args.launches + 2)}
    for leg, window in (("host_set_bases", 0), ("auto_index_base", W)):
        t = engine.Table(args.groups, cfg.cluster, cfg.self_slot, cfg.pre_vote)
        t.set_index_base(base)
        if window:
            t.set_auto_index_base(window)
        t.load_state(st0)
        mirror, dbs = base.copy(), []
        for b in batches:                                   # the host's mirror: the bases each launch starts with
            b32 = engine.pack32(b, index_base=mirror)
            dbs.append(engine.DeviceBatch32(t, b32, compact=True, wide=False))
            if window:
                engine.advance_index_base(b32, mirror, window)
        for i in range(2):
            t.submit_device(dbs[i])
        t.sync()
        t.wide_body_workgroups(reset=True)
        t.timing_begin()
        for i in range(2, len(dbs)):
            t.submit_device(dbs[i])
        ms = t.timing_end()
        t.sync()
        out[leg] = {"ms_per_launch": ms / args.launches, "int64_body_workgroups": t.wide_body_workgroups(),
                    "bases_moved": int(np.count_nonzero(t.index_base() != base)), "bases_equal_mirror": bool(np.array_equal(t.index_base(), mirror))}
        for db in dbs:
            db.free()
        t.close()
    out["auto_over_host_set"] = out["auto_index_base"]["ms_per_launch"] / out["host_set_bases"]["ms_per_launch"] - 1.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
