"""A stream of long-lived groups for RG_OPT_AUTO_INDEX_BASE (include/raftgpu.h, "automatic bases"): groups that start with their logs compacted near
2^40 and are carried forward, launch after launch, by RG_EV_LOG_FLUSH rows — wipes beyond `last` that jump the epoch by up to 2^29 (a snapshot install)
and trims inside the log (a compaction) — mixed with election traffic (timeouts, RequestVote / PreVote from peers at the same or the next term). Each
batch is built from the oracle's state before it, in absolute values; its index fields stay within the window of the automatic bases, so that a host
which packs relative to a mirror of the bases never holds a row back. Used by tests/devemu/emu_cases_auto_base.py and tests/test_auto_index_base_gpu.py."""
import numpy as np

from rafting_amd import abi

OFFSET = 1 << 40
WINDOW = 1 << 28                      # the recommended window
IDX_FIELDS = np.array([0, 0xA, 0x6, 0x2, 0x2, 0x2, 0, 0, 0, 0, 0x1, 0x2, 0, 0, 0, 0], dtype=np.uint32)      # rg_device.hpp: index_fields


def start_state(G, P, self_slot, seed):
    """fuzz.random_initial_state at 2^40, and the bases a host would set once at start (a little below every epoch)"""
    from tests import fuzz
    st = fuzz.random_initial_state(G, P, self_slot, seed, offset=OFFSET)
    return st, np.full(G, OFFSET - 1000, dtype=np.int64)


def _newest(st, g):
    """(last index, its term) of group g's log, or the epoch when the log is empty"""
    rc = int(st.run_count[g])
    if rc == 0:
        return int(st.epoch_index[g]), int(st.epoch_term[g])
    off = int(st.run_offset[g])
    return int(st.last_index[g]), int(st.run_term[off + min(rc, abi.TERM_RUNS) - 1])


def next_batch(st, rng, P, self_slot, wipe=0.25, trim=0.1, jump=(1 << 28, 1 << 29), idle=0.3):
    """one dense round for every group of `st` (the oracle's state before it)"""
    G = len(st.role)
    b = abi.Batch(1, G)
    peers = [s for s in range(P) if s != self_slot]
    for g in range(G):
        x = rng.random()
        last, last_term = _newest(st, g)
        term = int(st.current_term[g])
        if x < wipe and st.role[g] != abi.LEADER:
            a = max(last, int(st.epoch_index[g])) + int(rng.integers(jump[0], jump[1] + 1))
            b.head["hdr"][g] = abi.hdr_make(abi.EV_LOG_FLUSH)
            b.ab["x"][g], b.ab["y"][g] = a, max(term, 1)
        elif x < wipe + trim and st.run_count[g] > 0 and last > st.epoch_index[g]:
            b.head["hdr"][g] = abi.hdr_make(abi.EV_LOG_FLUSH)
            b.ab["x"][g], b.ab["y"][g] = last, last_term
        elif x < 1.0 - idle:
            y = rng.random()
            if y < 0.4:
                b.head["hdr"][g] = abi.hdr_make(abi.EV_TIMEOUT)
            else:
                kind = abi.EV_RV_REQ if y < 0.75 else abi.EV_PV_REQ
                t = term + int(rng.integers(0, 2))
                b.head["hdr"][g] = abi.hdr_make(kind, slot=int(rng.choice(peers)))
                b.ab["x"][g], b.ab["y"][g] = t, last
                b.cd["x"][g] = min(last_term, t)
    return b


def refresh_batch(st, wiped, P, self_slot, rng):
    """the round after a wipe: what the group's leader sends next — AppendEntries at the new epoch with one entry of its term and leaderCommit on it.
    (RaftLog.flush moves the epoch only: commitIndex and the emptied log's bounds stay behind. Left there, they would lie below a base that moved by
    more than the window, and the group would leave the 32-bit image — correctly, but not what a cluster in operation looks like.)"""
    G = len(st.role)
    b = abi.Batch(1, G)
    b.entry_terms = np.zeros(G, dtype=np.int64)
    b.entry_count = G
    peers = [s for s in range(P) if s != self_slot]
    for g in np.flatnonzero(wiped):
        if st.role[g] == abi.LEADER:
            continue
        term = int(st.current_term[g])
        lead = int(st.current_leader[g])
        slot = lead if lead != abi.NO_NODE else int(rng.choice(peers))
        ei = int(st.epoch_index[g])
        b.head["hdr"][g] = abi.hdr_make(abi.EV_AE_REQ, slot=slot, n=1)
        b.head["aux"][g] = g
        b.entry_terms[g] = term
        b.ab["x"][g], b.ab["y"][g] = term, ei
        b.cd["x"][g], b.cd["y"][g] = int(st.epoch_term[g]), ei + 1
    return b


def launch(orc, rng, P, self_slot, **kw):
    """one two-round launch: next_batch, then refresh_batch for the groups it wiped — built and decided round by round on the oracle `orc` (absolute
    values) -> (the two-round batch, the oracle's outcome, the state before it)"""
    from tests import fuzz
    cur = orc.read_state()
    b0 = next_batch(cur, rng, P, self_slot, **kw)
    o0 = orc.submit(b0, fill=0xAB)
    wiped = ((b0.head["hdr"] & 0xF) == abi.EV_LOG_FLUSH) & (b0.ab["x"] > orc.read_state().last_index) & (abi.flags_status(o0.reply["flags"]) == abi.OK)
    b1 = refresh_batch(orc.read_state(), wiped, P, self_slot, rng)
    o1 = orc.submit(b1, fill=0xAB)
    return fuzz.concat_batches([b0, b1]), fuzz.concat_outcomes([o0, o1]), cur


def relative(batch, base):
    """the batch with its index fields relative to `base` (per group): what a host that packs against a mirror of the bases sends. Raises when an index
    has no relative image — the stream is built so that none does."""
    kind = (batch.head["hdr"] & 0xF).astype(np.int64)
    ixf = IDX_FIELDS[kind]
    gid = np.arange(batch.count) if batch.gid is None else batch.gid.astype(np.int64)
    bb = np.tile(base[gid], batch.rounds)
    out = abi.Batch(batch.rounds, batch.count, gid=batch.gid)
    out.head[:] = batch.head
    out.entry_terms, out.entry_count = batch.entry_terms, batch.entry_count
    for k, (arr, f) in enumerate(((batch.ab, "x"), (batch.ab, "y"), (batch.cd, "x"), (batch.cd, "y"))):
        col = arr[f].astype(np.int64)
        is_ix = ((ixf >> k) & 1) != 0
        rel = np.where(is_ix & (col != 0), col - bb, col)
        assert not np.any(is_ix & (col != 0) & ((rel <= 0) | (rel >= 1 << 31))), "an index without a relative image"
        (out.ab if k < 2 else out.cd)[f] = rel
    return out


def advance(batch, base, window=WINDOW):
    """numpy restatement of the rule on wide rows (absolute a): every LOG_FLUSH row raises its group's base to max(base, a - window)"""
    kind = batch.head["hdr"] & 0xF
    gid = np.tile(np.arange(batch.count) if batch.gid is None else batch.gid.astype(np.int64), batch.rounds)
    out = base.copy()
    for row in np.flatnonzero(kind == abi.EV_LOG_FLUSH):
        out[gid[row]] = max(out[gid[row]], int(batch.ab["x"][row]) - window)
    return out
