"""Cases for the ELECTION BLOCK of the 32-bit step body (rg_tier1n.hpp: tier1n behind `(b_rare | b_el) != 0`): hand-built streams, decided by the oracle, that
enter every sub-block of that block alone and together. Shared by tests/test_election_round_gpu.py (an MI355X), tests/devemu/emu_cases_election_round.py (the
host emulation of the kernels) and tests/test_election_round_cpu.py.

WHY HAND-BUILT. The block is a chain of wave-uniform branches — {rare | election}, rare, election, vote replies, timeouts, vote requests, the conversion tail —
and what a sub-block leaves behind for the next (the predicate bits of the outcome row, the cached precondition words, the vote count) is only visible when the
sub-blocks are entered in a chosen combination: a fuzz stream of 65 groups enters nearly all of them in nearly every round. Here a round's rows are chosen so
that ONE class is alone in the wavefront, then the classes together, then an election row in the round right after a conversion of the same lane.

THE SHAPE. P nodes (5; and 3 and 7: two and six followers), self = slot 0, PreVote on, G = 65 groups — one full wavefront and a workgroup of one lane —, ROUNDS =
12 rounds in ONE launch. The cast, by group (every group has a log 1 .. 10 whose tail is of term 5; `w` = majority - 1, the grants a candidate needs):
    0, 64  Candidate (term 6, role epoch 7): RequestVote grants in rounds 0 .. w-1 (group 64: one round later) — counted, the last one wins —, then a timeout as
           the new, unprepared Leader in the round RIGHT AFTER the conversion (lead_prepare on the re-cached words)
    1      Follower after a PreVote timeout (term 5, role epoch 2): PreVote grants in rounds 1 .. w, the last converts to Candidate (term 6, role epoch 3); a
           RequestVote grant in the round right after it
    2      Leader that won at role epoch 7 (elected_epoch 7, role epoch 8): a late RequestVote reply of a HIGHER term in round 2 (late_higher: step down)
    3, 4, 5  Follower / Candidate / unprepared Leader: a STALE timeout in round 3 (dropped), a live one in round 4 (to_pre / to_candidate / lead_prepare)
    6      prepared Leader: a live timeout in round 4 (to_lead alone: timer reset, heartbeat)
    7      Follower: RequestVote of term 6 with an up-to-date log in round 5 (granted: converts), the same request again in round 6 (same term, same candidate)
    8      Follower: RequestVote of term 6 whose log is behind in round 5 (refused for log order: converts, votes for nobody)
    9      Follower after a PreVote timeout: a PreVote request of a higher term in round 5 (judged, granted, nothing persisted)
    10     prepared Leader: an ack of a HIGHER term in round 6 (ack_down)
    11     Follower: AppendEntries of a new leader (term 6) with entries of term 6 in round 0 — a new term run, the RARE sub-block — beside group 0's counted reply
    12     unprepared Leader of term 6 over a log of term 5: its FIRST client append in round 0 (rare: new run + prepareReplication), again beside group 0
    13     Candidate: a REFUSED RequestVote reply in rounds 7 and 9 (the vote-reply sub-block with nothing to count and nothing to convert), a grant in round 8
    14     prepared Leader, 15 Follower, 16 Candidate: round 8 — an ack of a higher term, a timeout, a RequestVote request (tier 1.5 decides it) — so that round 8
           has EVERY class at once with groups 13 (reply), 3 (timeout), 8 (request), 17 (rare: a new term run)
    18 .. 63  steady replication, so that the main block has work in every round: even groups are Followers that take a heartbeat with a rising leaderCommit,
           odd groups prepared Leaders that take an ack per round (and commit on the quorum)
Round 0 has ONE election row in the first wavefront (group 0's counted reply; at 3 nodes that grant wins, and group 13's refusal in round 7 is the round whose only
election row converts nothing) and none in the second; rounds 10 and 11 have none at all.

WHAT IS CHECKED. Every outcome row and persist row (rg_submit32c's compact rows, unpacked, and the rows themselves: tests/helpers.check_out32_rows), the table
afterwards, against the oracle; rg_wide_body_workgroups() == 0 (the 32-bit body is what ran); the same through rg_submit32 (wide outcome rows) and
rg_submit32c_sparse_rounds (the sparse kernel variant, every group listed); and once more with RG_FORCE_WIDE=1 — the 64-bit body on the same rows — as the
differential. reach() proves on the oracle's rows alone that the stream does what this docstring says."""
import functools
import os
import types

import numpy as np

from rafting_amd import abi, engine
from tests import oracle_lib
from tests.helpers import C, F, L, check_out32_rows, compare_outcomes, compare_states, set_group

G, ROUNDS, SELF = 65, 12, 0
CLUSTERS = (5, 3, 7)
ROUTES = ("submit32c", "submit32", "sparse_rounds")
LOG = (1, [(1, 4), (6, 5)], 10)                               # entries 1 .. 10, the newest run (6 .. 10) of term 5
STEADY = range(18, 64)


def initial_state(P):
    st = abi.GroupState(G, P)
    Fn = P - 1
    fresh = [(0, 11, 0, 0, 0)] * Fn                           # Leadership.State after prepareReplication: epoch 0, nextIndex last + 1, nothing matched
    follower = dict(role=F, term=5, voted_for=1, leader=1, log=LOG)
    candidate = dict(role=C, term=6, voted_for=SELF, role_epoch=7, log=LOG)
    prevoting = dict(role=F, term=5, voted_for=1, timeout_detected=1, role_epoch=2, log=LOG)
    leader = dict(role=L, term=5, voted_for=SELF, role_epoch=3, repl_prepared=1, log=LOG, peers=fresh)
    cast = {0: candidate, 64: candidate, 1: prevoting, 2: dict(role=L, term=6, voted_for=SELF, role_epoch=8, elected_epoch=7, elected_term=6, log=LOG),
            3: follower, 4: candidate, 5: dict(role=L, term=5, voted_for=SELF, role_epoch=3, log=LOG), 6: leader, 7: follower, 8: follower, 9: prevoting, 10: leader,
            11: follower, 12: dict(role=L, term=6, voted_for=SELF, role_epoch=4, log=LOG), 13: candidate, 14: leader, 15: follower, 16: candidate, 17: follower}
    for g in range(G):
        set_group(st, g, **cast.get(g, follower if g % 2 == 0 else leader))
    return st


def stream(P):
    """-> the abi.Batch of the launch (ROUNDS x G rows)"""
    w = P // 2                                                # majority - 1
    b = abi.Batch(ROUNDS, G)
    peer = lambda k: 1 + k % (P - 1)                          # noqa: E731  (a remote slot)
    for k in range(w):                                        # groups 0, 64: grants; the last one wins
        b.put(k, 0, abi.EV_RV_REPLY, slot=peer(k), flag=1, a=6, aux=7)
        b.put(k + 1, 64, abi.EV_RV_REPLY, slot=peer(k), flag=1, a=6, aux=7)
    b.put(w, 0, abi.EV_TIMEOUT, aux=0)                        # ... and the new Leader's first tick, in the round right after
    b.put(w + 1, 64, abi.EV_TIMEOUT, aux=8)
    for k in range(w):                                        # group 1: PreVote grants, then a RequestVote grant as the Candidate it became
        b.put(1 + k, 1, abi.EV_PV_REPLY, slot=peer(k), flag=1, a=5, aux=2)
    b.put(1 + w, 1, abi.EV_RV_REPLY, slot=peer(0), flag=1, a=6, aux=3)
    b.put(2, 2, abi.EV_RV_REPLY, slot=peer(1), flag=0, a=9, aux=7)
    for g, epoch in ((3, 1), (4, 7), (5, 3)):
        b.put(3, g, abi.EV_TIMEOUT, aux=epoch + 5)            # a ticket of another participant
        b.put(4, g, abi.EV_TIMEOUT, aux=epoch)
    b.put(4, 6, abi.EV_TIMEOUT, aux=0)
    for r in (5, 6):
        b.put(r, 7, abi.EV_RV_REQ, slot=peer(1), a=6, b=10, c=5)
    b.put(5, 8, abi.EV_RV_REQ, slot=peer(2), a=6, b=3, c=4)
    b.put(5, 9, abi.EV_PV_REQ, slot=peer(0), a=6, b=12, c=5)
    b.put(6, 10, abi.EV_AE_ACK, slot=peer(0), flag=0, a=8, b=0, c=10, aux=3)
    b.put(0, 11, abi.EV_AE_REQ, slot=peer(1), a=6, b=10, c=5, d=0, entries=[6, 6])
    b.put(0, 12, abi.EV_CLIENT_APPEND, n=2)
    b.put(7, 13, abi.EV_RV_REPLY, slot=peer(0), flag=0, a=6, aux=7)
    b.put(8, 13, abi.EV_RV_REPLY, slot=peer(1), flag=1, a=6, aux=7)
    b.put(9, 13, abi.EV_RV_REPLY, slot=peer(2), flag=0, a=6, aux=7)      # (at 3 nodes the grant of round 8 has made it Leader: a late reply, nothing to do)
    b.put(8, 14, abi.EV_AE_ACK, slot=peer(1), flag=1, a=7, b=0, c=10, aux=3)
    b.put(8, 3, abi.EV_TIMEOUT, aux=0)
    b.put(8, 15, abi.EV_TIMEOUT, aux=1)
    b.put(8, 8, abi.EV_RV_REQ, slot=peer(0), a=8, b=10, c=5)
    b.put(8, 16, abi.EV_RV_REQ, slot=peer(1), a=7, b=10, c=5)
    b.put(8, 17, abi.EV_AE_REQ, slot=peer(0), a=6, b=10, c=5, d=3, entries=[6])
    for g in STEADY:
        for r in range(ROUNDS):
            if g % 2 == 0:
                b.put(r, g, abi.EV_AE_REQ, slot=1, a=5, b=10, c=5, d=min(r + 1, 10))
            else:
                b.put(r, g, abi.EV_AE_ACK, slot=peer(r), flag=1, a=5, b=0, c=10, aux=3)
    assert abi.batch_fits_32(b)
    return b


@functools.lru_cache(maxsize=None)
def lead(P):
    """the oracle's half, once per cluster size: the initial state, the stream, the oracle's outcome rows and its table afterwards"""
    st0, b = initial_state(P), stream(P)
    orc = oracle_lib.OracleTable(G, P, SELF, True)
    orc.load_state(st0)
    want = orc.submit(b, fill=0xAB)
    end = orc.read_state()
    orc.close()
    return types.SimpleNamespace(P=P, st0=st0, batch=b, want=want, end=end)


def reach(P):
    """the rows the docstring promises, read from the ORACLE's outcome rows and final table alone (no kernel) -> {what: True}"""
    X, w = lead(P), P // 2
    fl = X.want.reply["flags"].reshape(ROUNDS, G)
    kind = (X.batch.head["hdr"] & 0xF).reshape(ROUNDS, G)
    status, role, changed = abi.flags_status(fl), abi.flags_role(fl), (fl & abi.F_ROLE_CHANGED) != 0
    success, replied, reset, emit = (fl & abi.F_SUCCESS) != 0, (fl & abi.F_REPLIED) != 0, (fl & abi.F_RESET_TIMER) != 0, abi.flags_emit(fl)
    election = np.isin(kind, [abi.EV_RV_REQ, abi.EV_PV_REQ, abi.EV_RV_REPLY, abi.EV_PV_REPLY, abi.EV_TIMEOUT])
    assert np.isin(status, [abi.OK, abi.DROPPED_STALE_ROLE]).all(), "a row of the stream is refused"
    seen = dict(
        counted_alone=int(election[0, :64].sum()) == 1 and not election[0, 64:].any() and status[0, 0] == abi.OK and (changed[0, 0] == (w == 1)),
        nothing_to_count_alone=int(election[7].sum()) == 1 and status[7, 13] == abi.OK and not changed[7, 13],
        rv_win=changed[w - 1, 0] and role[w - 1, 0] == L and changed[w, 64] and role[w, 64] == L,
        pv_win=changed[w, 1] and role[w, 1] == C and emit[w, 1] == abi.EMIT_REQVOTE,
        counted_before_win=(w == 1) or (not changed[0, 0] and not changed[1, 1]),
        late_higher=changed[2, 2] and role[2, 2] == F and X.end.elected_epoch[2] == 0 and X.end.current_term[2] == 9,
        stale_timeouts=all(status[3, g] == abi.DROPPED_STALE_ROLE for g in (3, 4, 5)),
        to_pre=changed[4, 3] and role[4, 3] == F and emit[4, 3] == abi.EMIT_PREVOTE,
        to_candidate=changed[4, 4] and role[4, 4] == C and emit[4, 4] == abi.EMIT_REQVOTE,
        lead_prepare=not changed[4, 5] and emit[4, 5] == abi.EMIT_HEARTBEAT and reset[4, 5] and X.end.repl_prepared[5] == 1,
        to_lead=not changed[4, 6] and emit[4, 6] == abi.EMIT_HEARTBEAT and reset[4, 6],
        vote_granted=changed[5, 7] and success[5, 7] and success[6, 7] and not changed[6, 7] and X.end.voted_for[7] == 2,
        vote_refused_on_log=changed[5, 8] and replied[5, 8] and not success[5, 8],
        prevote_judged=replied[5, 9] and success[5, 9] and not changed[5, 9] and reset[5, 9],
        ack_down=changed[6, 10] and role[6, 10] == F and changed[8, 14] and role[8, 14] == F,
        rare_beside_counted=(fl[0, 11] & abi.F_LOG_APPEND) != 0 and X.end.run_count[11] == 3 and (fl[0, 12] & abi.F_LOG_APPEND) != 0 and X.end.repl_prepared[12] == 1,
        row_after_conversion=status[w, 0] == abi.OK and emit[w, 0] == abi.EMIT_HEARTBEAT and X.end.repl_prepared[0] == 1 and status[w + 1, 1] == abi.OK and
        X.end.repl_prepared[64] == 1,
        all_classes_round=all(kind[8, g] != 0 for g in (13, 3, 15, 8, 16, 14, 17)) and changed[8, 16] and (fl[8, 17] & abi.F_LOG_APPEND) != 0,
        quiet_rounds=not election[10:].any(),
        steady=all((fl[r, 18] & abi.F_COMMIT) != 0 for r in range(10)) and bool(np.any((fl[:, 19] & abi.F_COMMIT) != 0)),
    )
    return seen


def _sub_all(b):
    """the dense batch as a list batch that lists every group"""
    s = abi.Batch(b.rounds, G, gid=np.arange(G, dtype=np.uint32))
    s.head[:], s.ab[:], s.cd[:] = b.head, b.ab, b.cd
    s.entry_terms, s.entry_count = b.entry_terms, b.entry_count
    return s


def case(P, route="submit32c", force_wide=False, slow_counts=None):
    """the stream through one route of the compact formats against the oracle. force_wide: RG_FORCE_WIDE=1 while the table is created (the 64-bit body on the
    same rows). slow_counts: a callable -> (lane-rounds, slow rows, slow wave-rounds) since its last call (the host emulation's counter of rows that reach the
    general handlers: rg_emu_slow_counts); the narrow run must not send a single row there. -> workgroups the 64-bit body decided"""
    X = lead(P)
    where = "%d nodes, %s%s" % (P, route, ", RG_FORCE_WIDE=1" if force_wide else "")
    old = os.environ.get("RG_FORCE_WIDE")
    os.environ["RG_FORCE_WIDE"] = "1" if force_wide else "0"
    try:
        gpu = engine.Table(G, P, SELF, True)
    finally:
        if old is None:
            os.environ.pop("RG_FORCE_WIDE", None)
        else:
            os.environ["RG_FORCE_WIDE"] = old
    gpu.load_state(X.st0)
    gpu.wide_body_workgroups(reset=True)
    if slow_counts is not None:
        slow_counts()
    raw = None
    if route == "submit32":
        got = gpu.submit32(engine.pack32(X.batch), fill=0xAB)
    elif route == "submit32c":
        raw = gpu.submit32c(engine.pack32(X.batch), fill=0xAB)
        got, _ = engine.unpack32(raw, ROUNDS, G, X.st0.role_epoch)
    else:
        raw = gpu.submit32c_sparse_rounds(_sub_all(X.batch), fill=0xAB)
        got, _ = engine.unpack32(raw, ROUNDS, G, X.st0.role_epoch)
    slow = None if slow_counts is None else slow_counts()
    assert not np.any(got.status == abi.NEED_HOST), where
    compare_outcomes(X.want, got, where)
    after = gpu.read_state()
    compare_states(X.end, after, where)
    if raw is not None:
        check_out32_rows(raw, got, types.SimpleNamespace(commit_index=X.st0.commit_index, role_epoch=X.st0.role_epoch),
                         types.SimpleNamespace(commit_index=after.commit_index, role_epoch=after.role_epoch), ROUNDS, G)
    wide = gpu.wide_body_workgroups()
    gpu.close()
    assert force_wide or wide == 0, "%s: %d workgroups on the 64-bit body" % (where, wide)
    if slow is not None and not force_wide:
        assert slow[0] >= ROUNDS * G and slow[1] == 0 and slow[2] == 0, "%s: %d rows in %d wave-rounds reached the general handlers" % (where, slow[1], slow[2])
    return wide
