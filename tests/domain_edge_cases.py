"""Cases that hold the 32-bit step body (rg_tier1n.hpp: tier 1 in sign words) to the oracle at the TOP of its value domain and at the floor of the relative
indices, under the full mixed traffic of tests/fuzz.py. Shared by tests/test_domain_edge_gpu.py (an MI355X), tests/devemu/emu_cases_domain_edge.py (the host
emulation of the kernels) and tests/test_domain_edge_cpu.py (what can be shown on the oracle and the stream alone).

WHY. s_lt(x, y) is the sign of x - y, s_ne the sign of (x ^ y) + 0x7fffffff, s_pos the sign of -x: right only while every value is below 2^30 + 2^29 and
|x - y| < 2^31. Every other fuzz stream of the suite draws terms below ~20, indices below a few hundred and role epochs below ~50, so a predicate that is right
for small operands only, a select that truncates, a run start that is mishandled near 2^30 would pass all of them. Here the same generator runs with its
state moved to a chosen magnitude (fuzz.random_initial_state's offsets) while its absolute draws stay small — prevLogIndex 0, leaderCommit 0, a wrong
prevLogTerm of 1 .. 9 — and three "far" draws add stale requests of term 1 or 2, acks that name epoch 1 and candidates whose log ends at (1, 1): large values
meet small ones with differences of about 2^30.

THE STREAM LEADS WITH THE ORACLE (as tests/sparse_rounds_cases.lead does): lead(point, P) draws every round from the ORACLE's state and records state, rows and
outcome rows per round, once per (point, cluster), shared by every route. So the stream the kernels are given is the stream whose reach and whose domain the CPU
test proves without any kernel. LAUNCHES launches of ROUNDS rounds; the first lists every group, the second about 60 % of them (the rows of the others are
RG_EV_NONE), so the same rows are one dense launch and one launch of a list of groups.

MAGNITUDE POINTS (LIM = 2^30, the limit of a row field and of the state a launch may start with on the 32-bit body):
    top_terms / top_indices / top_epochs / top_all   the named values start at LIM - SPAN - 8 and above, the others small, index base 0
    rel_floor    indices from 2^40 + 2, each group's base = its smallest non-zero index - 1: every relative value starts at 1, 2, ...
    rel_top      indices from 2^40 + LIM - SPAN - 8, base 2^40: relative indices at the top
    rel_hole     rel_floor, but every fourth group of the SECOND workgroup has its base AT its smallest non-zero index: that value has no image (to_rel answers
                 -1, which fails every range check), so that workgroup must take the 64-bit body in every launch and no other may
    straddle     terms LIM - 6 + (1 .. 8) in the SECOND workgroup only (groups 64 .. 127): that workgroup holds a value >= LIM, the others never do
SPAN. What a value can grow by in a run, from the generator's own bounds: the initial image spreads over INIT (terms 1 .. 8; indices: epoch <= 50, then at most
three runs of <= 30 entries and nextIndex one above: 141; role epochs 1 .. 5), and per round a term rises by at most 3 (a request of term + 3 is adopted; a row
names at most term + 3), an index by at most 40 (InstallSnapshot at epoch.index + 40, the largest index any row names), a role epoch by at most 2. With R_MAX =
64 rounds as the longest any route runs a group: SPAN = INIT + STEP * (R_MAX + 1), i.e. 203 / 2741 / 135. check_domain() asserts both halves on the drawn stream:
no value of a top point exceeds offset + SPAN, hence none reaches LIM.

WHICH BODY DECIDED. For every point but `straddle` and `rel_hole` no state value and no row field reaches LIM (check_domain, in Python, before any launch), so
rg_wide_body_workgroups() must stay 0: the sign-word body is what was tested. For those two expected_wide() applies the documented rule (rg_step.hpp,
rg_device.hpp "The 32-bit tier's domain"): a workgroup — 64 consecutive rows of the launch — takes the 64-bit body in a launch iff one of its groups starts the
launch with a term, relative index or small field outside [0, LIM), or one of its rows carries a field outside [0, LIM); the counter must equal that count, and
the rule must leave the first and the third workgroup at 0. Every dense compact route ends with one launch of RG_EV_NONE rows alone: there the STATE is all that
can send a workgroup to the 64-bit body (in any other launch of `straddle` a row field at 2^30 does so too, which would hide a wrong limit in fits32).

RG_NEED_HOST. The oracle's log is lossless; the device answers RG_NEED_HOST where a lookup leaves its four cached term runs and skips the group's later rows of
the launch. The host's half of that protocol is sparse_rounds_cases.repair (a shadow oracle one launch behind stands in for the host's log; the row is resubmitted
with its hint, the skipped rows after it, as wide rows), after which EVERY row and the whole table must equal the oracle's. The rows decided that way are not
decided by the kernels under test, hence the project's cap: at most 2 % of the event rows (follower_sweep_cases.step_case)."""
import functools
import types

import numpy as np

from rafting_amd import abi, engine
from tests import compact_large_cluster_cases as K
from tests import fuzz, oracle_lib
from tests import sparse_rounds_cases as X
from tests import test_gpu_parity as T
from tests.helpers import check_out32_rows, compare_outcomes, compare_states
from tests.sparse_tick_cases import subset

LIM, HALF, BIG = 1 << 30, 1 << 29, 1 << 40
G, ROUNDS, LAUNCHES, WG = 130, 24, 2, 64
TICKS = 16
R_MAX = 64
assert ROUNDS * LAUNCHES <= R_MAX and TICKS <= R_MAX
INIT = dict(term=8, index=141, epoch=5)
STEP = dict(term=3, index=40, epoch=2)
SPAN = {k: INIT[k] + STEP[k] * (R_MAX + 1) for k in INIT}
TOP = {k: LIM - SPAN[k] - 8 for k in INIT}
STRADDLE_TERM, STRADDLE_GROUPS = LIM - 6, slice(WG, 2 * WG)
HOLE_GROUPS = slice(WG, 2 * WG, 4)
FAR = dict(far_stale=0.04, far_ack=0.04, far_vote=0.04)

POINTS = ("top_terms", "top_indices", "top_epochs", "top_all", "rel_floor", "rel_top", "straddle", "rel_hole")
SPLIT_POINTS = ("straddle", "rel_hole")                       # the second workgroup is outside the domain, by construction; the others inside
ROUTES = ("submit32", "submit32c", "sparse_rounds", "tick")          # (and "wide_rows", which the runners add per RG_SPLIT setting)
# 5 nodes for every point; 3 and 9 nodes (the latter through RG_OPT_COMPACT_ANY_CLUSTER) for top_all and rel_floor
SHAPES = tuple((p, 5) for p in POINTS) + tuple((p, c) for p in ("top_all", "rel_floor") for c in (3, 9))
# which quantities are large at a point (the row classes that are DEFINED by a magnitude can only occur there)
LARGE = dict(top_terms="T", top_indices="I", top_epochs="E", top_all="TIE", rel_floor="", rel_top="I", straddle="T", rel_hole="")
# (point, cluster) -> seed where the default one misses a row class: nine nodes need four granted votes in a row for a conversion to Leader, which the default
# seeds of the two 9-node streams do not draw within 48 rounds (tests/test_domain_edge_cpu.py holds every stream to its classes)
SEEDS = {("top_all", 9): 1000, ("rel_floor", 9): 1001}


def seed_of(point, P):
    return SEEDS.get((point, P), 900 + 16 * POINTS.index(point) + P)


def offsets(point):
    """fuzz.random_initial_state's offsets at a point -> (index offset, term offset, epoch offset)"""
    index = {"top_indices": TOP["index"], "top_all": TOP["index"], "rel_floor": BIG + 2, "rel_hole": BIG + 2, "rel_top": BIG + TOP["index"]}.get(point, 0)
    term = TOP["term"] if point in ("top_terms", "top_all") else 0
    epoch = TOP["epoch"] if point in ("top_epochs", "top_all") else 0
    return index, term, epoch


def state_maker(point):
    def make(groups, P, self_slot, seed):
        index, term, epoch = offsets(point)
        st = fuzz.random_initial_state(groups, P, self_slot, seed, offset=index, term_offset=term, epoch_offset=epoch)
        if point == "straddle":
            fuzz.shift_state(st, term_offset=STRADDLE_TERM, groups=STRADDLE_GROUPS)
        return st
    return make


INDEX_COLUMNS = ("commit_index", "epoch_index", "first_index", "last_index", "run_start", "peer_last_epoch", "peer_next_index", "peer_match_index")
TERM_COLUMNS = ("current_term", "epoch_term", "elected_term", "run_term")


def _per_group(st, name):
    a = getattr(st, name).astype(np.int64).reshape(st.count, -1)
    if name.startswith("run_"):                               # (only the live slots of the run cache hold values)
        a = np.where(np.arange(a.shape[1])[None, :] < st.run_count.astype(np.int64)[:, None], a, 0)
    return a


def base_maker(point):
    """the table's index bases at a point, as a function of the initial state (None: no bases)"""
    if point == "rel_top":
        return lambda st: np.full(st.count, BIG, dtype=np.int64)
    if point in ("rel_floor", "rel_hole"):
        def floor(st):
            cols = np.concatenate([_per_group(st, n) for n in INDEX_COLUMNS], axis=1)
            low = np.where(cols != 0, cols, np.iinfo(np.int64).max).min(axis=1)
            assert np.all(low >= BIG - 30) and np.all(low < np.iinfo(np.int64).max)
            base = (low - 1).astype(np.int64)
            if point == "rel_hole":
                base[HOLE_GROUPS] += 1
            return base
        return floor
    return None


def _rel(x, base):
    """rg_device.hpp's to_rel for arrays whose rows are groups: 0 stays 0, x == base != 0 has no image (-1)"""
    if base is None:
        return x
    b = base.reshape((-1,) + (1,) * (x.ndim - 1))
    return np.where(x == 0, 0, np.where(x == b, -1, x - b))


IXF = np.array([0, 0xA, 0x6, 0x2, 0x2, 0x2, 0, 0, 0, 0, 0x1, 0x2, 0, 0, 0, 0], dtype=np.uint32)      # which of a, b, c, d are log indices, by event kind
AUX_IS_EPOCH = np.isin(np.arange(16), [abi.EV_AE_ACK, abi.EV_IS_ACK, abi.EV_RV_REPLY, abi.EV_PV_REPLY, abi.EV_TIMEOUT])
A_IS_TERM = np.isin(np.arange(16), [abi.EV_AE_REQ, abi.EV_AE_ACK, abi.EV_IS_ACK, abi.EV_RV_REQ, abi.EV_PV_REQ, abi.EV_RV_REPLY, abi.EV_PV_REPLY, abi.EV_IS_REQ])


def row_fields(b, base, groups=None):
    """the fields of the rows of batch b as the compact format carries them (log indices relative to their group's base) -> kind, [4][rows] fields, aux"""
    kind = (b.head["hdr"] & 0xF).astype(np.int64)
    cols = np.stack([b.ab["x"], b.ab["y"], b.cd["x"], b.cd["y"]]).astype(np.int64)
    if base is not None:
        gb = base if groups is None else base[groups]
        gb = np.tile(gb, len(kind) // len(gb))
        is_ix = ((IXF[kind][None, :] >> np.arange(4, dtype=np.uint32)[:, None]) & 1) != 0
        cols = np.where(is_ix & (cols != 0), cols - gb[None, :], cols)
    return kind, cols, b.head["aux"].astype(np.int64)


def state_extremes(st, base):
    """-> per group: the largest term, relative index and small field (role epochs, votes, node ids + 1) of a state image, and the smallest relative index"""
    term = np.concatenate([_per_group(st, n) for n in TERM_COLUMNS], axis=1)
    index = np.concatenate([_rel(_per_group(st, n), base) for n in INDEX_COLUMNS], axis=1)
    small = np.stack([st.role_epoch.astype(np.int64), st.elected_epoch.astype(np.int64), st.votes.astype(np.int64), st.current_leader.astype(np.int64) + 1,
                      st.voted_for.astype(np.int64) + 1], axis=1)
    return types.SimpleNamespace(term=term.max(axis=1), index=index.max(axis=1), index_min=index.min(axis=1), small=small.max(axis=1),
                                 term_min=term.min(axis=1), small_min=small.min(axis=1), epoch=np.maximum(st.role_epoch, st.elected_epoch).astype(np.int64))


def rows_out_of_domain(b, base, groups=None):
    """rows of batch b that send their workgroup to the 64-bit body (class_word in rg_step.hpp): a field outside [0, LIM) — `aux` too where it is a role epoch or
    the one term of a request's entries"""
    kind, cols, aux = row_fields(b, base, groups)
    bad = ((cols < 0) | (cols >= LIM)).any(axis=0)
    n = (b.head["hdr"] >> 12).astype(np.int64)
    same = np.zeros(len(kind), dtype=bool)                    # RG_HDR_SAME_TERM as the packer sets it: every entry of the row has one term, carried in aux
    for r in np.flatnonzero((kind == abi.EV_AE_REQ) & (n > 0)):
        e = b.entry_terms[int(aux[r]): int(aux[r]) + int(n[r])]
        if len(e) == n[r] and np.all(e == e[0]):
            same[r] = True
            bad[r] |= int(e[0]) >= LIM
    return bad | (AUX_IS_EPOCH[kind] & (aux >= LIM))


def state_out_of_domain(st, base):
    """groups whose image cannot start a launch on the 32-bit body (fits32, small_fields_fit and the index-base rule of step32_kernel)"""
    x = state_extremes(st, base)
    bad = (x.term >= LIM) | (x.term_min < 0) | (x.index >= LIM) | (x.index_min < 0) | (x.small >= LIM) | (x.small_min < 0)
    if base is not None:
        bad |= (base != 0) & (_rel(st.epoch_index.astype(np.int64), base) <= 0)
    return bad


def expected_wide(start, big, rows, base, rounds):
    """the documented rule, per workgroup (64 consecutive rows of the launch: `rows` are their groups) -> [workgroups] 0 / 1: it takes the 64-bit body"""
    n = len(rows)
    out = (state_out_of_domain(start, base)[rows]) | rows_out_of_domain(big, base, rows).reshape(rounds, n).any(axis=0)
    return np.array([int(out[w:w + WG].any()) for w in range(0, n, WG)])


@functools.lru_cache(maxsize=None)
def lead(point, P):
    """the oracle's half of a case, once per (point, cluster): LAUNCHES x ROUNDS rounds drawn from the oracle's state, each decided by the oracle"""
    seed, self_slot = seed_of(point, P), 1 % P
    st0 = state_maker(point)(G, P, self_slot, seed)
    base = base_maker(point)
    base = None if base is None else base(st0)
    orc = oracle_lib.OracleTable(G, P, self_slot, True)
    orc.load_state(st0)
    fz = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False, **FAR)
    rng = np.random.default_rng(seed)
    launches, unpackable, drawn = [], 0, 0
    for k in range(LAUNCHES):
        pick = np.ones(G, dtype=bool) if k == 0 else rng.random(G) < 0.6
        pick[[0, WG, 2 * WG]] = True                          # (a row of every workgroup in every launch)
        states, batches, outs = [], [], []
        for r in range(ROUNDS):
            cur = orc.read_state()
            b = abi.Batch(1, G)
            fz.round(cur, b, 0)
            T.blank_rows(b, ~pick)
            drawn += int(np.count_nonzero(b.head["hdr"] & 0xF))
            if base is not None:                              # (what the format cannot hold relative to the bases: index_base_case sends such rows beside the batch)
                bad = T.unpackable_rows(b, base) & ((b.head["hdr"] & 0xF) != 0)
                unpackable += int(np.count_nonzero(bad))
                T.blank_rows(b, bad)
            assert base is not None or abi.batch_fits_32(b)
            states.append(cur)
            batches.append(b)
            outs.append(orc.submit(b))
        big = fuzz.concat_batches(batches)
        launches.append(types.SimpleNamespace(pick=pick, rows=np.flatnonzero(pick), start=states[0], states=states, batches=batches, outs=outs, big=big,
                                              want=fuzz.concat_outcomes(outs), end=orc.read_state()))
    orc.close()
    # (rel_floor and rel_top: about 3 % — a prevLogIndex or an acknowledged epoch one below the group's epoch, a candidate whose log ends at index 1; rel_hole: 6 %,
    #  a group whose epoch.index is the hole can be sent next to nothing that names it)
    assert unpackable * 10 <= drawn, "%d of %d rows cannot travel relative to the bases" % (unpackable, drawn)
    return types.SimpleNamespace(point=point, P=P, self_slot=self_slot, seed=seed, st0=st0, base=base, launches=launches)


# ---- on the oracle and the stream alone -------------------------------------------------------------------------------------------------------------------
def check_domain(L):
    """No value of the stream reaches LIM where none is expected, and no value of a top point grew by more than SPAN; `straddle`: the rule sends the second
    workgroup of every dense launch to the 64-bit body and no other. -> the largest (term, relative index, small field) seen"""
    index_off, term_off, epoch_off = offsets(L.point)
    if L.base is not None:
        index_off = index_off - BIG if L.point == "rel_top" else 0
    top = dict(term=0, index=0, epoch=0)
    for la in L.launches:
        for st in la.states + [la.end]:
            x = state_extremes(st, L.base)
            top["term"], top["index"], top["epoch"] = max(top["term"], int(x.term.max())), max(top["index"], int(x.index.max())), max(top["epoch"], int(x.epoch.max()))
            if L.point not in SPLIT_POINTS:
                assert not state_out_of_domain(st, L.base).any(), "%s: a state value outside [0, LIM)" % L.point
            else:
                bad = state_out_of_domain(st, L.base)
                assert not bad[:WG].any() and not bad[2 * WG:].any() and bad[STRADDLE_GROUPS].any()
        for b in la.batches:
            kind, cols, aux = row_fields(b, L.base)
            bad = rows_out_of_domain(b, L.base)
            if L.point not in SPLIT_POINTS:
                assert not bad.any(), "%s: a row field outside [0, LIM)" % L.point
            else:
                assert not bad[:WG].any() and not bad[2 * WG:].any()
            is_ix = ((IXF[kind][None, :] >> np.arange(4, dtype=np.uint32)[:, None]) & 1) != 0
            top["index"] = max(top["index"], int(np.where(is_ix, cols, 0).max()))
            top["epoch"] = max(top["epoch"], int(np.where(AUX_IS_EPOCH[kind], aux, 0).max()))
            if L.point != "straddle":
                top["term"] = max(top["term"], int(np.where(~is_ix & (kind != abi.EV_CLIENT_APPEND), cols, 0).max()), int(b.entry_terms[:b.entry_count].max(initial=0)))
        if L.point in SPLIT_POINTS:
            w = expected_wide(la.start, la.big, np.arange(G), L.base, ROUNDS)
            assert list(w) == [0, 1, 0], w
            quiet = state_out_of_domain(la.end, L.base)       # ... by its STATE alone, whatever the rows carry
            assert quiet[STRADDLE_GROUPS].any() and not quiet[:WG].any() and not quiet[2 * WG:].any()
    if L.point == "rel_hole":
        assert max(top.values()) < LIM
    elif L.point != "straddle":
        assert top["term"] <= term_off + SPAN["term"] and top["index"] <= index_off + SPAN["index"] and top["epoch"] <= epoch_off + SPAN["epoch"], (L.point, top)
        assert max(top.values()) < LIM
        for dim, key in (("T", "term"), ("I", "index"), ("E", "epoch")):      # ... and a point's large quantities really are at the top
            assert (top[key] > LIM - 2 * SPAN[key] - 16) == (dim in LARGE[L.point]), (L.point, key, top)
    return top


CLASSES = ("conflict_truncates", "vote_granted", "vote_refused_on_log", "ack_commits", "to_leader", "to_follower_by_term", "flush_trims", "push_shifts_out")
FAR_CLASSES = dict(T=("stale_ae_far", "vote_granted_large_row", "vote_refused_small_row"), I=("ae_prev0_far", "vote_granted_large_row", "vote_refused_small_row"),
                   E=("fenced_ack_far",))


def required(point):
    need = list(CLASSES)
    for dim in LARGE[point]:
        need += [c for c in FAR_CLASSES[dim] if c not in need]
    if point == "rel_top":
        # a candidate whose log ends at (1, 1) names an index BELOW the groups' base (2^40): the compact format has no image for it (only 0 travels as 0), such a
        # row travels as a wide row beside the batch (index_base_case) and never meets the 32-bit body. The small operand of this point is prevLogIndex 0.
        need.remove("vote_refused_small_row")
    return need


def reach(L):
    """what the stream hits, from the oracle's states and outcome rows -> {class: rows}. Indices are taken relative to the bases (what the 32-bit body sees)."""
    seen = dict.fromkeys(CLASSES + tuple(c for v in FAR_CLASSES.values() for c in v), 0)
    big_t, big_i = "T" in LARGE[L.point], "I" in LARGE[L.point]
    K_ = abi.TERM_RUNS
    for la in L.launches:
        for r in range(ROUNDS):
            cur, nxt, b, oo = la.states[r], (la.states[r + 1] if r + 1 < ROUNDS else la.end), la.batches[r], la.outs[r]
            kind, (a, bb, c, d), aux = row_fields(b, L.base)
            fl = oo.reply["flags"]
            ok = abi.flags_status(fl) == abi.OK
            replied, success = (fl & abi.F_REPLIED) != 0, (fl & abi.F_SUCCESS) != 0
            term, role, rc = cur.current_term.astype(np.int64), cur.role, cur.run_count.astype(np.int64)
            last = _rel(cur.last_index.astype(np.int64), L.base)
            lt = cur.run_term.reshape(G, K_)[np.arange(G), np.maximum(rc, 1) - 1].astype(np.int64)
            ae = kind == abi.EV_AE_REQ
            seen["stale_ae_far"] += int(np.count_nonzero(ae & replied & ~success & (term - a > HALF)))
            seen["ae_prev0_far"] += int(np.count_nonzero(ae & replied & (a >= term) & (bb == 0) & (rc > 0) & (last > HALF)))
            seen["conflict_truncates"] += int(np.count_nonzero(ae & ((fl & abi.F_LOG_TRUNC) != 0)))
            vq = ((kind == abi.EV_RV_REQ) | (kind == abi.EV_PV_REQ)) & (role == abi.FOLLOWER) & (rc > 0) & ok & replied
            granted = vq & success
            refused = vq & (kind == abi.EV_RV_REQ) & (a > term) & ~success      # a RequestVote of a higher term at a Follower is refused by logUpToDate alone
            row_large = np.zeros(G, dtype=bool) | (big_t & (c > HALF)) | (big_i & (bb > HALF))
            row_small = np.zeros(G, dtype=bool) | (big_t & (lt - c > HALF)) | (big_i & (last - bb > HALF))
            seen["vote_granted"] += int(np.count_nonzero(granted))
            seen["vote_refused_on_log"] += int(np.count_nonzero(refused))
            seen["vote_granted_large_row"] += int(np.count_nonzero(granted & row_large))
            seen["vote_refused_small_row"] += int(np.count_nonzero(refused & row_small))
            ack = (kind == abi.EV_AE_ACK) | (kind == abi.EV_IS_ACK)
            seen["ack_commits"] += int(np.count_nonzero((kind == abi.EV_AE_ACK) & ((fl & abi.F_COMMIT) != 0)))
            seen["fenced_ack_far"] += int(np.count_nonzero(ack & (abi.flags_status(fl) == abi.DROPPED_STALE_ROLE) & (cur.role_epoch.astype(np.int64) - aux > HALF)))
            changed = (fl & abi.F_ROLE_CHANGED) != 0
            seen["to_leader"] += int(np.count_nonzero(changed & (abi.flags_role(fl) == abi.LEADER)))
            seen["to_follower_by_term"] += int(np.count_nonzero(changed & (abi.flags_role(fl) == abi.FOLLOWER) & A_IS_TERM[kind] & (a > term)))
            rc2 = nxt.run_count.astype(np.int64)
            s0, s0_next = cur.run_start.reshape(G, K_)[:, 0], nxt.run_start.reshape(G, K_)[:, 0]
            seen["flush_trims"] += int(np.count_nonzero((kind == abi.EV_LOG_FLUSH) & ok & (rc > 0) & ((rc2 < rc) | ((rc2 == rc) & (s0_next > s0)))))
            seen["push_shifts_out"] += int(np.count_nonzero(((fl & abi.F_LOG_APPEND) != 0) & (rc == K_) & (rc2 == K_) & (s0_next > s0)))
    return seen


# ---- the kernels against the recorded stream ------------------------------------------------------------------------------------------------------------
def _rows_of(out, idx):
    o = abi.Outcome(len(idx))
    o.reply, o.logfx, o.persist = out.reply[idx], out.logfx[idx], out.persist[idx]
    return o


def _repair(gpu, shadow, la, rows, sub, got, where):
    """The host half of the RG_NEED_HOST protocol for one launch, by sparse_rounds_cases.repair: `shadow` (an oracle one launch behind) stands in for the host's
    log, the row that answered RG_NEED_HOST is resubmitted with its hint and the rows the launch skipped after it, round by round, as wide rows; `got` is
    repaired in place, the shadow steps through the launch -> the event rows that were decided that way and not by the launch"""
    n = len(rows)
    st = got.status.reshape(ROUNDS, n)
    stopped = (st == abi.NEED_HOST) | (st == abi.SKIPPED_AFTER_NEED_HOST)
    t = types.SimpleNamespace(R=ROUNDS, n=n, rows=rows, gid=rows.astype(np.uint32), batch=sub, subs=[subset(b, rows) for b in la.batches], dense=la.batches,
                              nows=[0] * ROUNDS)
    cols = X.repair(gpu, shadow, t, got)
    assert (len(cols) > 0) == bool(stopped.any()), where
    return int(np.count_nonzero(stopped))


def _sub(big, rows, rounds):
    """the rows of groups `rows` of the dense `rounds`-round batch as a list batch"""
    n, Gd = len(rows), big.count
    s = abi.Batch(rounds, n, gid=rows.astype(np.uint32))
    s.head[:] = big.head.reshape(rounds, Gd)[:, rows].reshape(-1)
    s.ab[:], s.cd[:] = big.ab.reshape(rounds, Gd)[:, rows].reshape(-1), big.cd.reshape(rounds, Gd)[:, rows].reshape(-1)
    s.entry_terms, s.entry_count = big.entry_terms, big.entry_count
    return s


def launch_case(point, P, route):
    """the recorded stream through rg_submit32 (compact rows, wide outcome rows), rg_submit32c (compact outcome rows) — dense multi-round launches — or
    rg_submit32c_sparse_rounds (each launch's listed groups): every outcome row and the table after every launch bit for bit, and which body decided.
    "wide_rows": the same launches as wide rows through rg_submit (step_kernel or step_split_kernel, as RG_SPLIT says when the table is created) — 64-bit
    arithmetic throughout, no index bases, no compact launch: the general handlers on the same magnitudes, and a second witness of the recorded rows."""
    assert route in ("submit32", "submit32c", "sparse_rounds", "wide_rows")
    L = lead(point, P)
    check_domain(L)
    with K.routed(None):                                      # (RG_OPT_COMPACT_ANY_CLUSTER: what lets the 9-node table in; nothing at 7 nodes and below)
        gpu = engine.Table(G, P, L.self_slot, True)
    if L.base is not None and route != "wide_rows":
        gpu.set_index_base(L.base)
    gpu.load_state(L.st0)
    shadow = oracle_lib.OracleTable(G, P, L.self_slot, True)
    shadow.load_state(L.st0)
    gpu.wide_body_workgroups(reset=True)
    expected, lost, events = [], 0, 0
    for k, la in enumerate(L.launches):
        where = "%s, %d nodes, %s, launch %d" % (point, P, route, k)
        rows = la.rows if route == "sparse_rounds" else np.arange(G)
        n = len(rows)
        ep0 = la.start.role_epoch[rows]
        base_rows = None if L.base is None else L.base[rows]
        sub = _sub(la.big, rows, ROUNDS)
        kinds = (sub.head["hdr"] & 0xF).reshape(ROUNDS, n)
        if route == "sparse_rounds":
            raw = gpu.submit32c_sparse_rounds(sub, fill=0xAB, index_base=L.base)
            got, _ = engine.unpack32(raw, ROUNDS, n, ep0, index_base=base_rows)
            want = _rows_of(la.want, (np.arange(ROUNDS)[:, None] * G + rows[None, :]).reshape(-1))
        elif route == "wide_rows":
            got = gpu.submit(la.big, fill=0xAB)
            want = la.want
        else:
            b32 = engine.pack32(la.big, index_base=L.base)
            if route == "submit32":
                got = gpu.submit32(b32, fill=0xAB)
            else:
                raw = gpu.submit32c(b32, fill=0xAB)
                got, _ = engine.unpack32(raw, ROUNDS, G, ep0, index_base=L.base)
            want = la.want
        clean = not np.any(got.status == abi.NEED_HOST)
        gone = _repair(gpu, shadow, la, rows, sub, got, where)
        assert clean == (gone == 0), where
        compare_outcomes(want, got, where)
        after = gpu.read_state()
        compare_states(la.end, after, where)
        if route in ("submit32c", "sparse_rounds") and L.base is None and clean:
            check_out32_rows(raw, got, types.SimpleNamespace(commit_index=la.start.commit_index[rows], role_epoch=ep0),
                             types.SimpleNamespace(commit_index=after.commit_index[rows], role_epoch=after.role_epoch[rows]), ROUNDS, n)
        lost, events = lost + gone, events + int(np.count_nonzero(kinds))
        if route == "wide_rows":                              # (no compact launch: the counter does not move)
            expected.append(np.zeros(3, dtype=np.int64))
        else:
            expected.append(expected_wide(la.start, la.big if route != "sparse_rounds" else _as_dense(sub), rows, L.base, ROUNDS))
    if route in ("submit32", "submit32c"):                    # one launch of RG_EV_NONE rows: the state alone says which body runs
        quiet, where = abi.Batch(1, G), "%s, %d nodes, %s, the quiet launch" % (point, P, route)
        b32 = engine.pack32(quiet, index_base=L.base)
        got = gpu.submit32(b32) if route == "submit32" else engine.unpack32(gpu.submit32c(b32), 1, G, L.launches[-1].end.role_epoch, index_base=L.base)[0]
        compare_outcomes(shadow.submit(quiet), got, where)
        compare_states(L.launches[-1].end, gpu.read_state(), where)
        expected.append(expected_wide(L.launches[-1].end, quiet, np.arange(G), L.base, 1))
    wide = gpu.wide_body_workgroups()
    gpu.close()
    shadow.close()
    print("%s, %d nodes, %s: %d of %d event rows lost behind RG_NEED_HOST, %d workgroups on the 64-bit body" % (point, P, route, lost, events, wide))
    assert lost * 50 <= events, "%d of %d rows were not decided by the launch (cap: 2 %%)" % (lost, events)
    want_wide = int(sum(int(w.sum()) for w in expected))
    if point not in SPLIT_POINTS:
        assert want_wide == 0
    elif route in ("submit32", "submit32c"):
        assert all(list(w) == [0, 1, 0] for w in expected), expected      # (the first and the third workgroup stay narrow)
    assert wide == want_wide, "%s, %d nodes, %s: %d workgroups took the 64-bit body, the rule says %d" % (point, P, route, wide, want_wide)
    return lost, events, wide


def _as_dense(sub):
    """a list batch seen as a dense batch over its own rows (row_fields only reads the columns)"""
    return types.SimpleNamespace(head=sub.head, ab=sub.ab, cd=sub.cd, entry_terms=sub.entry_terms, entry_count=sub.entry_count, count=sub.count, rounds=sub.rounds)


def tick_case(point, P, nodes=None):
    """one recording of the dense device-resident tick (test_gpu_parity.tick2_case) with the point's magnitudes passed through to the state generator and the
    fuzzer; before every launch the state and the rows are held to the domain in Python, and the rule counts the workgroups that must take the 64-bit body"""
    base_fn = base_maker(point)
    box = dict(base=None, expected=0)

    def bases(st0):
        box["base"] = base_fn(st0)
        return box["base"]

    def watch(cur, b):
        w = expected_wide(cur, b, np.arange(G), box["base"], 1)
        if point not in SPLIT_POINTS:
            assert not w.any(), "%s: a value outside [0, LIM) before a tick" % point
        else:
            assert list(w) == [0, 1, 0], w
        box["expected"] += int(w.sum())
    report = {}
    with K.routed(None):
        T.tick2_case(G=G, P=P, ticks=TICKS, seed=seed_of(point, P) + 7, nodes=nodes, make_state=state_maker(point), fuzz_kw=FAR,
                     index_base=None if base_fn is None else bases, watch=watch, report=report)
    print("%s, %d nodes, tick: %d rows repaired through the hint protocol, %d workgroups on the 64-bit body" % (point, P, report["repaired"], report["wide_bodies"]))
    assert report["repaired"] * 50 <= G * TICKS
    assert report["wide_bodies"] == box["expected"], "%s tick: %d workgroups took the 64-bit body, the rule says %d" % (point, report["wide_bodies"], box["expected"])
    return report["wide_bodies"]


def case(point, P, route):
    """-> the workgroups the 64-bit body decided"""
    if route == "tick":
        return tick_case(point, P)
    return launch_case(point, P, route)[2]
