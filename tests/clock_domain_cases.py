"""Cases that hold every kernel that takes a clock to the oracle at the clock values real hosts pass. Shared by tests/test_clock_domain_gpu.py (an MI355X),
tests/devemu/emu_cases_clock_domain.py (the host emulation of the kernels) and tests/test_clock_domain_cpu.py (what can be shown on the oracle and the stream alone).

WHY. The reference takes `now` from System.currentTimeMillis(): about 1.76e12, 2^40.7. Every other clock of the suite is tests/clock.py's default origin, 10_000,
plus a few thousand: below 2^17. A clock, a deadline or a requestSuccess / requestFailure column narrowed to 32 bits, an (int32_t) or (uint32_t) cast, a hash in
election_timeout() that takes the low word of `now`, a compare on a truncated difference in ready_of — each is an identity below 2^31 and would pass all of them.
Kernels: timers_arm / _update / _update32 / _count / _scan / _emit, health_update / _failure, ready, and inside the recorded ticks fold_rows_of, expire_tail,
ready_of and the in-flight walk of replicate_wave.

CLOCK POINTS (POINTS): the origin of a run; a run advances TICK_MS per round, TICKS rounds, so a cross* run has clocks, deadlines and requestSuccess values on both
sides of its power of two (crossing(), asserted on the ORACLE's columns).

THE DOMAIN (include/raftgpu.h, "the clock"): 1 <= now <= 2^62; election_ms, heartbeat_ms >= 1. 0, -1 and INT64_MAX in the deadline column mean "no ticket",
"fired" and "muted".

THE STAND-ALONE LOOP LEADS WITH THE ORACLE: loop(point, P, compact, device) draws every round from the ORACLE's state with generators seeded by (point, P), so the
run without a device (device=False: tests/test_clock_domain_cpu.py's reach proofs) is the very stream the kernels are given.

NEED_HOST rows are repaired through the hint protocol as in tests/test_gpu_parity.py and are not decided by the kernels under test: the project's cap, 2 % of
the rows, holds here too."""
import contextlib
import functools
import hashlib
import types

import numpy as np

from rafting_amd import abi, engine
from tests import assemble_cases as A
from tests import clock, fuzz, oracle_lib
from tests import compact_large_cluster_cases as K
from tests import in_flight_cases as I
from tests import sparse_rounds_cases as X
from tests import sparse_tick_cases as S
from tests import test_gpu_parity as T
from tests.helpers import compare_outcomes, compare_states, make_state, simple_log

INT64_MAX = (1 << 63) - 1
NOW_MAX = 1 << 62                                             # the documented top of the clock's domain
POINTS = dict(
    epoch_ms=1_760_000_000_000,    # any 32-bit narrowing at the product's own magnitude (System.currentTimeMillis())
    cross31=(1 << 31) - 1000,      # a signed 32-bit path: the run starts below 2^31 and ends above it
    cross32=(1 << 32) - 1000,      # an unsigned 32-bit path or a low-word hash: the run crosses 2^32
    high=NOW_MAX,                  # the top of the domain: now + 2 * election_ms must not wrap, INT64_MAX stays apart from every deadline
)
CROSSES = dict(cross31=31, cross32=32)
TICK_MS, TICKS = 150, 16                                      # (>= 14 ticks: 2 100 ms, past the 1 000 ms a cross* origin lies below its power of two)
E_MS, HB_MS, TIMER_SEED = 900, 300, 1234
READY_PAIRS = ((0, 0), (1, 0), (0, 60), (2, 100), (1, 10 ** 9))      # (critical_point, cool_down), as test_health_replay_matches_oracle asks
G_LOOP, CLUSTERS = 300, (3, 5, 9)                             # two workgroups of the timer kernels, a ragged last wavefront
SHORT = 17                                                    # the expired list's capacity in the rounds r % 7 == SHORT_AT
SHORT_AT = 6
G_TICK = 130
# (point, P) -> seed: chosen so that every reach condition of check_reach holds on the ORACLE's run (tests/test_clock_domain_cpu.py); what is rare is a row that
# resets the timer of a participant whose ticket has fired and whose onTimeout is still on its way, and a nine-node leader that is ready
LOOP_SEEDS = {("epoch_ms", 3): 3116, ("epoch_ms", 5): 3100, ("epoch_ms", 9): 3139, ("cross31", 3): 3125, ("cross31", 5): 3101, ("cross31", 9): 3211,
              ("cross32", 3): 3150, ("cross32", 5): 3116, ("cross32", 9): 3135, ("high", 3): 3116, ("high", 5): 3100, ("high", 9): 3135}


def seed_of(point, P):
    return LOOP_SEEDS[(point, P)]


def crossing(point, deadlines, successes, where=""):
    """a cross* run has deadlines and requestSuccess values on both sides of its power of two"""
    if point not in CROSSES:
        return
    edge = 1 << CROSSES[point]
    for name, col in (("deadlines", deadlines), ("requestSuccess", successes)):
        v = np.asarray(col, dtype=np.int64).reshape(-1)
        v = v[(v > 0) & (v < INT64_MAX)]
        assert len(v) and int(v.min()) < edge <= int(v.max()), "%s %s: the %s do not cross 2^%d" % (point, where, name, CROSSES[point])


class Watch:
    """what the ORACLE's timer and health columns held whenever a case read them (the recorded ticks are existing case functions: this is how their runs are
    held to crossing()) and every clock the oracle was given (clocks: the default-origin identity of tests/test_clock_domain_cpu.py)"""

    def __init__(self):
        self.deadlines, self.successes, self.clocks = [], [], []


@contextlib.contextmanager
def watching():
    w = Watch()
    saved = {n: getattr(oracle_lib.OracleTable, n) for n in ("timers_read", "health_read", "submit", "timers_arm", "timers_update", "timers_expired",
                                                              "timers_expired_epochs", "health_failure", "ready")}

    def timers_read(self, *a, **kw):
        d = saved["timers_read"](self, *a, **kw)
        w.deadlines.append(d.copy())
        return d

    def health_read(self, *a, **kw):
        h = saved["health_read"](self, *a, **kw)
        w.successes.append(h[0].copy())
        return h

    def submit(self, batch, out=None, fill=0, now=None):
        if now is not None:
            w.clocks.append(("submit",) + tuple(int(x) for x in now))
        return saved["submit"](self, batch, out, fill, now)

    def timers_update(self, batch_rounds, batch_count, reply, now, gid=None):
        w.clocks.append(("timers_update",) + tuple(int(x) for x in now))
        return saved["timers_update"](self, batch_rounds, batch_count, reply, now, gid)

    def with_now(name, at):
        def f(self, *a, **kw):
            w.clocks.append((name, int(a[at])))
            return saved[name](self, *a, **kw)
        return f
    patch = dict(timers_read=timers_read, health_read=health_read, submit=submit, timers_update=timers_update, timers_arm=with_now("timers_arm", 0),
                 timers_expired=with_now("timers_expired", 0), timers_expired_epochs=with_now("timers_expired_epochs", 0),
                 health_failure=with_now("health_failure", 3), ready=with_now("ready", 0))
    for n, f in patch.items():
        setattr(oracle_lib.OracleTable, n, f)
    try:
        yield w
    finally:
        for n, f in saved.items():
            setattr(oracle_lib.OracleTable, n, f)


def clock_digest(w):
    return hashlib.sha256(repr(w.clocks).encode()).hexdigest()


# ---- RaftRoutine.resetTimer, restated in Python (a third witness beside the oracle's C and the kernels' rearm) --------------------------------------------------
def rearm_branch(d, flags):
    """-> which branch of rearm a reply row with RG_F_RESET_TIMER takes on a deadline d"""
    fresh = bool(flags & abi.F_ROLE_CHANGED)
    if fresh:
        d = 0
    if int(abi.flags_role(flags)) == abi.LEADER:
        return "leader_no_ticket" if d == 0 else "leader_ticket"
    if d < 0:
        return "fired_kept"
    if flags & abi.F_TIMER_MUTED:
        return "muted"
    return "draw"


BRANCHES = ("fresh", "leader_no_ticket", "leader_ticket", "fired_kept", "muted", "draw")


def check_rearm(before, after, flags, now, seen, where):
    """every re-armed deadline is what its branch says, literally; the election draw lies in [now + E, now + 2E]"""
    for g in np.flatnonzero(flags & abi.F_RESET_TIMER):
        f, d0, d1 = int(flags[g]), int(before[g]), int(after[g])
        br = rearm_branch(d0, f)
        seen[br] += 1
        seen["fresh"] += bool(f & abi.F_ROLE_CHANGED)
        if br == "leader_no_ticket":
            assert d1 == now, (where, g, br, d1)
        elif br == "leader_ticket":
            assert d1 == now + HB_MS, (where, g, br, d1)
        elif br == "fired_kept":
            assert d1 == d0 == -1, (where, g, br, d0, d1)
        elif br == "muted":
            assert d1 == INT64_MAX, (where, g, br, d1)
        else:
            assert now + E_MS <= d1 <= now + 2 * E_MS, (where, g, br, d1 - now)
    quiet = (flags & abi.F_RESET_TIMER) == 0
    assert np.array_equal(before[quiet], after[quiet]), where


# ---- 1. the stand-alone calls in a closed loop ---------------------------------------------------------------------------------------------------------------------
def _same_health(gpu, orc, where):
    h = orc.health_read()
    if gpu is not None:
        for name, a, c in zip(("requestSuccess", "requestFailure", "recentFailure"), gpu.health_read(), h):
            assert np.array_equal(a, c), (where, name, np.argwhere(a != c)[:4].tolist())
    return h


def _same_timers(gpu, orc, where):
    d = orc.timers_read()
    if gpu is not None:
        got = gpu.timers_read()
        assert np.array_equal(got, d), (where, "deadline", [(int(g), int(got[g]), int(d[g])) for g in np.flatnonzero(got != d)[:4]])
    return d


def loop(point, P, compact=False, device=True, origin=None):
    """arm -> timers_expired_epochs -> TIMEOUT rows -> submit -> health_update / timers_update -> health_failure -> replicate -> ready, TICKS rounds at the
    point's origin, G_LOOP groups: outcome rows, deadlines, expired lists with epochs, the three health columns, the send table, readiness and the table, bit for
    bit against the oracle after every step. compact: submit32c + timers_update32 + health_update32. device=False: the oracle alone -> the reach statistics."""
    G, self_slot, seed = G_LOOP, 2 % P, seed_of(point, P)
    origin = POINTS[point] if origin is None else origin
    st0 = fuzz.random_initial_state(G, P, self_slot, seed)
    orc = oracle_lib.OracleTable(G, P, self_slot, True)
    gpu = None
    if device:
        with K.routed(None):                                  # (RG_OPT_COMPACT_ANY_CLUSTER: what lets the 9-node table onto the compact route)
            gpu = engine.Table(G, P, self_slot, True)
    fz, rng = fuzz.Fuzzer(G, P, self_slot, seed, allow_miss=False), np.random.default_rng(seed + 1)
    for t in (gpu, orc):
        if t is not None:
            t.load_state(st0)
            t.timers_configure(E_MS, HB_MS, TIMER_SEED)
            t.timers_arm(origin)
    d = _same_timers(gpu, orc, "armed")
    seen = dict.fromkeys(BRANCHES, 0)
    check_rearm(np.zeros(G, np.int64), d, np.full(G, abi.F_RESET_TIMER | abi.F_ROLE_CHANGED, np.uint32) | (st0.role.astype(np.uint32) << abi.F_ROLE_SHIFT),
                origin, dict.fromkeys(BRANCHES, 0), "armed")
    stats = types.SimpleNamespace(fired_rounds=0, fired=0, late=0, ready={p: np.zeros(2, np.int64) for p in READY_PAIRS}, bites={p: 0 for p in READY_PAIRS},
                                  branches=seen, hinted=0, events=0, deadlines=[d], successes=[])
    unlisted, held = np.zeros(0, np.int64), [(np.zeros(0, np.uint32), np.zeros(0, np.uint32))] * 2
    for r in range(TICKS):
        now, where = origin + TICK_MS * r, "%s, %d nodes, round %d" % (point, P, r)
        cap = SHORT if r % 7 == SHORT_AT else G
        eo, epo, no = orc.timers_expired_epochs(now, capacity=cap)
        if gpu is not None:
            eg, epg, ng = gpu.timers_expired_epochs(now, capacity=cap)
            assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo), where
        assert np.all(np.diff(eo.astype(np.int64)) > 0) and np.all(d[eo] > 0) and np.all(d[eo] <= now) and no == np.count_nonzero((d > 0) & (d <= now)), where
        stats.late += int(np.count_nonzero(np.isin(eo, unlisted)))          # a ticket a short buffer left unlisted fires in the next call
        unlisted = np.setdiff1d(np.flatnonzero((d > 0) & (d <= now)), eo)
        assert len(unlisted) == no - len(eo)
        stats.fired, stats.fired_rounds = stats.fired + len(eo), stats.fired_rounds + (len(eo) > 0)
        d = _same_timers(gpu, orc, where + " after the expiry")
        assert np.all(d[eo] == -1) and np.all(d[unlisted] > 0)
        cur = orc.read_state()
        b = abi.Batch(1, G)
        fz.round(cur, b, 0)
        late_g, late_e = held.pop(0)                          # every third fired ticket gets its onTimeout two rounds late: until then its group's rows meet
        held.append((eo[eo % 3 == 0], epo[eo % 3 == 0]))      # the fired ticket (RaftRoutine.resetTimer leaves it alone), and the fence may have moved on
        for g, e in zip(np.concatenate([eo[eo % 3 != 0], late_g]), np.concatenate([epo[eo % 3 != 0], late_e])):      # onTimeout, fenced
            b.head[int(g)] = (int(abi.hdr_make(abi.EV_TIMEOUT)), int(e))
        assert abi.batch_fits_32(b)
        stats.events += int(np.count_nonzero(b.head["hdr"] & 0xF))
        if gpu is not None:
            if compact:
                raw = gpu.submit32c(engine.pack32(b), fill=0xAB)
                got, _ = engine.unpack32(raw, 1, G, cur.role_epoch)
            else:
                got = gpu.submit(b, fill=0xAB)
            bad = np.flatnonzero(got.status == abi.NEED_HOST)
            stats.hinted += T._resolve_need_host(gpu, orc, b, got, cur)
            if compact:
                gpu.timers_update32(1, raw, [now])
                gpu.health_update32(b, raw, [now])
                if len(bad):                                  # (the repaired rows, folded like the others: what tick2_case does)
                    gpu.timers_update(1, len(bad), got.reply[bad], [now], gid=bad.astype(np.uint32))
                    gpu.health_update(T._subset(b, bad, bad.astype(np.uint32)), got.reply[bad], [now])
            else:
                gpu.timers_update(1, G, got.reply, [now])
                gpu.health_update(b, got.reply, [now])
        oo = orc.submit(b, fill=0xAB, now=[now])
        if gpu is not None:
            compare_outcomes(oo, got, where)
        orc.timers_update(1, G, oo.reply, [now])
        after = _same_timers(gpu, orc, where + " after the update")
        check_rearm(d, after, oo.reply["flags"], now, seen, where)
        d = after
        _same_health(gpu, orc, where + " after the update")
        n = int(rng.integers(0, G // 2))                      # RPC errors / timeouts, repeats of a (group, follower) and the self slot included
        fg, fs, ff = rng.integers(0, G, n).astype(np.uint32), rng.integers(0, P, n).astype(np.uint8), rng.integers(0, 4, n).astype(np.uint8)
        leaders = np.flatnonzero(orc.read_state().role == abi.LEADER)      # ... and every fourth round a burst at the leaders: unreachable followers, so that
        burst = rng.random((len(leaders), P)) < (0.25 if r % 4 == 1 else 0.0)      # recentFailure passes a critical point before the next success clears it
        lg, ls = np.nonzero(burst)
        fg, fs = np.concatenate([fg, leaders[lg].astype(np.uint32)]), np.concatenate([fs, ls.astype(np.uint8)])
        ff = np.concatenate([ff, np.ones(len(lg), np.uint8)])
        for t in (gpu, orc):
            if t is not None:
                t.health_failure(fg, fs, ff, now + 7)
        h = _same_health(gpu, orc, where + " after the failures")
        stats.deadlines.append(d)
        stats.successes.append(h[0])
        hb, fl = (rng.random(G) < 0.5).astype(np.uint8), rng.integers(0, 24, (G, P - 1)).astype(np.uint16)
        ho, so = orc.replicate(None, hb, fl)
        if gpu is not None:
            hg, sg = gpu.replicate(None, hb, fl)
            need = sg["kind"] == abi.SEND_NEED_HOST           # (a cache miss: the host would look prevLogTerm up itself)
            assert np.array_equal(hg, ho), where
            for f in ("prev_index", "last_index", "count"):
                assert np.array_equal(sg[f], so[f]), (where, f)
            assert np.array_equal(sg["kind"][~need], so["kind"][~need]) and np.array_equal(sg["prev_term"][~need], so["prev_term"][~need]), where
            compare_states(orc.read_state(), gpu.read_state(), where)
        plain = None
        for cp, cd in READY_PAIRS:
            ro = orc.ready(now + 20, cp, cd)
            if gpu is not None:
                assert np.array_equal(gpu.ready(now + 20, cp, cd), ro), (where, cp, cd)
            plain = ro if plain is None else plain
            stats.ready[(cp, cd)] += np.bincount(ro, minlength=2)[:2]
            stats.bites[(cp, cd)] += int(np.count_nonzero((plain == 1) & (ro == 0)))      # the health criterion alone turned a ready group away
    for t in (gpu, orc):
        if t is not None:
            t.close()
    return stats


@functools.lru_cache(maxsize=None)
def lead(point, P):
    """the oracle's run of loop(point, P), once: the reach statistics and the columns crossing() looks at"""
    return loop(point, P, device=False)


def check_reach(point, P, st):
    """the reach conditions of a stand-alone loop, on the oracle's run alone"""
    where = "%s, %d nodes" % (point, P)
    crossing(point, np.concatenate(st.deadlines), np.concatenate([s.reshape(-1) for s in st.successes]), where)
    assert st.fired_rounds * 2 >= TICKS and st.fired * 4 >= G_LOOP, (where, st.fired_rounds, st.fired)
    assert st.late > 0, (where, "no ticket was left unlisted by a short buffer and fired in the next call")
    for pair in READY_PAIRS:
        assert st.ready[pair][0] and st.ready[pair][1], (where, pair, st.ready[pair])
        if pair != (0, 0):
            assert st.bites[pair] > 0, (where, pair, "no ready group was turned away by its followers' health")
    missing = [b for b in BRANCHES if not st.branches[b]]
    assert not missing, (where, missing, st.branches)


def loop_case(point, P, compact):
    want = lead(point, P)
    check_reach(point, P, want)                               # (on the oracle's columns, before any kernel is compared)
    got = loop(point, P, compact=compact)
    print("%s, %d nodes, %s rows: %d of %d event rows answered through the hint protocol, %d tickets fired" % (
        point, P, "compact" if compact else "wide", got.hinted, got.events, got.fired))
    assert got.fired == want.fired and got.branches == want.branches and got.events == want.events
    assert got.hinted * 50 <= got.events, "%d of %d rows were not decided by the launch (cap: 2 %%)" % (got.hinted, got.events)
    return got


def low_word_case(device=True):
    """At cross32: the same table armed at `now` and at `now + 2^32` — two clocks that differ in bit 32 alone. A hash that takes the low word of `now` gives
    every group the same draw twice; the oracle's draws differ (shown first), and the device must give the oracle's."""
    G, P, now = G_LOOP, 3, POINTS["cross32"] + 400
    assert (now ^ (now + (1 << 32))) == 1 << 32
    st0 = make_state(P, G, role=abi.FOLLOWER, term=3)
    draws = []
    for at in (now, now + (1 << 32)):
        orc = oracle_lib.OracleTable(G, P, 0, True)
        gpu = engine.Table(G, P, 0, True) if device else None
        for t in (gpu, orc):
            if t is not None:
                t.load_state(st0)
                t.timers_configure(E_MS, HB_MS, TIMER_SEED)
                t.timers_arm(at)
        d = _same_timers(gpu, orc, "armed at %d" % at)
        assert np.all(d >= at + E_MS) and np.all(d <= at + 2 * E_MS)
        draws.append(d - at)
        for t in (gpu, orc):
            if t is not None:
                t.close()
    same = int(np.count_nonzero(draws[0] == draws[1]))
    assert same * 20 < G, "%d of %d groups draw the same timeout at two clocks that differ in bit 32" % (same, G)      # (uniform over 901 values: ~0.3 expected)


# ---- 2. the recorded ticks, through the case functions that exist ---------------------------------------------------------------------------------------------------
TICK_CASES = {
    "dense": lambda: T.tick2_case(G=G_TICK, P=5, ticks=TICKS, seed=821),
    "dense_two_nodes": lambda: T.tick2_case(G=G_TICK, P=5, ticks=TICKS, seed=822, nodes=2),
    "dense_four_nodes": lambda: T.tick2_case(G=G_TICK, P=5, ticks=TICKS, seed=823, nodes=4),
    "dense_resident": lambda: T.tick2_case(G=G_TICK, P=5, ticks=TICKS, seed=824, device_resident=True),
    "dense_nine_nodes": lambda: T.tick2_case(G=G_TICK, P=9, ticks=TICKS, seed=829),
    "sparse": lambda: S.sparse_tick_case(G_TICK, 845, TICKS, P=5, expect_all=False),
    "sparse_rounds": lambda: X.rounds_tick_case(G_TICK, 865, TICKS, P=5, expect_all=False),
    "in_flight": lambda: I.lockstep_case(G_TICK, 5, 885, TICKS, expect_all=False),
    "assembled": lambda: A.assembled_tick_case(G_TICK, 895, TICKS, P=5, expect_all=False),
    "once_per_tick": lambda: T.tick_path_case(G=G_TICK, P=5, ticks=TICKS),
}
CLOCKLESS = ("once_per_tick",)                                # (rg_tick_*: the step alone, no clock travels; kept so that every recording runs under every origin)


def tick_case(point, name, origin=None):
    """one existing tick case with every clock of it moved to the point's origin; what the oracle's columns held is then held to crossing()"""
    with clock.at(POINTS[point] if origin is None else origin), K.routed(None), watching() as w:
        TICK_CASES[name]()
    if name not in CLOCKLESS:
        assert w.deadlines and w.successes, name
        crossing(point, np.concatenate(w.deadlines), np.concatenate([s.reshape(-1) for s in w.successes]), name)
    return w


# ---- 3. directed boundaries: literal expected values, and the oracle -----------------------------------------------------------------------------------------------
def _pair(G, P, st, arm=None):
    gpu, orc = engine.Table(G, P, 0, True), oracle_lib.OracleTable(G, P, 0, True)
    for t in (gpu, orc):
        t.load_state(st)
        t.timers_configure(E_MS, HB_MS, TIMER_SEED)
        if arm is not None:
            t.timers_arm(arm)
    return gpu, orc


def _expire(gpu, orc, now, where):
    eg, epg, ng = gpu.timers_expired_epochs(now)
    eo, epo, no = orc.timers_expired_epochs(now)
    assert ng == no and np.array_equal(eg, eo) and np.array_equal(epg, epo), where
    return eg.astype(np.int64)


def _reply_rows(G, rows):
    """hand-made reply rows: {group: (flags, role epoch)}; every other row carries no flag"""
    rep = np.zeros(G, dtype=abi.REPLY_DT)
    for g, (flags, epoch) in rows.items():
        rep["flags"][g], rep["role_epoch"][g] = flags, epoch
    return rep


def timer_boundaries_case(O):
    """the deadline column at its marks and at deadline == now, on 130 groups at clock origin O"""
    G, P, LEADERS = G_TICK, 3, 10
    role = lambda r: np.uint32(r << abi.F_ROLE_SHIFT)        # noqa: E731
    st = make_state(P, G, role=abi.FOLLOWER, term=5, role_epoch=2)
    st.role[:LEADERS] = abi.LEADER
    gpu, orc = _pair(G, P, st)
    assert len(_expire(gpu, orc, NOW_MAX, "never armed")) == 0            # deadline == 0 (never armed): never fires, at any clock of the domain
    assert not _same_timers(gpu, orc, "never armed").any()
    for t in (gpu, orc):
        t.timers_arm(O)
    d = _same_timers(gpu, orc, "armed")
    assert np.all(d[:LEADERS] == O)                                        # Leader, no ticket: now
    assert np.all(d[LEADERS:] >= O + E_MS) and np.all(d[LEADERS:] <= O + 2 * E_MS)
    a = LEADERS + int(np.argmin(d[LEADERS:]))                              # the follower whose ticket comes first
    fired = _expire(gpu, orc, int(d[a]) - 1, "deadline == now + 1")
    assert fired.tolist() == list(range(LEADERS))                          # deadline == now + 1: does not fire (the leaders' tickets, at O, do)
    assert int(_same_timers(gpu, orc, "deadline == now + 1")[a]) == int(d[a])
    fired = _expire(gpu, orc, int(d[a]), "deadline == now")
    assert a in fired and fired.tolist() == (np.flatnonzero(d[LEADERS:] == d[a]) + LEADERS).tolist()      # deadline == now: fires, the list holds it ...
    d1 = _same_timers(gpu, orc, "deadline == now")
    assert int(d1[a]) == -1 and np.all(d1[:LEADERS] == -1)                 # ... and the column reads -1
    now, ep = int(d[a]) + 5, 7
    RESET, CHANGED, MUTED = abi.F_RESET_TIMER, abi.F_ROLE_CHANGED, abi.F_TIMER_MUTED
    quiet = [int(g) for g in np.flatnonzero(d1 > 0)[:3]]                   # three followers whose tickets have not fired
    m, l1, l2 = quiet
    rows = {0: (RESET | role(abi.FOLLOWER), ep),                           # a follower row with RESET_TIMER and a fired ticket: stays -1
            1: (RESET | CHANGED | role(abi.FOLLOWER), ep),                 # the same row with ROLE_CHANGED: re-armed in [now + E, now + 2E]
            2: (RESET | MUTED | role(abi.CANDIDATE), ep),                  # muted, but the fired ticket stays
            m: (RESET | MUTED | role(abi.FOLLOWER), ep),                   # muted: INT64_MAX
            l1: (RESET | CHANGED | role(abi.LEADER), ep),                  # a new Leader: no ticket -> now
            l2: (RESET | role(abi.LEADER), ep)}                            # Leader with a ticket -> now + heartbeat_ms
    rep = _reply_rows(G, rows)
    for t in (gpu, orc):
        t.timers_update(1, G, rep, [now])
    d2 = _same_timers(gpu, orc, "directed rows")
    assert int(d2[0]) == -1 and now + E_MS <= int(d2[1]) <= now + 2 * E_MS and int(d2[2]) == -1
    assert int(d2[m]) == INT64_MAX and int(d2[l1]) == now and int(d2[l2]) == now + HB_MS
    untouched = np.setdiff1d(np.arange(G), list(rows))
    assert np.array_equal(d2[untouched], d1[untouched])
    rep = _reply_rows(G, {l1: (RESET | role(abi.LEADER), ep)})             # ... and the new Leader's next keep-alive: a ticket now
    for t in (gpu, orc):
        t.timers_update(1, G, rep, [now + 3])
    d3 = _same_timers(gpu, orc, "keep-alive")
    assert int(d3[l1]) == now + 3 + HB_MS
    fired = _expire(gpu, orc, NOW_MAX, "the top of the domain")           # every ticket fires at the top of the domain but: muted, fired, (none unarmed here)
    want = np.flatnonzero((d3 > 0) & (d3 < INT64_MAX))
    assert fired.tolist() == want.tolist() and m not in fired and 0 not in fired and 2 not in fired
    d4 = _same_timers(gpu, orc, "the top of the domain")
    assert int(d4[m]) == INT64_MAX and int(d4[0]) == -1 and np.all(d4[want] == -1)      # muted: never fires; fired: stays -1
    assert len(_expire(gpu, orc, NOW_MAX, "nothing left")) == 0
    gpu.close()
    orc.close()


def health_boundaries_case(O):
    """Leadership.State.isHealthy at its two thresholds and the monotone clocks of statSuccess / statFailure, 130 leader groups of a 3-node cluster: only
    follower 1 ever succeeds, so a group is ready iff that follower is healthy (1 + 1 > 2 / 2)."""
    G, P = G_TICK, 3
    st = make_state(P, G, role=abi.LEADER, term=5, voted_for=0, role_epoch=3, repl_prepared=1, log=simple_log(50, 5), peers=[(0, 51, 0, 0, 0)] * 2)
    gpu, orc = _pair(G, P, st)
    cls = np.arange(G) % 5                                    # 0: cool-down, 1: recentFailure == critical_point, 2: one above, 3: no success at all, 4: clocks run backwards
    t0, tf, CD, CP = O + 100, O + 500, 60, 2
    big = abi.Batch(2, G)
    for g in range(G):
        if cls[g] != 3:
            big.put(0, g, abi.EV_AE_ACK, slot=1, flag=1, a=5, b=0, c=40, aux=3)
        if cls[g] == 4:
            big.put(1, g, abi.EV_AE_ACK, slot=1, flag=1, a=5, b=0, c=45, aux=3)
    nows = [t0 + 50, t0 + 20]                                 # the second round's clock runs behind the first's
    og = gpu.submit(big, fill=0xAB)
    gpu.health_update(big, og.reply, nows)
    compare_outcomes(orc.submit(big, fill=0xAB, now=nows), og, "acks")
    assert np.all(og.status[:G][cls != 3] == abi.OK) and np.all(og.status[G:][cls == 4] == abi.OK)
    ok, fail, recent = _same_health(gpu, orc, "acks")
    assert np.all(ok[cls != 3, 0] == t0 + 50) and not ok[cls == 3].any() and not ok[:, 1].any()      # requestSuccess keeps its maximum
    sel = lambda c: np.flatnonzero(cls == c).astype(np.uint32)      # noqa: E731
    one = lambda g: np.ones(len(g), np.uint8)                # noqa: E731
    calls = [(sel(0), 0, tf), (sel(1), 1, tf), (sel(1), 1, tf), (np.repeat(sel(2), 3), 1, tf),      # (repeats of a pair within one call)
             (sel(3), 1, tf), (sel(4), 0, tf + 30), (sel(4), 0, tf)]                               # class 4: the second failure's clock runs behind
    for gids, flag, at in calls:
        for t in (gpu, orc):
            t.health_failure(gids, one(gids), one(gids) * flag, at)
    ok, fail, recent = _same_health(gpu, orc, "failures")
    assert np.all(fail[cls == 4, 0] == tf + 30) and np.all(fail[cls < 4, 0] == tf) and not fail[:, 1].any()      # requestFailure keeps its maximum
    assert recent[:, 0].tolist() == [(0, 2, 3, 1, 0)[c] for c in cls] and np.all(ok[cls != 3, 0] == t0 + 50)

    def ready(now, cp, cd):
        got, want = gpu.ready(now, cp, cd), orc.ready(now, cp, cd)
        assert np.array_equal(got, want), (now, cp, cd)
        return got
    r = ready(tf + CD, 0, CD)                                 # now - requestFailure == cool_down: healthy
    assert np.all(r[cls == 0] == 1) and np.all(r[cls == 3] == 0) and np.all(r[cls == 4] == 0)      # (class 4 failed 30 ms later; class 3 never succeeded)
    r = ready(tf + CD - 1, 0, CD)                             # ... == cool_down - 1: unhealthy
    assert np.all(r[cls == 0] == 0)
    r = ready(tf + 30 + CD, 0, CD)
    assert np.all(r[cls == 4] == 1)
    r = ready(tf + 10 ** 6, CP, 0)                            # recentFailure == critical_point: healthy; one above: unhealthy; requestSuccess == 0: never ready
    assert np.all(r[cls == 1] == 1) and np.all(r[cls == 2] == 0) and np.all(r[cls == 0] == 1) and np.all(r[cls == 3] == 0)
    for cp, cd in READY_PAIRS:
        assert not ready(NOW_MAX, cp, cd)[cls == 3].any()
    r = ready(NOW_MAX, 3, 10 ** 9)                            # the top of the domain: now - requestFailure is huge, nothing wraps
    assert np.all(r[cls != 3] == 1)
    gpu.close()
    orc.close()


def boundaries_case(origin):
    timer_boundaries_case(origin)
    health_boundaries_case(origin)


# ---- 4. the quorum of ready_of at every cluster size ------------------------------------------------------------------------------------------------------------------
def quorum_case(P, pending=False, origin=POINTS["epoch_ms"]):
    """64 leader groups of a P-node cluster; group g has exactly g mod (F + 1) followers with a success, in rotating positions; pending: the first of them has
    its pending-snapshot bit set. Leader.isReady's loop, written out: ready iff k >= 1 and 1 + k > F / 2 (integer division), k the followers that succeeded and
    are not pending. Through rg_ready and through the ready column of a dense tick."""
    G, F = 64, P - 1
    k = np.arange(G) % (F + 1)
    st = make_state(P, G, role=abi.LEADER, term=5, voted_for=0, role_epoch=3, repl_prepared=1, log=simple_log(50, 5), peers=[(0, 51, 0, 0, 0)] * F)
    if pending:
        for g in np.flatnonzero(k >= 1):
            st.peer_pending[g * F + g % F] = 1
    with K.routed(None):
        gpu = engine.Table(G, P, 0, True)
    orc = oracle_lib.OracleTable(G, P, 0, True)
    for t in (gpu, orc):
        t.load_state(st)
        t.timers_configure(E_MS, HB_MS, TIMER_SEED)
    big = abi.Batch(F, G)
    for g in range(G):
        for i in range(int(k[g])):
            big.put(i, g, abi.EV_AE_ACK, slot=1 + (g + i) % F, flag=1, a=5, b=0, c=40, aux=3)
    nows = [origin + 10 * i for i in range(F)]
    og = gpu.submit(big, fill=0xAB)
    gpu.health_update(big, og.reply, nows)
    compare_outcomes(orc.submit(big, fill=0xAB, now=nows), og, "%d nodes" % P)
    ok, _, _ = _same_health(gpu, orc, "%d nodes" % P)
    after = orc.read_state()
    compare_states(after, gpu.read_state(), "%d nodes" % P)
    assert np.array_equal(np.count_nonzero(ok, axis=1), k)
    if pending:                                               # (an AppendEntries ack does not end a pending installation)
        assert np.array_equal(after.peer_pending.reshape(G, F).sum(axis=1), (k >= 1).astype(np.int64))
    good = k - (pending & (k >= 1))
    want = ((good >= 1) & (1 + good > F // 2)).astype(np.uint8)
    assert (want.any() or (pending and P == 2)) and not want.all()      # (two nodes: the one follower is the pending one)
    now = origin + 10 * F + 1
    got = gpu.ready(now, 0, 0)
    assert np.array_equal(got, want), (P, pending, np.flatnonzero(got != want)[:8].tolist())
    assert np.array_equal(orc.ready(now, 0, 0), want)
    tick = engine.Tick2(gpu, 1, expired_cap=G, critical_point=0, cool_down_ms=0)
    tick.refill(abi.Batch(1, G), [now])
    tick.launch()
    tick.wait()
    col = tick.readiness()
    assert np.array_equal(col, want), (P, pending, "tick", np.flatnonzero(col != want)[:8].tolist())
    tick.close()
    gpu.close()
    orc.close()


# ---- 5. more than 64 rounds in one call -------------------------------------------------------------------------------------------------------------------------------
LONG_ROUNDS, LONG_MAX, CHUNK = (64, 65, 130), 130, 64
LONG_SEED = 4100
BACKWARDS = (40, 70)                                          # rounds whose clock runs behind the two before them


def long_nows(origin=POINTS["epoch_ms"]):
    nows = [origin + 37 * r for r in range(LONG_MAX)]
    for r in BACKWARDS:
        nows[r] -= 100
    assert len(set(nows)) == LONG_MAX and all(nows[r] < nows[r - 2] for r in BACKWARDS)
    return nows


@functools.lru_cache(maxsize=None)
def long_lead():
    """the oracle's half: LONG_MAX rounds of fuzzed traffic at epoch_ms, one clock per round, decided and folded round by round"""
    G, P, seed, nows = G_TICK, 5, LONG_SEED, long_nows()
    st0 = fuzz.random_initial_state(G, P, 1, seed)
    orc = oracle_lib.OracleTable(G, P, 1, True)
    orc.load_state(st0)
    orc.timers_configure(E_MS, HB_MS, TIMER_SEED)
    orc.timers_arm(nows[0])
    fz = fuzz.Fuzzer(G, P, 1, seed, allow_miss=False)
    states, batches, outs, timers, health = [], [], [], [], []
    for r in range(LONG_MAX):
        cur = orc.read_state()
        b = abi.Batch(1, G)
        fz.round(cur, b, 0)
        assert abi.batch_fits_32(b)
        oo = orc.submit(b, fill=0xAB, now=[nows[r]])
        orc.timers_update(1, G, oo.reply, [nows[r]])
        states.append(cur)
        batches.append(b)
        outs.append(oo)
        timers.append(orc.timers_read())
        health.append(orc.health_read())
    orc.close()
    flags = np.stack([o.reply["flags"] for o in outs])       # [round][group]
    return types.SimpleNamespace(G=G, P=P, st0=st0, nows=nows, states=states, batches=batches, outs=outs, timers=timers, health=health, flags=flags)


def long_reach(L, rounds):
    """-> the groups that convert in one of the last two rounds of the first chunk and draw an election timeout in a later chunk of the call with the role epoch
    that conversion left (no row of theirs in between carries RG_F_PERSIST): the carry from one launch to the next"""
    hit = []
    for g in range(L.G):
        for r in (CHUNK - 2, CHUNK - 1):
            if not L.flags[r, g] & abi.F_ROLE_CHANGED:
                continue
            for r2 in range(r + 1, rounds):
                f = int(L.flags[r2, g])
                if f & abi.F_PERSIST:                         # (the row may carry a role epoch of its own)
                    break
                if r2 >= CHUNK and f & abi.F_RESET_TIMER and rearm_branch(int(L.timers[r2 - 1][g]), f) == "draw":
                    hit.append(g)
                    break
    return sorted(set(hit))


def long_rounds_case(rounds, compact):
    """rg_timers_update + rg_health_update (compact: their ...32 forms) over `rounds` rounds in ONE call == the same rows one round per call == the oracle.
    The rows are those of fuzzed traffic at epoch_ms, decided by the device twice: in lockstep with the oracle (single-round launches of submit / submit32c, so
    that a row that answers RG_NEED_HOST stops nothing after it and every group can be compared), and in ONE multi-round launch at the end. The 32 forms read the device's raw compact rows: a group one of whose rows answered RG_NEED_HOST has
    that row's flags in no raw row, so against the ORACLE the 32 forms are compared on the other groups; chunked == per round holds for every group."""
    L = long_lead()
    G, P, nows = L.G, L.P, L.nows[:rounds]
    if rounds > CHUNK:
        assert long_reach(L, rounds), "no group carries a conversion of rounds 62 / 63 into a draw of a later chunk"
    assert np.any(np.diff(np.array(nows)) < 0)

    def table():
        t = engine.Table(G, P, 1, True)
        t.load_state(L.st0)
        t.timers_configure(E_MS, HB_MS, TIMER_SEED)
        t.timers_arm(nows[0])
        return t
    gpu, once, shadow = table(), table(), oracle_lib.OracleTable(G, P, 1, True)      # gpu: decides, folds round by round; once: folds all rounds in one call
    shadow.load_state(L.st0)                                  # (the host's log for the hint protocol)
    raws, gots, hinted = [], [], np.zeros(G, dtype=bool)
    for r in range(rounds):
        b, cur, where = L.batches[r], L.states[r], "round %d of %d" % (r, rounds)
        if compact:
            raw = gpu.submit32c(engine.pack32(b), fill=0xAB)
            got, _ = engine.unpack32(raw, 1, G, cur.role_epoch)
            raws.append(raw)
        else:
            got = gpu.submit(b, fill=0xAB)
        hinted |= got.status == abi.NEED_HOST
        T._resolve_need_host(gpu, shadow, b, got, cur)
        shadow.submit(b)
        compare_outcomes(L.outs[r], got, where)
        gots.append(got)
        if compact:
            gpu.timers_update32(1, raw, [nows[r]])
            gpu.health_update32(b, raw, [nows[r]])
        else:
            gpu.timers_update(1, G, got.reply, [nows[r]])
            gpu.health_update(b, got.reply, [nows[r]])
        clean = ~hinted if compact else np.ones(G, dtype=bool)
        assert np.array_equal(gpu.timers_read()[clean], L.timers[r][clean]), where
        for a, c in zip(gpu.health_read(), L.health[r]):
            assert np.array_equal(a[clean], c[clean]), where
    big = fuzz.concat_batches(L.batches[:rounds])
    if compact:
        all32 = abi.Outcome32(rounds * G, wide=False)
        all32.row, all32.persist = np.concatenate([x.row for x in raws]), np.concatenate([x.persist for x in raws])
        once.timers_update32(rounds, all32, nows)
        once.health_update32(big, all32, nows)
    else:
        reply = np.concatenate([x.reply for x in gots])
        once.timers_update(rounds, G, reply, nows)
        once.health_update(big, reply, nows)
    assert np.array_equal(once.timers_read(), gpu.timers_read()), "deadlines: %d rounds in one call != round by round" % rounds
    for name, a, c in zip(("requestSuccess", "requestFailure", "recentFailure"), once.health_read(), gpu.health_read()):
        assert np.array_equal(a, c), "%s: %d rounds in one call != round by round" % (name, rounds)
    # the epochs the calls left behind: a draw at one more clock hashes them (a row that resets a follower's timer and carries no RG_F_PERSIST)
    if compact:
        one = abi.Outcome32(G, wide=False)
        one.row["flags"] = abi.F_RESET_TIMER
        for t in (once, gpu):
            t.timers_update32(1, one, [nows[-1] + 1000])
        assert np.array_equal(once.timers_read(), gpu.timers_read()), "the role epochs %d rounds in one call left behind" % rounds
    clean = ~hinted if compact else np.ones(G, dtype=bool)
    print("%d rounds, %s rows: %d of %d groups had a row answered through the hint protocol" % (rounds, "compact" if compact else "wide", int(hinted.sum()), G))
    assert np.count_nonzero(clean) * 2 >= G
    if rounds > CHUNK and compact:
        assert any(clean[g] for g in long_reach(L, rounds))
    # the same stream decided by ONE multi-round launch (submit / submit32c over all the rounds) whose own rows are folded in one call. No host stands between
    # the rounds of a launch: a group that answers RG_NEED_HOST has its later rows skipped, so the launch is compared on the groups it decided to the end.
    multi = table()
    if compact:
        raw = multi.submit32c(engine.pack32(big), fill=0xAB)
        got, _ = engine.unpack32(raw, rounds, G, L.st0.role_epoch)
        multi.timers_update32(rounds, raw, nows)
        multi.health_update32(big, raw, nows)
    else:
        got = multi.submit(big, fill=0xAB)
        multi.timers_update(rounds, G, got.reply, nows)
        multi.health_update(big, got.reply, nows)
    st = got.status.reshape(rounds, G)
    went = ~((st == abi.NEED_HOST) | (st == abi.SKIPPED_AFTER_NEED_HOST)).any(axis=0)
    print("%d rounds, %s rows, one launch: %d of %d groups decided to the end" % (rounds, "compact" if compact else "wide", int(went.sum()), G))
    assert np.count_nonzero(went) * 2 >= G and (rounds <= CHUNK or any(went[g] for g in long_reach(L, rounds)))
    want = np.concatenate([o.reply for o in L.outs[:rounds]]).reshape(rounds, G)
    assert np.array_equal(got.reply.reshape(rounds, G)[:, went], want[:, went]), "the reply rows of one launch of %d rounds" % rounds
    assert np.array_equal(multi.timers_read()[went], L.timers[rounds - 1][went]), "deadlines after one launch and one call of %d rounds" % rounds
    for name, a, c in zip(("requestSuccess", "requestFailure", "recentFailure"), multi.health_read(), L.health[rounds - 1]):
        assert np.array_equal(a[went], c[went]), "%s after one launch and one call of %d rounds" % (name, rounds)
    for t in (gpu, once, multi, shadow):
        t.close()


# ---- 6. the expiry list at its capacities -------------------------------------------------------------------------------------------------------------------------------
EXPIRY_GROUPS = (1, 63, 64, 65, 257, 300)
SENTINEL = 0xABABABAB


def _expired_raw(gpu, now, capacity, epochs, device, room):
    """rg_timers_expired / rg_timers_expired_epochs into buffers of `room` >= capacity entries pre-filled with a sentinel -> (gids[room], epochs[room] or None, count)"""
    L, n = engine.lib(), engine.C.c_uint32()
    assert room >= capacity
    host_g, host_e = np.full(room, SENTINEL, np.uint32), np.full(room, SENTINEL, np.uint32)
    if device:
        dg, de = engine.DeviceBuffer.from_host(gpu, host_g), engine.DeviceBuffer.from_host(gpu, host_e)
        pg, pe = dg.ptr, de.ptr
    else:
        pg, pe = host_g.ctypes.data, host_e.ctypes.data
    mem = abi.MEM_DEVICE if device else abi.MEM_HOST
    if epochs:
        gpu._check(L.rg_timers_expired_epochs(gpu._h, now, pg, pe, capacity, engine.C.byref(n), mem))
    else:
        gpu._check(L.rg_timers_expired(gpu._h, now, pg, capacity, engine.C.byref(n), mem))
    if device:
        host_g, host_e = dg.to_host(np.uint32, room), de.to_host(np.uint32, room)
        dg.free()
        de.free()
    return host_g, (host_e if epochs else None), int(n.value)


def expiry_case(G, epochs, device, origin=POINTS["epoch_ms"]):
    """the three-pass expiry list at capacities 0, total - 1, total, total + 1 and G: the count is always the total; the list is the first min(capacity, total)
    expired groups in ascending order; exactly those read -1 afterwards; the buffer beyond is untouched; a second call at the same clock lists the rest."""
    P, seed = 3, 5000 + G
    st0 = fuzz.random_initial_state(G, P, 0, seed)
    now = origin + (E_MS + E_MS // 2 if G > 1 else 2 * E_MS)
    orc = oracle_lib.OracleTable(G, P, 0, True)               # what is due at `now`, from the oracle's deadlines and the rule written out
    orc.load_state(st0)
    orc.timers_configure(E_MS, HB_MS, TIMER_SEED)
    orc.timers_arm(origin)
    d = orc.timers_read()
    orc.close()
    due = np.flatnonzero((d > 0) & (d <= now))
    total = len(due)
    assert total >= min(G, 2) and (total < G or G == 1), (G, total)
    for cap in sorted({0, total - 1, total, total + 1, G} - {-1}):
        where = "G = %d, capacity %d of %d" % (G, cap, total)
        gpu, orc = _pair(G, P, st0, arm=origin)
        assert np.array_equal(_same_timers(gpu, orc, "armed"), d)
        k = min(cap, total)
        eo, epo, no = orc.timers_expired_epochs(now, capacity=cap)
        assert no == total and eo.tolist() == due[:k].tolist() and epo.tolist() == st0.role_epoch[due[:k]].tolist(), where
        room = max(cap, G) + 8
        gids, eps, n = _expired_raw(gpu, now, cap, epochs, device, room)
        assert n == total, (where, n)
        assert gids[:k].tolist() == due[:k].tolist() and np.all(gids[k:] == SENTINEL), where
        if epochs:
            assert eps[:k].tolist() == st0.role_epoch[due[:k]].tolist() and np.all(eps[k:] == SENTINEL), where
        d1 = _same_timers(gpu, orc, where)
        want = d.copy()
        want[due[:k]] = -1
        assert np.array_equal(d1, want), where
        gids, eps, n = _expired_raw(gpu, now, G, epochs, device, room)      # the rest, at the same clock
        assert n == total - k and gids[: total - k].tolist() == due[k:].tolist() and np.all(gids[total - k:] == SENTINEL), where
        if epochs:
            assert eps[: total - k].tolist() == st0.role_epoch[due[k:]].tolist() and np.all(eps[total - k:] == SENTINEL), where
        orc.timers_expired_epochs(now, capacity=G)
        d2 = _same_timers(gpu, orc, where + ", second call")
        assert np.all(d2[due] == -1) and np.array_equal(d2 == -1, np.isin(np.arange(G), due)), where
        gpu.close()
        orc.close()


# ---- 7. the default origin: the clocks the cases always had ----------------------------------------------------------------------------------------------------------
# sha256 over every clock the oracle is given (submit, timers_arm / _update / _expired*, health_failure, ready; in call order) by the runs below at the default
# origin, recorded from the case modules as they were while their clocks were literals
DEFAULT_LEAD_DIGEST = "9c4b4e53e9bad56d7c0f856bee00344f31f786fb769ac506041c4c2ee3d54029"
DEFAULT_DEVICE_DIGEST = "7ae68436df55379c1568ddf861461cbf7de95acd6c8b44cbb668792245187a89"


def default_origin_digest(device):
    """device=False: the oracle-only leads of the sparse-rounds, assembled and in-flight ticks; device=True: the tick cases themselves, small (the dense tick with
    its closing compact launch, the sparse tick, the sparse-rounds tick and stand-alone launch, the in-flight sequences and ticks)"""
    assert clock.origin() == clock.DEFAULT == 10_000
    with watching() as w:
        if not device:
            X.lead_only(G_TICK, 5, 865, 6)
            X.lead_only(G_TICK, 5, 866, 6, replicate=False)
            A.lead_only(G_TICK, 5, 895, 6)
            I.lead_only(G_TICK, 5, 885, 6)
        else:
            T.tick2_case(G=64, P=3, ticks=4, seed=1)
            S.sparse_tick_case(64, 2, 4, P=3, expect_all=False)
            S.same_as_dense_case(64, ticks=2)
            X.one_round_case(64, ticks=2)
            X.same_as_dense_case(64, ticks=2)
            A.standalone_case(64, 3, 4, 2)
            I.constructed_case()
            I.saturation_case()
            I.same_as_dense_case(64, ticks=2)
            I.one_round_case(64, ticks=2)
            I.option_off_case(G=64, ticks=2)
    assert len(w.clocks) > 20
    return clock_digest(w)
