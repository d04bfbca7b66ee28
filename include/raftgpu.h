/*
 * raftgpu.h — C-ABI of the MI355X batched multi-Raft decision engine (libraftgpu.so).
 *
 * This is the drop-in boundary for ONE path of curioloop/rafting: the per-RaftContext
 * EventLoop decision logic (io.lubricant.consensus.raft.context.**).  Everything the Java
 * host would bind through JNI is declared here with plain pointers and sizes; no C++ or
 * torch types appear in any signature.  Paths below are relative to
 *   /root/reference/src/main/java/io/lubricant/consensus/raft/
 *
 * What each entry point replaces
 * ------------------------------
 *   rg_table_create / rg_table_destroy
 *       ContextManager.buildContext + RaftContext.<init>/initialize
 *       (context/ContextManager.java:57-106, context/RaftContext.java:62-113): instead of one
 *       RaftContext object per group, ONE structure-of-arrays table of G groups in HBM.
 *   rg_load_state / rg_read_state
 *       StableLock.restore -> switchTo(Follower, term, ballot) (context/RaftContext.java:96-104),
 *       RaftLog.epoch()/last() (command/storage/RocksLog.java:112-119) and, for leaders,
 *       Leader.prepareReplication (context/member/Leader.java:30-50).
 *   rg_submit
 *       The EventLoop drain itself (support/EventLoopGroup.java:32-46): one row = one task that
 *       the reference would have run on a ContextLoop thread (or, for responses, on a Netty
 *       thread), i.e. one call of
 *         RaftParticipant.appendEntries / preVote / requestVote   (RaftParticipant.java:34-44)
 *         Leader.replicateLog response callbacks                  (member/Leader.java:174-188,218-237)
 *         Candidate.startElection / Follower.prepareElection tally callbacks
 *                                                                (member/Candidate.java:121-134, member/Follower.java:258-270)
 *         RaftParticipant.onTimeout                               (RaftParticipant.java:24)
 *         Leader.acceptCommand -> RaftLog.newEntry                (member/Leader.java:128-140, storage/RocksLog.java:82-89)
 *         RaftLog.flush                                           (storage/RocksLog.java:228-242)
 *       The reply row is the RaftResponse(term, success) (RaftResponse.java:8-24) plus the
 *       instructions the host-owned plugins (RaftLog, StableLock, timers) must carry out.
 *
 * Ordering contract: rows of one group are applied in (round, row) order — the only ordering
 * the reference EventLoop guarantees (one context is pinned to one loop thread,
 * support/EventLoopGroup.java:77-80).  Groups are independent.
 *
 * Error convention: functions return 0 on success, <0 on API misuse / HIP failure
 * (text via rg_last_error).  Reference protocol violations (AssertionError sites) are NOT API
 * errors: they are reported per row in rg_reply_t.flags status bits, bit-exactly as the
 * reference would have hit them (the handler dies, no reply is sent, earlier side effects stay).
 *
 * Environment knobs read by rg_table_create (experiments / tests only): RG_FAST=0 routes every row through the
 * general handlers (no fast-path tier); RG_SPLIT=1|0 forces the two-wavefront (decide + I/O) or the single-wavefront
 * step kernel instead of choosing per launch; RG_LANES=8|16|32|64 sets the raft groups per wavefront of the latter.
 *
 * Threading: a table is not re-entrant; one host thread + one HIP stream per table.  Different
 * tables (different GPUs) are fully independent.  No RCCL, no cross-table traffic.
 */
#ifndef RAFTGPU_H
#define RAFTGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_ABI_VERSION      6     /* 2: RG_EV_IS_REQ, RG_EV_TIMEOUT.aux fence, RG_F_TIMER_MUTED, rg_timers_expired_epochs, rg_submit_async(_packed), 48-byte rg_send_head_t
                                     3: rg_submit32 / rg_batch32_pack, RG_HDR_SAME_TERM in rg_batch32_t rows
                                     4: compact OUTCOME rows (rg_out32_t, rg_submit32c, rg_outcome32_unpack, RG_F_WIDE_VALUES); rg_table_option; the index base of the compact formats (rg_index_base_set)
                                     5: the device-resident tick on compact outcome rows: rg_timers_update32, rg_health_update32, rg_tick2_*; clusters of up to 15 nodes
                                     6: automatic index bases: RG_OPT_AUTO_INDEX_BASE, rg_index_base_advance / rg_index_base_advance32
                                        (still 6, new symbols only — nothing that existed changed: rg_submit32c_sparse, rg_tick2_rows_t, rg_tick2_create_sparse;
                                         then rg_submit32c_sparse_rounds, rg_tick2_rounds_t, rg_tick2_create_sparse_rounds: a list of groups with R rounds;
                                         then RG_OPT_COMPACT_ANY_CLUSTER: a new value of the option enum, no new symbol, no struct change;
                                         then RG_OPT_DEVICE_IN_FLIGHT: a new option value, rg_in_flight_read / rg_in_flight_set, RG_HEALTH_NO_REQUEST, and — with the option on
                                         only — a meaning for rg_send_head_t.reserved, which stays 0 without it) */
#define RG_MIN_CLUSTER      2     /* P: cluster size incl. self (RaftCluster.size()) */
#define RG_MAX_CLUSTER      15    /* (ABI 5; the slot field of a row header is 4 bits. Leadership.majorIndices sorts any number of followers, member/Leadership.java:116-130.)
                                     Every cluster size has the wide-row entry points (rg_submit, rg_submit_async). The compact formats (rg_submit32*, rg_submit_async_packed)
                                     and the ticks (rg_tick_*, rg_tick2_*) take clusters of up to RG_MAX_COMPACT_CLUSTER nodes as they are, and larger ones — up to
                                     RG_MAX_CLUSTER — for a table that has RG_OPT_COMPACT_ANY_CLUSTER; without the option they answer -1 for such a table. */
#define RG_MAX_COMPACT_CLUSTER 7  /* what the compact formats and the ticks take WITHOUT the option (unchanged by it) */
#define RG_TERM_RUNS        4     /* K: cached term runs of the log tail per group */
#define RG_NO_NODE          (-1)  /* Java null for a RaftCluster.ID */

/* ---- roles: class of RaftContext.participant() (context/RaftContext.java:169) ------------ */
enum { RG_FOLLOWER = 0, RG_CANDIDATE = 1, RG_LEADER = 2 };

/* ---- event kinds (rg_ev_head_t.hdr bits 0-3) ------------------------------------------------ */
enum {
    RG_EV_NONE          = 0,  /* row not addressed this round                                          */
    RG_EV_AE_REQ        = 1,  /* RaftParticipant.appendEntries       a=term b=prevLogIndex c=prevLogTerm d=leaderCommit
                                 slot=leaderId n=#entries aux=offset of entry terms in entry_terms[];
                                 entry k has index prevLogIndex+1+k (what Leader.replicateLog builds, member/Leader.java:192-212) */
    RG_EV_AE_ACK        = 2,  /* Leader AE response callback         a=result.term b=epoch.index at send c=lastIndex sent
                                 slot=responder flag=result.success aux=roleEpoch the request was sent under */
    RG_EV_IS_ACK        = 3,  /* Leader InstallSnapshot callback     a=result.term b=epoch.index at send, slot, flag, aux as AE_ACK */
    RG_EV_RV_REQ        = 4,  /* RaftParticipant.requestVote        a=term b=lastLogIndex c=lastLogTerm slot=candidateId */
    RG_EV_PV_REQ        = 5,  /* RaftParticipant.preVote            same fields */
    RG_EV_RV_REPLY      = 6,  /* Candidate.startElection callback    a=result.term slot=responder flag=result.success aux=roleEpoch */
    RG_EV_PV_REPLY      = 7,  /* Follower.prepareElection callback   same fields */
    RG_EV_TIMEOUT       = 8,  /* RaftParticipant.onTimeout (election timer for F/C, heartbeat tick for L).
                                 aux = role epoch of the participant whose ticket fired (rg_timers_expired_epochs reports it), or 0 =
                                 "whoever is current". The reference runs onTimeout only if ticket.participant() == context.participant()
                                 (context/RaftRoutine.java:70): a row whose aux names a replaced participant is RG_DROPPED_STALE_ROLE */
    RG_EV_CLIENT_APPEND = 9,  /* Leader.acceptCommand x n            n=#commands appended at currentTerm */
    RG_EV_LOG_FLUSH     = 10, /* RaftLog.flush(index, term)          a=index b=term (log compaction / snapshot install moved the epoch) */
    RG_EV_IS_REQ        = 11  /* RaftParticipant.installSnapshot    a=term b=lastIncludedIndex c=lastIncludedTerm slot=leaderId
                                 flag = what RaftContext.installSnapshot returns (context/RaftContext.java:270-278: the host downloads and
                                 applies the snapshot; the decision row only carries its verdict). The term checks, the assertion, the
                                 Follower refresh after a timeout and the timer handling are member/Follower.java:129-152 and
                                 member/RaftMember.java:61-66. After a successful install the host submits the RG_EV_LOG_FLUSH row. */
};
#define RG_EV_IS_REQ_DEFINED 1

#define RG_HDR_KIND(h)        ((uint32_t)(h) & 0xFu)
#define RG_HDR_SLOT(h)        (((uint32_t)(h) >> 4) & 0xFu)
#define RG_HDR_FLAG(h)        (((uint32_t)(h) >> 8) & 0x1u)
#define RG_HDR_HINT(h)        (((uint32_t)(h) >> 9) & 0x1u)
#define RG_HDR_N(h)           ((uint32_t)(h) >> 12)
#define RG_HDR_MAKE(kind, slot, flag, n) \
    (((uint32_t)(kind) & 0xFu) | (((uint32_t)(slot) & 0xFu) << 4) | (((uint32_t)(flag) & 1u) << 8) | ((uint32_t)(n) << 12))
#define RG_HDR_HINT_BIT       (1u << 9)
#define RG_HDR_SAME_TERM      (1u << 10)  /* rg_batch32_t rows only, RG_EV_AE_REQ with n >= 1: ALL n carried entries have the term held in `aux`
                                             (what a leader replicating its own term sends); entry_terms is not consulted for the row.
                                             Must be 0 in rg_batch_t rows. Bit 11 is reserved (0). */
#define RG_MAX_ENTRIES        ((1u << 20) - 1)   /* what the header field can carry */
#define RG_MAX_AE_ENTRIES     200u               /* what a row may carry: 4 x REPLICATE_LIMIT (member/Leadership.java:10; the reference never
                                                    ships more than REPLICATE_LIMIT per request, member/Leader.java:194). Larger -> RG_BAD_EVENT:
                                                    one lane walks the entries of its row, an oversized row would stall its whole wavefront */

/* ---- wire structs: structure-of-small-structs so every lane issues 16-byte accesses -------- */
typedef struct { uint32_t hdr; uint32_t aux; } rg_ev_head_t;       /*  8 B */
typedef struct { int64_t  x;   int64_t  y;   } rg_ev_pair_t;       /* 16 B: (a,b) / (c,d) / hints */

/* reply: always written for every row */
typedef struct {
    int64_t  resp_term;   /* RaftResponse.term (valid iff RG_F_REPLIED) */
    uint32_t flags;       /* RG_F_* | status << 16 */
    uint32_t role_epoch;  /* role epoch AFTER the row: tag the host must attach to RPCs it now emits */
} rg_reply_t;             /* 16 B */

/* log / commit effects: written iff flags & (RG_F_COMMIT | RG_F_LOG_APPEND | RG_F_LOG_TRUNC), or status NEED_HOST */
typedef struct {
    int64_t commit_index; /* RaftLog.lastCommitted() after the row (valid iff RG_F_COMMIT)                 */
    int64_t log_from;     /* first log index the host must (re)write from the request's entries, after
                             deleting [log_from, oldLast] when RG_F_LOG_TRUNC (RocksLog.truncate+append);
                             CLIENT_APPEND: index of the first new entry; NEED_HOST: the index whose term is needed */
} rg_logfx_t;             /* 16 B */

/* durable membership: written iff flags & RG_F_PERSIST — what RaftMember.<init> hands to
 * StableLock.persist(currentTerm, lastCandidate) BEFORE the reply may leave (member/RaftMember.java:25) */
typedef struct {
    int64_t term;
    int32_t voted_for;    /* peer slot or RG_NO_NODE */
    int32_t role;
} rg_persist_t;           /* 16 B */

/* reply.flags bits */
#define RG_F_SUCCESS      (1u << 0)   /* RaftResponse.success                                             */
#define RG_F_REPLIED      (1u << 1)   /* a RaftResponse is produced (requests only; absent when an assertion killed the handler) */
#define RG_F_PERSIST      (1u << 2)   /* >=1 role conversion happened: fsync (term, votedFor) before replying */
#define RG_F_ROLE_CHANGED (1u << 3)   /* participant object was replaced (RaftRoutine.convertTo)            */
#define RG_F_RESET_TIMER  (1u << 4)   /* handler re-armed the election timer (ctx.resetTimer / convertTo)   */
#define RG_F_COMMIT       (1u << 5)   /* markCommitted advanced commitIndex                                 */
#define RG_F_LOG_TRUNC    (1u << 6)   /* RaftLog.truncate(log_from) must run before the append              */
#define RG_F_LOG_APPEND   (1u << 7)   /* entries with index >= log_from must be written                     */
#define RG_F_EMIT_SHIFT   8           /* what the new/refreshed participant broadcasts                      */
#define RG_F_EMIT_MASK    (3u << 8)
#define RG_EMIT_NONE      0u
#define RG_EMIT_PREVOTE   1u          /* preVote(currentTerm+1, self, last|epoch)   member/Follower.java:223-279 */
#define RG_EMIT_REQVOTE   2u          /* requestVote(currentTerm, self, last|epoch) member/Candidate.java:90-143 */
#define RG_EMIT_HEARTBEAT 3u          /* Leader.onTimeout -> replicateLog(true)      member/Leader.java:120-126  */
#define RG_F_ROLE_SHIFT   10          /* role after the row                                                 */
#define RG_F_ROLE_MASK    (3u << 10)
#define RG_F_TIMER_MUTED  (1u << 12)  /* the handler left the election timer MUTED: it called resetTimer(this, true) (deadline = Long.MAX_VALUE,
                                         context/RaftRoutine.java:101-107) and returned or threw before the un-muting call — Follower.java:43 then
                                         the throw at :48-50, Follower.java:118 then the throw in logUpToDate, Follower.java:134 then :136-139.
                                         The timer does not fire until a later handler re-arms it. Only set together with RG_F_RESET_TIMER */
#define RG_F_WIDE_VALUES  (1u << 13)  /* rg_out32_t rows only: a value of this row does not fit int32 — the row's numbers are the low 32 bits only,
                                         the full ones are in the wide columns of rg_outcome32_t at the same row index (when the caller gave any) */
#define RG_F_STATUS_SHIFT 16
#define RG_F_STATUS(f)    (((f) >> RG_F_STATUS_SHIFT) & 0xFFu)
#define RG_F_EMIT(f)      (((f) & RG_F_EMIT_MASK) >> RG_F_EMIT_SHIFT)
#define RG_F_ROLE(f)      (((f) & RG_F_ROLE_MASK) >> RG_F_ROLE_SHIFT)

/* per-row status (reply.flags bits 16-23).  A_* = the reference throws at that site: the event
 * task dies (EventLoopGroup.java:40-44), NO reply is sent, side effects made before the throw stay. */
enum {
    RG_OK                       = 0,
    RG_A_TWO_LEADERS            = 1,   /* member/Follower.java:48-50   */
    RG_A_PREV_ZERO_MISMATCH     = 2,   /* member/Follower.java:179-181 */
    RG_A_EPOCH_TERM_MISMATCH    = 3,   /* member/Follower.java:184-186 */
    RG_A_IMPOSSIBLE_LOG         = 4,   /* member/Follower.java:199-204 */
    RG_A_COMMIT_ROLLBACK        = 5,   /* storage/RocksLog.java:101-103 (via Follower.java:80, Leader.java:265/269) */
    RG_A_LOG_NOT_CONTINUOUS     = 6,   /* storage/RocksLog.java:175-177,180-188 */
    RG_A_LEADER_SELF_AE         = 7,   /* member/Leader.java:71-73     */
    RG_A_SAME_TERM_LEADER       = 8,   /* member/Leader.java:79-81     */
    RG_A_LEADER_NOT_SELF_VOTE   = 9,   /* member/Leader.java:101-105   */
    RG_A_CAND_SELF_RV           = 10,  /* member/Candidate.java:53-55  */
    RG_A_CAND_NOT_SELF_VOTE     = 11,  /* member/Candidate.java:64-66  */
    RG_A_LEADER_UNCHANGED       = 12,  /* member/Membership.java:86-90 */
    RG_A_CAND_BALLOT            = 13,  /* member/Membership.java:103-105 */
    RG_A_MATCH_ROLLBACK         = 14,  /* member/Leadership.java:76-81 (AbstractMethodError) */
    RG_A_IMPOSSIBLE_REPLICATION = 15,  /* member/Leader.java:251-253 (unreachable after a sort; kept for completeness) */
    RG_NPE_MAJOR_NULL           = 16,  /* member/Leader.java:256-257,277-279: log.get(majorIndex)==null, caught+logged, no commit */
    RG_DROPPED_STALE_ROLE       = 17,  /* response to a fenced participant (transport/rpc/Async.java:157-171) */
    RG_NOT_LEADER               = 18,  /* command/RaftStub.java:79-91: command submitted to a non-leader */
    RG_FLUSH_OUT_OF_BOUNDS      = 19,  /* storage/RocksLog.java:230-233 (IndexOutOfBoundsException) */
    RG_A_INSTALL_BEFORE_AE      = 20,  /* member/RaftMember.java:61-66, member/Follower.java:138-139: installSnapshot with term >= currentTerm at a
                                          Leader/Candidate, or term > currentTerm at a Follower */
    RG_A_NO_DOWNGRADE           = 21,  /* context/RaftRoutine.java:170-172 (unreachable when every switch goes through trySwitch first, as it does
                                          under one-row-per-group serialisation; kept so every assertion site of the path has a code) */
    RG_NEED_HOST                = 32,  /* term-run cache miss: row NOT applied; host looks up the term of
                                          logfx.log_from in its RaftLog and resubmits the row with a hint */
    RG_SKIPPED_AFTER_NEED_HOST  = 33,  /* later round of a group that hit NEED_HOST in this launch: NOT applied */
    RG_BAD_EVENT                = 34,  /* malformed row (slot out of range / self, kind unknown, response
                                          whose epoch matches a role that cannot have sent it): NOT applied */
    RG_UNSUPPORTED_LOG_STATE    = 35   /* CLIENT_APPEND on an empty log whose epoch.index>0 (RocksLog.newEntry
                                          would write key 1 below the epoch, storage/RocksLog.java:83-84): NOT applied */
};

/* ---- batches -------------------------------------------------------------------------------- */
enum { RG_MEM_HOST = 0, RG_MEM_DEVICE = 1 };

typedef struct {
    uint32_t            rounds;       /* R >= 1; round r occupies rows [r*count, (r+1)*count)             */
    uint32_t            count;        /* rows per round. dense: == number of groups                       */
    const uint32_t     *gid;          /* NULL: dense, row i of every round addresses group i.
                                         else sparse: row -> group id, strictly ascending, rounds must be 1 */
    const rg_ev_head_t *head;         /* [rounds*count] */
    const rg_ev_pair_t *ab;           /* [rounds*count] fields a,b */
    const rg_ev_pair_t *cd;           /* [rounds*count] fields c,d */
    const int64_t      *entry_terms;  /* AE_REQ entry terms, addressed by head.aux; may be NULL if no row has n>0 */
    uint64_t            entry_count;  /* length of entry_terms; at most 2^29 per batch */
    const rg_ev_pair_t *hint;         /* optional [rounds*count]; consulted only for rows with RG_HDR_HINT_BIT:
                                         AE_REQ: x = term of the host log at prevLogIndex (-1 = no such entry),
                                                 y = RaftLog.conflict(entries).index() (0 = none)
                                         AE_ACK: x = index, y = term of the host log at that index (-1 = none) */
} rg_batch_t;

typedef struct {
    rg_reply_t   *reply;    /* [rounds*count], required */
    rg_logfx_t   *logfx;    /* [rounds*count], required */
    rg_persist_t *persist;  /* [rounds*count], required */
} rg_outcome_t;

/* ---- group state exchange (host SoA, one element per group unless noted) -------------------- */
typedef struct {
    int64_t  *current_term;    /* RaftMember.currentTerm                                     */
    int32_t  *voted_for;       /* RaftMember.lastCandidate as peer slot, RG_NO_NODE = null    */
    int32_t  *role;            /* RG_FOLLOWER / RG_CANDIDATE / RG_LEADER                      */
    int32_t  *current_leader;  /* Follower.currentLeader                                      */
    uint8_t  *timeout_detected;/* Follower.timeoutDetected                                    */
    uint8_t  *repl_prepared;   /* Leader.followerStatus != null                               */
    uint32_t *role_epoch;      /* identity of the participant object / its AsyncHead          */
    int32_t  *votes;           /* AtomicInteger votes of the running (pre-)election           */
    uint32_t *elected_epoch;   /* role epoch of the Candidate whose election head stayed un-aborted after it won (0 = none) */
    int64_t  *elected_term;
    int64_t  *commit_index;    /* RocksLog.commitIndex                                        */
    int64_t  *epoch_index;     /* RaftLog.epoch()                                             */
    int64_t  *epoch_term;
    int64_t  *first_index;     /* smallest key stored (epoch.index or epoch.index+1); ignored when log empty */
    int64_t  *last_index;      /* RaftLog.last().index(); log empty <=> run_count == 0        */
    uint32_t *run_count;       /* number of term runs supplied (device keeps the newest RG_TERM_RUNS) */
    uint32_t *run_offset;      /* start of this group's runs in run_start/run_term            */
    int64_t  *run_start;       /* [sum run_count] ascending start index of each maximal equal-term run */
    int64_t  *run_term;
    /* per (group, follower j) with j = slot<self ? slot : slot-1, array index g*(P-1)+j (Leadership.State) */
    int64_t  *peer_last_epoch;
    int64_t  *peer_next_index;
    int64_t  *peer_match_index;
    int32_t  *peer_rejection;  /* recentRejection */
    uint8_t  *peer_pending;    /* pendingInstallation */
} rg_group_state_t;

typedef struct rg_table rg_table_t;

/* ---- life cycle ----------------------------------------------------------------------------- */
int         rg_abi_version(void);
/* device: HIP device ordinal. groups: G. cluster: P (self included). self_slot in [0,P). pre_vote: RaftConfig.preVote(). */
int         rg_table_create(int device, uint32_t groups, uint32_t cluster, uint32_t self_slot,
                            int pre_vote, rg_table_t **out);
int         rg_table_destroy(rg_table_t *t);
const char *rg_last_error(const rg_table_t *t);      /* t may be NULL for create failures */
/* Table options. RG_OPT_REQUIRE_FENCED_TIMEOUTS (default 0): with 1, an RG_EV_TIMEOUT row whose aux is 0 ("whoever is current") is refused as
 * RG_BAD_EVENT instead of being resolved against the participant of the moment. The reference's timer thread checks ticket.participant() ==
 * context.participant() BEFORE the event loop sees the task (context/RaftRoutine.java:65-77); a serial engine can only reproduce that when the
 * row names the participant whose ticket fired (rg_timers_expired_epochs supplies it) — the ordering contract of INTEGRATION.md section 1,
 * enforced instead of merely stated. The C++ host's IngressFlusher turns it on. */
enum { RG_OPT_REQUIRE_FENCED_TIMEOUTS = 1,
       RG_OPT_AUTO_INDEX_BASE = 2,          /* (ABI 6) value = the window W of the automatic index bases: 0 = off (default), 1 <= W < 2^30 = on, anything else -1.
                                               See "THE INDEX BASE OF THE COMPACT FORMATS" below. Switching it on or off bumps what a recorded tick has baked in:
                                               rg_tick_launch / rg_tick2_launch of an earlier recording then refuse (-1). Recommended window: 2^28. */
       RG_OPT_COMPACT_ANY_CLUSTER = 3,      /* value 0 (default): the compact formats and the ticks refuse a table of more than RG_MAX_COMPACT_CLUSTER nodes (-1, "wide rows").
                                               value 1: they take the table's cluster size, whatever it is (2 .. RG_MAX_CLUSTER): rg_submit32, rg_submit32c, rg_submit32c_sparse,
                                               rg_submit32c_sparse_rounds, rg_submit_async_packed, rg_tick_create, rg_tick2_create, rg_tick2_create_sparse,
                                               rg_tick2_create_sparse_rounds — same rows, same outcomes, bit-identical to the wide-row entry points. Any other value: -1.
                                               A table of up to RG_MAX_COMPACT_CLUSTER nodes is decided by the same kernels with the option on or off. Switching it bumps
                                               what a recorded tick has baked in, like the other options: a recording made under one setting refuses to launch under the
                                               other. COST at 8 .. 15 nodes: the compact-row kernels keep one matchIndex per follower in registers and one record per
                                               follower in LDS (25 KB per workgroup at 7 followers, 38 KB at 14), so fewer workgroups share a CU than at 5 nodes: three
                                               wavefronts per SIMD at 8 followers, two at 14. Its rate against the wide-row kernels has NOT been measured yet (DESIGN.md
                                               section 6, "Compact rows above 7 nodes", names the measurement): until it is, the option buys the formats and the ticks,
                                               not a known speed. The C++ ingress / flusher and the Java row packer do not set the option. */
       RG_OPT_DEVICE_IN_FLIGHT = 4 };       /* value 0 (default): nothing changes anywhere — the send step of a tick reads the caller's heartbeat[] / in_flight[] columns.
                                               value 1: the table keeps State.requestInFlight (member/Leadership.java:31) itself, one uint16_t per (follower, group), laid out
                                               like the health columns, zero when the option is switched on (switching it off drops the counts), and the send step of a recorded
                                               tick needs no host column: see "THE SEND STEP WITH DEVICE-RESIDENT IN-FLIGHT COUNTS" at rg_tick2_io_t. rg_load_state zeroes the
                                               counts of the groups it loads, as it resets their health; rg_health_failure takes the failed requests off; rg_in_flight_read /
                                               rg_in_flight_set read and write them. rg_replicate is unchanged: it keeps its explicit columns and never touches the counts.
                                               Any other value: -1. Like every option it is part of a recording: rg_tick2_launch refuses a tick recorded before it changed.
                                               The C++ ingress / flusher, the JNI shim and the Java packer do not set it. */
int         rg_table_option(rg_table_t *t, int option, int value);
uint32_t    rg_table_groups(const rg_table_t *t);
uint32_t    rg_table_cluster(const rg_table_t *t);

/* ---- state ---------------------------------------------------------------------------------- */
/* Load groups [first, first+count). Arrays are indexed from 0 for group `first`. Runs beyond the
 * newest RG_TERM_RUNS are not cached (lookups into them answer RG_NEED_HOST). */
int rg_load_state(rg_table_t *t, uint32_t first, uint32_t count, const rg_group_state_t *src);
/* Read groups back. run arrays must hold count*RG_TERM_RUNS elements; run_offset[i] is set to i*RG_TERM_RUNS. */
int rg_read_state(rg_table_t *t, uint32_t first, uint32_t count, rg_group_state_t *dst);

/* ---- the hot path --------------------------------------------------------------------------- */
/* memspace RG_MEM_HOST: caller-owned host buffers (ideally from rg_host_alloc), staged over PCIe and copied back,
 * synchronous; logfx/persist rows that are not flagged valid come back zeroed. Sparse gid lists are validated.
 * memspace RG_MEM_DEVICE: all pointers are device pointers (rg_dev_alloc or any hipMalloc memory on
 * the table's device); the launch is asynchronous on the table's stream — call rg_sync. Unflagged logfx/persist
 * rows keep their previous content; a sparse gid list is trusted (it cannot be inspected from the host). */
int rg_submit(rg_table_t *t, const rg_batch_t *in, const rg_outcome_t *out, int memspace);
int rg_sync(rg_table_t *t);

/* The host-memory path, PIPELINED. rg_submit(RG_MEM_HOST) is one synchronous H2D -> kernel -> D2H chain: the link idles while the
 * kernel runs and each direction idles while the other moves. rg_submit_async stages a batch on a copy-in stream, runs the step kernel
 * on the table's stream and returns the outcome on a copy-out stream, chained by events, and RETURNS AT ONCE; up to
 * RG_PIPELINE_DEPTH batches are in flight (one more call first waits for the oldest), so the upload of batch k+1 overlaps the kernel
 * and the download of batch k — PCIe is full duplex. Batches apply in submission order (their kernels share one stream).
 *   - caller buffers (in->*, out->*) must stay valid and untouched until the batch has been waited for, and should be page-locked
 *     (rg_host_alloc): pageable memory makes every copy synchronous;
 *   - out->reply is written for every row; out->logfx / out->persist rows are meaningful only where the reply's flags say so. The
 *     CONTENT OF THE OTHER ROWS IS UNDEFINED (the columns are copied back densely from staging memory that is not cleared between
 *     batches — unlike rg_submit, which zeroes them): read a logfx / persist row only after checking its reply;
 *   - rg_submit_wait blocks until the OLDEST batch in flight has landed in its buffers; returns 1 when nothing is in flight;
 *   - every other entry point that touches the table first drains the pipeline. */
#define RG_PIPELINE_DEPTH 2
int rg_submit_async(rg_table_t *t, const rg_batch_t *in, const rg_outcome_t *out);
int rg_submit_wait(rg_table_t *t);

/* The same pipeline with COMPACT transfer formats: the link, not the kernel, bounds the host-memory path, so what
 * crosses it is cut to what carries information.
 *   upload    rg_batch32_t: a, b, c, d and the entry terms as int32 (16 + 4n bytes per row instead of 32 + 8n; 16 bytes flat for the
 *             AppendEntries rows whose entries share one term, RG_HDR_SAME_TERM). Legal only while every one of those values is in
 *             [0, 2^31) — raft terms and log indices of any deployment younger than 2^31 entries; a host that meets a larger value
 *             submits that batch through rg_submit_async instead (the two may be mixed freely). The rows are decided as they arrive by
 *             the compact-format step kernel: the decisions are the 64-bit ones, bit for bit (rg_submit32 below). No hint column (hints
 *             answer RG_NEED_HOST rows, which are rare: use the wide format for those batches).
 *   download  rg_outcome_packed_t: reply stays one row per event; logfx and persist come back PACKED, in row order, one item per row whose
 *             reply says it has one —  logfx:   flags & (RG_F_COMMIT | RG_F_LOG_APPEND | RG_F_LOG_TRUNC), or status RG_NEED_HOST
 *                                      persist: flags & RG_F_PERSIST
 *             so a host that walks reply[0 .. rows) takes the next item of a list whenever a row carries the mark. counts[0] / counts[1] =
 *             items produced (logfx / persist); items beyond the capacity given are dropped, counts still say how many there were.
 *             reply, logfx, persist and counts MUST be page-locked (rg_host_alloc): the lists are written by the device straight into
 *             them (their length is not known when the copy would have to be queued). -1 with a message otherwise.
 * Everything else — depth, ordering, rg_submit_wait — is as for rg_submit_async. */
typedef struct { int32_t a, b, c, d; } rg_ev_quad32_t;            /* 16 B */
typedef struct {
    uint32_t              rounds, count;  /* as rg_batch_t */
    const uint32_t       *gid;            /* as rg_batch_t */
    const rg_ev_head_t   *head;           /* [rounds*count] */
    const rg_ev_quad32_t *abcd;           /* [rounds*count] */
    const int32_t        *entry_terms;    /* [entry_count], addressed by head.aux */
    uint64_t              entry_count;
} rg_batch32_t;
typedef struct {
    rg_reply_t   *reply;                  /* [rounds*count] */
    rg_logfx_t   *logfx;                  /* [logfx_cap] packed */
    rg_persist_t *persist;                /* [persist_cap] packed */
    uint32_t     *counts;                 /* [2] */
    uint32_t      logfx_cap, persist_cap;
} rg_outcome_packed_t;
int rg_submit_async_packed(rg_table_t *t, const rg_batch32_t *in, const rg_outcome_packed_t *out);

/* THE ONCE-PER-TICK PATH (ABI 4). A host that flushes once per tick (support/EventLoopGroup.java:32-46 drains whatever is queued; a 300 ms-tick cluster queues
 * one or two events per group) submits small batches of a FIXED shape from the same page-locked buffers over and over, and what it feels is not the kernel
 * but the driver: rg_submit_async_packed is nine runtime calls per batch (copies up, three kernels, copies down, events). rg_tick_create records that
 * whole chain ONCE — upload of the compact rows, the step kernel, the packing of the effect lists, the download of the replies — as a HIP graph bound to
 * the caller's buffers; rg_tick_launch replays it with one call. The host refills `in`'s buffers between a wait and the next launch.
 *   in      shape and buffers are fixed at creation: rounds, count, gid (NULL = dense), head, abcd; entry_terms with entry_count = its CAPACITY (the whole
 *           array is uploaded every tick; 0 when every AppendEntries row carries RG_HDR_SAME_TERM). All page-locked (rg_host_alloc).
 *   out     as for rg_submit_async_packed (reply dense; logfx / persist lists with counts), page-locked.
 * Same decisions as rg_submit_async_packed on the same rows; launches of one table run in the order they were made, with every other submission
 * (they share the table's stream). Table options and whether the table has index bases are read at creation (set both first). At most one launch of a tick is in flight: rg_tick_launch waits for the previous one. Destroy a tick before its table. */
typedef struct rg_tick rg_tick_t;
int rg_tick_create(rg_table_t *t, const rg_batch32_t *in, const rg_outcome_packed_t *out, rg_tick_t **tick);
int rg_tick_launch(rg_tick_t *tick);      /* returns at once */
int rg_tick_wait(rg_tick_t *tick);        /* the launch has landed in `out` */
int rg_tick_destroy(rg_tick_t *tick);

/* The compact rows as a batch format of their own — what a host that keeps its batches in HBM (or builds them there) hands over:
 * 24 bytes per event instead of 40 + 8n, no gathered entry-term loads. Same contract as rg_submit (memspace, dense / sparse, rounds,
 * outcome columns, per-row status), same results: the kernel decides a workgroup's 64 groups on 32-bit values while every value of
 * those groups and of their rows is below 2^30 and restarts that workgroup's rounds in 64-bit arithmetic at the first value that is
 * not — nothing was written to the table by then, outcome rows are written again — so a table may hold any int64 state.
 * Rows whose values do not fit int32 cannot be expressed in this format at all: submit those batches through rg_submit.
 * The 32-bit tier's domain also covers the small fields it compares: role epochs, elected epochs and vote counts below 2^30, node ids >= -1,
 * `aux` below 2^30 where it is a role epoch or the entries' term, fewer than 2^24 rounds per launch — anything else is decided by the 64-bit
 * body as well, with the same results. Limit of the format: at most 2^28 - 1 rows per round (a row is addressed as scalar base + 32-bit lane
 * offset); larger batches are refused (-2, rg_last_error). RG_FORCE_WIDE=1 in the environment of rg_table_create makes every compact batch of
 * that table take the 64-bit body ("rg::step32_wide_kernel" in a profile): differential tests, and bench.py's int64-body pass. */
int rg_submit32(rg_table_t *t, const rg_batch32_t *in, const rg_outcome_t *out, int memspace);
/* Host-side packer (no device involved): rewrites a wide batch into caller buffers head[rows], abcd[rows], entry_terms[<= in->entry_count].
 * AppendEntries rows whose entries all have one term get RG_HDR_SAME_TERM and carry it in aux; the others keep their terms, renumbered.
 * Returns the entry_count of the compact batch, or < 0: -1 missing column, -2 the batch has hints, -3 a value outside [0, 2^31),
 * -4 entry_terms needed but NULL. rounds / count / gid are the wide batch's. */
int64_t rg_batch32_pack(const rg_batch_t *in, rg_ev_head_t *head, rg_ev_quad32_t *abcd, int32_t *entry_terms);

/* THE INDEX BASE OF THE COMPACT FORMATS (ABI 4). Every quantity of the path is a Java long (command/RaftLog.java:72-132); terms stay small (one per
 * election) but a group that lives long enough pushes its log indices past 2^30, which — with absolute 32-bit rows — would put it beyond the compact
 * formats and its whole workgroup on the 64-bit body for good. So every group has an index base (0 after rg_table_create), and in rg_batch32_t rows
 * and rg_out32_t rows a log index x of group g travels RELATIVE to it:
 *       x == 0 ("none": prevLogIndex of an empty log, leaderCommit 0, matchIndex of a follower that has not answered)  ->  0
 *       any other x                                                                                                      ->  x - base[g], in [1, 2^31)
 * The index fields of a row are: AE_REQ b, d; AE_ACK b, c; IS_ACK b; RV_REQ / PV_REQ b; LOG_FLUSH a; IS_REQ b (terms, n and aux travel as they are);
 * of an rg_out32_t row: commit_index and log_from. rg_outcome_t columns, rg_group_state_t and rg_send_t always speak absolute values.
 * The host keeps the base BELOW every non-zero index the group can meet — in practice a little below epoch.index, moved up after a compaction
 * (RaftLog.flush, command/storage/RocksLog.java:228-242) between two launches; a group whose epoch.index is 0 keeps base 0. Decisions never depend
 * on the base: the 32-bit body works on the relative image while every non-zero index of the group lies in (base, base + 2^30) and epoch.index > base,
 * the 64-bit body on absolute values otherwise (a value without an image in an rg_out32_t row: RG_F_WIDE_VALUES). base = 0 is ABI 3's format. */
/* AUTOMATIC BASES (ABI 6). With RG_OPT_AUTO_INDEX_BASE = W the table moves the bases itself, so that a host which packs its rows relative to a mirror
 * of them never has to call rg_index_base_set after a compaction. The rule:
 *       every RG_EV_LOG_FLUSH row a submission carries for group g, WHATEVER ITS STATUS (RG_FLUSH_OUT_OF_BOUNDS, RG_SKIPPED_AFTER_NEED_HOST and RG_NEED_HOST
 *       included), raises base[g] to max(base[g], a - W), a = the row's flush index in ABSOLUTE terms (a compact row's a is relative to the base the launch
 *       STARTED with; a = 0 moves nothing). All rows and outcome rows of a launch stay relative to the bases the launch started with; the new bases apply
 *       from the next launch (the next replay, for a recorded tick).
 * It depends on the rows only, never on outcomes: a host works out the bases of batch k + 1 before batch k is decided (rg_index_base_advance* below), which
 * is what two batches in flight need. Every submission path applies it — rg_submit / rg_submit_async (wide rows: absolute a), rg_submit32, rg_submit32c, rg_submit32c_sparse(_rounds),
 * rg_submit_async_packed, rg_tick_*, rg_tick2_* (dense and sparse), host and device memory alike. Nothing else moves a base: rg_load_state leaves the bases alone, rg_index_base_set
 * still sets them and the automatic moves go on from there, and the rule never lowers one. Decisions never depend on it (every reply, effect and persist row
 * is the one without it); it only decides which body decides a workgroup, and what rg_index_base_get reports. A group whose state falls outside
 * (base, base + 2^30) after a move — a lagging follower's non-zero matchIndex at a leader, say — is decided by the 64-bit body, correctly. W is how far
 * below the newest flush a stale row's index may lie and still have a relative image: 2^28 is the recommended value. */
int rg_index_base_set(rg_table_t *t, uint32_t first, uint32_t count, const int64_t *base);
int rg_index_base_get(rg_table_t *t, uint32_t first, uint32_t count, int64_t *base);
/* Host-side (no device involved): the rule above applied IN PLACE to a caller's mirror index_base[groups] for one batch, every round, dense (count == groups)
 * or a list of groups (gid < groups, any number of rounds: row (r, i) at r * count + i belongs to group gid[i]). rg_index_base_advance takes wide rows (absolute a); rg_index_base_advance32 compact rows, whose a is relative to the
 * array AS IT IS ON ENTRY. window: as RG_OPT_AUTO_INDEX_BASE, 1 <= W < 2^30. Returns 0; -1 a missing column (head, ab / abcd, index_base) or a window out of
 * range; -2 a batch of another shape (count, gid). */
int rg_index_base_advance(const rg_batch_t *in, int32_t window, uint32_t groups, int64_t *index_base);
int rg_index_base_advance32(const rg_batch32_t *in, int32_t window, uint32_t groups, int64_t *index_base);
/* rg_batch32_pack with bases: index_base[g] for every group of the table (NULL: all 0); -3 also when an index lies at or below its group's base */
int64_t rg_batch32_pack_rel(const rg_batch_t *in, const int64_t *index_base, rg_ev_head_t *head, rg_ev_quad32_t *abcd, int32_t *entry_terms);
/* COMPACT OUTCOME ROWS (ABI 4). What a reply carries is RaftResponse(term, success) (RaftResponse.java:8-24) plus instructions; while a
 * group's values are below 2^31 all of it fits ONE 16-byte row per event that every lane stores unconditionally — instead of a 16-byte reply
 * plus a conditional 16-byte effect row that half of the lanes store (32-byte write granules: measured 1.17x inflation) — and the role epoch,
 * which only changes with a conversion, moves into the persist row that a conversion writes anyway. Per 64-round launch of 65 536 groups the
 * outcome stream shrinks from ~125 MB to ~68 MB.
 *   rg_out32_t      always written.  resp_term: RaftResponse.term, 0 unless RG_F_REPLIED.  flags: as rg_reply_t.flags.  commit_index:
 *                   RaftLog.lastCommitted() AFTER the row, whatever the flags say (rg_logfx_t only has it for rows that carry an effect).
 *                   log_from: as rg_logfx_t.log_from WHERE the row carries RG_F_LOG_APPEND / RG_F_LOG_TRUNC or the status RG_NEED_HOST; UNDEFINED on every
 *                   other row (the kernel stores it without a select: a raw consumer must test the flags first — rg_outcome32_unpack does).
 *   rg_persist32_t  written iff RG_F_PERSIST (every conversion sets it: RaftMember.<init> persists, member/RaftMember.java:25): the durable
 *                   pair, the role, and the role epoch AFTER the row — the tag for the RPCs the host emits from now on. A row without
 *                   RG_F_PERSIST leaves the group's role epoch where it was.
 *   wide            optional (all three columns or none, [rounds*count] each): where a workgroup that left the 32-bit domain (the 64-bit body,
 *                   see rg_submit32) puts the full rows of an event whose values do not fit — such a row carries RG_F_WIDE_VALUES and the
 *                   low 32 bits. The columns are not touched otherwise. Without them the full values of such a row are lost to the caller
 *                   (rg_read_state still has the group's state).
 * Same batches, same decisions, same table state as rg_submit32. rg_submit32c takes dense batches only (gid == NULL); a LIST of groups goes through
 * rg_submit32c_sparse (below). The device-side timers and health statistics take the rows of a dense batch as they are: rg_timers_update32 /
 * rg_health_update32 (ABI 5), or the whole tick as one graph: rg_tick2_* — dense, or for a list of groups (rg_tick2_create_sparse). */
typedef struct { int32_t resp_term; uint32_t flags; int32_t commit_index; int32_t log_from; } rg_out32_t;          /* 16 B */
typedef struct { int32_t term; int32_t voted_for; uint32_t role_epoch; int32_t role; } rg_persist32_t;            /* 16 B */
typedef struct {
    rg_out32_t     *row;       /* [rounds*count], required */
    rg_persist32_t *persist;   /* [rounds*count], required */
    rg_outcome_t    wide;      /* optional overflow columns */
} rg_outcome32_t;
int rg_submit32c(rg_table_t *t, const rg_batch32_t *in, const rg_outcome32_t *out, int memspace);
/* The same for a LIST of groups: compact rows of the groups in->gid names in, compact outcome rows out. in->gid is required (strictly ascending, each below the
 * table's group count), rounds == 1, count <= groups; everything else as rg_submit32c — both memspaces, the overflow columns all three or none, RG_FORCE_WIDE,
 * index bases: the indices of row i, in and out, are relative to the base of ITS group gid[i]. RG_MEM_HOST validates the list as rg_submit does, RG_MEM_DEVICE
 * trusts it. Every outcome column holds `count` rows, row i for group gid[i]; groups the list does not name are not touched. The rows — after
 * rg_outcome32_unpack(_rel) with the role epochs / index bases of the listed groups gathered per row — and the table state are those of rg_submit32 on the
 * same batch. */
int rg_submit32c_sparse(rg_table_t *t, const rg_batch32_t *in, const rg_outcome32_t *out, int memspace);
/* rg_submit32c_sparse for R >= 1 ROUNDS, one launch: what a busy tick queues for a few groups — an AppendEntries, its ack, a client append (the reference's event
 * loop drains whatever is queued per context, support/EventLoopGroup.java:32-46). Round r of every column, in and out, occupies rows [r * count, (r + 1) * count);
 * row i of EVERY round belongs to group gid[i]; a group with fewer events than R carries RG_EV_NONE rows. in->rounds is bounded as for rg_submit32c, a round holds
 * fewer than 2^28 rows, RG_MEM_HOST validates the list as rg_submit does and stages rounds * count rows; everything else as rg_submit32c_sparse. The contract:
 *   - outcome row (r, i) equals row (r, gid[i]) of rg_submit32c on the dense rounds x groups batch that holds the same rows at the listed groups and RG_EV_NONE
 *     everywhere else (log_from under its marks, persist under RG_F_PERSIST, as everywhere), and the table state afterwards is the same; groups outside the list are
 *     untouched bit for bit. That covers a group that answers RG_NEED_HOST in round r — RG_SKIPPED_AFTER_NEED_HOST in its later rounds of the launch, its state as
 *     it was —, a workgroup that leaves the 32-bit domain in the middle of the launch and starts again on the 64-bit body, and RG_FORCE_WIDE=1;
 *   - index bases: the rows of every round, in and out, are relative to the bases the launch STARTED with; every LOG_FLUSH row of any round moves its group's base
 *     for the next launch under RG_OPT_AUTO_INDEX_BASE (rg_index_base_advance / rg_index_base_advance32 take the same shape);
 *   - with rounds == 1 the rows are rg_submit32c_sparse's. */
int rg_submit32c_sparse_rounds(rg_table_t *t, const rg_batch32_t *in, const rg_outcome32_t *out, int memspace);
/* Host-side (no device involved): compact outcome rows -> the wide columns, for callers written against rg_outcome_t. `in` and `out` are HOST
 * arrays of rounds*count rows (out->logfx / out->persist rows that carry nothing are zeroed, like rg_submit's). role_epoch: [count], the role
 * epoch of every group BEFORE the batch (rg_group_state_t.role_epoch); updated in place to the epochs after it. Rows flagged
 * RG_F_WIDE_VALUES are copied from in->wide (-3 when that is missing). Returns 0, or < 0. */
int rg_outcome32_unpack(const rg_outcome32_t *in, uint32_t rounds, uint32_t count, uint32_t *role_epoch, const rg_outcome_t *out);
/* the same for a table with index bases (below): index_base[count] puts commit_index / log_from back on the groups' bases (NULL: all 0) — the bases the
 * batch was PACKED with, i.e. those at the start of its launch (with RG_OPT_AUTO_INDEX_BASE the table may have moved them by the time the rows arrive) */
int rg_outcome32_unpack_rel(const rg_outcome32_t *in, uint32_t rounds, uint32_t count, uint32_t *role_epoch, const int64_t *index_base, const rg_outcome_t *out);
/* which step kernel a batch of `count` rows per round is decided by: "rg::step_split_kernel" (a deciding and an I/O
 * wavefront per 64 groups; chosen while the batch has at most one wavefront of groups per SIMD) or "rg::step_kernel";
 * compact batches (rg_submit32, rg_submit_async_packed) are always decided by "rg::step32_kernel" */
const char *rg_step_kernel(rg_table_t *t, uint32_t count);

/* ---- N1: the leader's send side ---------------------------------------------------------------- */
/* Leader.replicateLog (member/Leader.java:142-245) for many leader groups at once: WHAT to send to each follower —
 * heartbeat / entries range / InstallSnapshot — decided from nextIndex, pendingInstallation, the log window and the
 * in-flight gate. The host then reads the payload range [prev_index+1, prev_index+count] from its RaftLog, ships the
 * RPC tagged with head.role_epoch, and keeps (head.epoch_index, send.last_index) for the response row (AE_ACK b, c).
 * Runs Leader.prepareReplication first for a leader that has not sent anything yet (the only state change). */
enum {
    RG_SEND_NONE      = 0,   /* the group is not a Leader: nothing to send                                   */
    RG_SEND_APPEND    = 1,   /* appendEntries(term, self, prev_index, prev_term, entries[count], leaderCommit) */
    RG_SEND_SNAPSHOT  = 2,   /* installSnapshot(term, self, epoch.index, epoch.term)  (Leader.java:168-190)   */
    RG_SEND_GATED     = 3,   /* requestInFlight > IN_FLIGHT_LIMIT / (heartbeat ? 10 : 1)  (Leader.java:162-166) */
    RG_SEND_NEED_HOST = 4    /* term of prev_index is below the cached runs: host reads it from its RaftLog    */
};
#define RG_REPLICATE_LIMIT 50    /* member/Leadership.java:10 */
#define RG_IN_FLIGHT_LIMIT 20    /* member/Leadership.java:11 */

typedef struct {                 /* one per row */
    int64_t  term;               /* currentTerm                                    */
    int64_t  leader_commit;      /* RaftLog.lastCommitted()                        */
    int64_t  epoch_index;        /* RaftLog.epoch() at send time (closure state of the callback) */
    int64_t  epoch_term;
    uint32_t role_epoch;         /* tag for the response rows                      */
    uint32_t is_leader;          /* 0: every send of this row is RG_SEND_NONE      */
    uint64_t reserved;           /* pads the row to three 16-byte words so a wavefront stores whole 1 KiB lines. 0 — except in the send step of a tick on a table
                                    with RG_OPT_DEVICE_IN_FLIGHT, where it says what the tick derived for the row: RG_SENT_TRIGGERED | RG_SENT_HEARTBEAT */
} rg_send_head_t;                /* 48 B */

#define RG_SENT_TRIGGERED  1u    /* rg_send_head_t.reserved, RG_OPT_DEVICE_IN_FLIGHT: a handler of the row's rounds sent (acceptCommand or onTimeout); clear: every send is RG_SEND_NONE */
#define RG_SENT_HEARTBEAT  2u    /* ... and it was onTimeout alone: replicateLog(true), fetch limit 25, in-flight limit 2 */

typedef struct {                 /* one per (row, follower j); j = slot<self ? slot : slot-1 */
    int64_t  prev_index;
    int64_t  prev_term;
    int64_t  last_index;         /* lastIndex of Leader.replicateLog: what the success ack will claim */
    uint32_t count;              /* entries to ship: indices prev_index+1 .. prev_index+count         */
    uint32_t kind;               /* RG_SEND_* */
} rg_send_t;                     /* 32 B; stored follower-major: send[j * count + row], so a wavefront writes 2 KiB runs */

/* rows: `count` groups; gid NULL = groups 0..count-1 (count == table groups), else strictly ascending group ids.
 * heartbeat[i] != 0: Leader.onTimeout path (fetch limit 25, in-flight limit 2); else the acceptCommand path (50, 20).
 * in_flight: [(cluster-1) * count] State.requestInFlight, follower-major like `send`; NULL = all zero.
 * head: [count]; send: [(cluster-1) * count], element (j, row) at j * count + row.
 * memspace as rg_submit (RG_MEM_DEVICE is asynchronous). */
int rg_replicate(rg_table_t *t, uint32_t count, const uint32_t *gid, const uint8_t *heartbeat, const uint16_t *in_flight,
                 rg_send_head_t *head, rg_send_t *send, int memspace);

/* ---- N4: election / heartbeat timers on the device ------------------------------------------------ */
/* RaftRoutine.resetTimer / electionTimeout / keepAlive (context/RaftRoutine.java:53-130) for all groups: instead of two
 * ScheduledFuture operations per AppendEntries on the host, one deadline per group lives in HBM.
 *   rg_timers_update  folds the RG_F_RESET_TIMER / RG_F_ROLE_CHANGED flags of a finished batch into the deadlines:
 *                     Follower/Candidate -> now + election timeout drawn uniformly from [E, 2E] (RaftConfig.java:187-190;
 *                     the draw is splitmix64(seed, gid, role_epoch, now), not Java's ThreadLocalRandom), a new Leader ->
 *                     now (first heartbeat at once), a Leader's tick -> now + H. A ticket that already fired is only
 *                     replaced by a new participant (TimerTicket.TIMEOUT makes resetTimer return false).
 *   rg_timers_expired lists, in ascending group order, every group whose deadline has passed (wavefront ballot +
 *                     popcount compaction) and marks its ticket fired: the host turns each into one RG_EV_TIMEOUT row.
 * now / deadlines are milliseconds on a clock of the host's choosing (System.currentTimeMillis() in the reference), 64 bits wide throughout. THE CLOCK'S
 * DOMAIN: 1 <= now <= 2^62 for every `now` of this header (rg_timers_*, rg_health_*, rg_ready, the clocks of a tick), and election_ms, heartbeat_ms >= 1.
 * 0, negative values and INT64_MAX are marks of the deadline column — 0 = no ticket yet, -1 = the ticket fired, INT64_MAX = muted — so no clock and no
 * deadline may coincide with them, and now + 2 * election_ms and now + heartbeat_ms must not wrap. A clock outside the domain is the host's error and is not
 * refused, like an index outside [1, 2^30) relative to its base. The clock need not be monotonic: requestSuccess / requestFailure keep their maxima
 * (increaseMono), and a deadline is whatever the last reset made it. */
int rg_timers_configure(rg_table_t *t, int64_t election_ms, int64_t heartbeat_ms, uint64_t seed);
/* reply: the rg_reply_t rows of the batch just submitted ([rounds*count], same gid convention as rg_submit);
 * now: [rounds] timestamp of every round. memspace applies to reply and gid (now is always a host array). */
int rg_timers_update(rg_table_t *t, uint32_t rounds, uint32_t count, const uint32_t *gid, const rg_reply_t *reply,
                     const int64_t *now, int memspace);
/* out_gid: caller buffer for up to `capacity` group ids (host or device per memspace); *out_count receives the number of
 * expired groups (may exceed capacity: then only the first `capacity` were written AND marked fired). Synchronous. */
int rg_timers_expired(rg_table_t *t, int64_t now, uint32_t *out_gid, uint32_t capacity, uint32_t *out_count, int memspace);
/* the same, also reporting for every expired group the role epoch of the participant whose ticket fired: the host puts it into
 * the aux field of the RG_EV_TIMEOUT row, so a timeout that is overtaken by a row which replaces the participant is dropped like
 * the reference drops it (context/RaftRoutine.java:70). out_epoch: [capacity], same memspace as out_gid. */
int rg_timers_expired_epochs(rg_table_t *t, int64_t now, uint32_t *out_gid, uint32_t *out_epoch, uint32_t capacity, uint32_t *out_count,
                             int memspace);
/* The same from COMPACT outcome rows (ABI 5; dense batches only — the rows of rg_submit32c_sparse go through rg_outcome32_unpack and the wide call with their gid list): row = the rg_out32_t column, persist32 = the rg_persist32_t column of the
 * batch just decided, [rounds * groups] each. A compact row names its role epoch only where a conversion happened (rg_persist32_t.role_epoch); the
 * rows before a batch's first conversion are chained from the epoch the group had after the PREVIOUS batch, which the table remembers per group —
 * refreshed by rg_load_state, rg_timers_arm and by every rg_timers_update / rg_timers_update32: the timers must see every batch of the table, in
 * order (they must anyway: a skipped batch loses its RG_F_RESET_TIMER flags). Deadlines are those rg_timers_update makes of the unpacked rows. */
int rg_timers_update32(rg_table_t *t, uint32_t rounds, const rg_out32_t *row, const rg_persist32_t *persist32, const int64_t *now, int memspace);
/* arm every group that has no ticket yet (after rg_load_state): role from the table, as rg_timers_update would */
int rg_timers_arm(rg_table_t *t, int64_t now);
int rg_timers_read(rg_table_t *t, uint32_t first, uint32_t count, int64_t *deadline);

/* ---- N4 (second half): follower health and the leader's readiness gate ------------------------------ */
/* Leadership.State.{requestSuccess, requestFailure, recentFailure} with statSuccess / statFailure / isUnhealthy / isReady
 * (member/Leadership.java:28-73) and Leader.isReady (member/Leader.java:52-64), the gate RaftStub.process puts in front of
 * client commands (command/RaftStub.java:83-87). Wall-clock inputs arrive as `now`; nothing here feeds back into decisions.
 *   rg_health_update   fold a finished batch: every AE_ACK / IS_ACK row that reached statSuccess (not fenced, no higher
 *                      term, row applied) sets requestSuccess = max(.., now) and clears recentFailure; a group that
 *                      became Leader gets fresh State objects (all zero).
 *   rg_health_failure  statFailure(now, unreachable, reject) for RPCs that ended in an error / timeout on the host
 *                      (flags bit0 = unreachable, bit1 = reject; reject also bumps recentRejection of the table).
 *                      With RG_OPT_DEVICE_IN_FLIGHT it is also the callback's requestInFlight-- (member/Leader.java:176,221, then statFailure): the count
 *                      of every (gid, slot) given goes down by one per entry, clamped at 0, whatever the group's role — EXCEPT for an entry with bit2,
 *                      RG_HEALTH_NO_REQUEST: the "service is not available" call of Leader.java:242, where nothing was sent; its statistics are as always
 *                      and no count moves. Entries may repeat a (gid, slot) pair; each takes one off. Without the option bit2 is ignored.
 *   rg_ready           Leader.isReady per group: 1 when self + healthy followers exceed half the followers, else 0
 *                      (0 for non-leaders and for leaders that have not prepared replication). */
int rg_health_update(rg_table_t *t, uint32_t rounds, uint32_t count, const uint32_t *gid, const rg_ev_head_t *head,
                     const rg_reply_t *reply, const int64_t *now, int memspace);
/* rg_health_update from compact outcome rows (ABI 5; dense): head = the batch's event heads, row = its rg_out32_t column */
int rg_health_update32(rg_table_t *t, uint32_t rounds, const rg_ev_head_t *head, const rg_out32_t *row, const int64_t *now, int memspace);
#define RG_HEALTH_NO_REQUEST 4u
int rg_health_failure(rg_table_t *t, uint32_t n, const uint32_t *gid, const uint8_t *slot, const uint8_t *flags, int64_t now);
int rg_ready(rg_table_t *t, int64_t now, int32_t critical_point, int64_t cool_down_ms, uint8_t *ready, int memspace);
/* request_success / request_failure / recent_failure: [count * (cluster-1)], index g*(P-1)+j like rg_group_state_t peers */
int rg_health_read(rg_table_t *t, uint32_t first, uint32_t count, int64_t *request_success, int64_t *request_failure,
                   int32_t *recent_failure);
/* State.requestInFlight of groups [first, first + count) as a table with RG_OPT_DEVICE_IN_FLIGHT keeps it: in_flight is [count * (cluster-1)], index g*(P-1)+j like
 * rg_health_read. rg_in_flight_set overwrites the counts (a restart that knows what is outstanding; tests). Both wait for the table's stream; both answer -1 with a
 * message while the option is off. */
int rg_in_flight_read(rg_table_t *t, uint32_t first, uint32_t count, uint16_t *in_flight);
int rg_in_flight_set(rg_table_t *t, uint32_t first, uint32_t count, const uint16_t *in_flight);

/* ---- THE DEVICE-RESIDENT TICK (ABI 5) --------------------------------------------------------------------------------------------------
 * "closes the loop leader-step -> follower-step on device". One tick of a node, recorded ONCE as a HIP graph on the table's stream
 * and replayed with one call:
 *     rg::step32_kernel (compact rows in, compact outcome rows out: rg_submit32c)                        support/EventLoopGroup.java:32-46
 *  -> timers_update32   the batch's RESET_TIMER / ROLE_CHANGED / TIMER_MUTED flags into the deadlines     context/RaftRoutine.java:86-130
 *  -> health_update32   acks that reached statSuccess into requestSuccess / recentFailure                 member/Leadership.java:53-63
 *  -> timers_expired    the tickets that fired by now[rounds - 1], ascending, with their role epochs      context/RaftRoutine.java:53-77
 *  -> replicate         what every leader sends to every follower                                          member/Leader.java:142-245
 *  -> ready             Leader.isReady per group                                                           member/Leader.java:52-64
 * (the last three are optional: leave their outputs NULL). Nothing is copied: every pointer below must be DEVICE-VISIBLE for the life of the tick —
 * device memory (rg_dev_alloc) or page-locked host memory (rg_host_alloc, which the device reads and writes over the link) — and is read / written where
 * it lies, so the caller decides per column what stays in HBM (the rows of a resident replay, the send table a gateway kernel consumes) and what crosses
 * the link (the expired list, a few counters). The per-round clocks are READ from `now` when the graph runs: refill rows and clocks, launch, wait.
 * Decisions, deadlines, statistics and send rows are those of the separate calls (tests/test_gpu_parity.py::test_the_device_resident_tick_matches_the_oracle).
 * The table's options and index bases at creation are part of the recording: rg_tick2_launch refuses (-1) when they have changed since.
 *
 * THE SEND STEP WITH DEVICE-RESIDENT IN-FLIGHT COUNTS (RG_OPT_DEVICE_IN_FLIGHT = 1). heartbeat[] and in_flight[] are per row, so a host that fills them must know which
 * group sits in which row — which a tick fed by rg_assemble32 does not. With the option on, all three of rg_tick2_create, rg_tick2_create_sparse and
 * rg_tick2_create_sparse_rounds REFUSE a non-NULL io->heartbeat or io->in_flight (-1, a message that names the option, nothing recorded), and a tick that has a send step
 * (send_head != NULL) derives both from its own rows. For every row it decides, over that row's rounds 0 .. R - 1 in order:
 *   - a row with RG_F_ROLE_CHANGED forgets the trigger collected so far; if the role after it is Leader it zeroes the group's P - 1 counts (fresh State objects: what
 *     the fold does for the health statistics);
 *   - an RG_EV_AE_ACK / RG_EV_IS_ACK row takes one off the count of its follower, clamped at 0, unless its status is RG_DROPPED_STALE_ROLE or RG_BAD_EVENT, it carries
 *     RG_F_ROLE_CHANGED, or its slot is not a follower's. The callback decrements before it looks at the result (member/Leader.java:176,221): reached, success and a
 *     mismatch status do not matter; a stale ack belongs to State objects that no longer exist;
 *   - the trigger: `command` = an RG_EV_CLIENT_APPEND row with status RG_OK and RG_F_LOG_APPEND (acceptCommand); `heartbeat` = a row whose RG_F_EMIT is
 *     RG_EMIT_HEARTBEAT (a Leader's onTimeout). A row with any command sends as acceptCommand (fetch limit 50, in-flight limit 20) whatever else it holds; one with
 *     heartbeats only as onTimeout (25, 2); one with neither does not send.
 * THE SENDS OF A ROW'S ROUNDS COLLAPSE INTO ONE PLAN, taken after round R - 1 — as they always have in a tick: the reference would have sent once per handler.
 *   - a triggered row: send_head[row] and send[j][row] are exactly what rg_replicate(t, 1, &gid, &hb, counts, ..) gives at that point, hb from the trigger, counts =
 *     the group's counts after the decrements above; every follower whose kind comes out RG_SEND_APPEND, RG_SEND_SNAPSHOT or RG_SEND_NEED_HOST gets +1 (saturating at
 *     65 535), RG_SEND_GATED and RG_SEND_NONE nothing;
 *   - a row without a trigger (say, one whose only event was an ack): the head's scalar fields and is_leader are the group's, every send is {0, 0, 0, 0, RG_SEND_NONE},
 *     Leader.prepareReplication does NOT run, no count goes up. (Without the option rg_replicate's answer is written for every listed leader row.)
 *   - send_head.reserved carries RG_SENT_TRIGGERED and RG_SENT_HEARTBEAT (0 with the option off).
 * Rows >= n and rounds >= R stay untouched, as always; the counts of groups outside a sparse tick's list are not touched. A tick without a send step moves no count.
 * The dense tick's step-by-step recording (RG_TICK_NODES=4, an experiment knob) is recorded as RG_TICK_NODES=2 with the option on.            */
typedef struct {
    /* in */
    uint32_t              rounds;           /* 1 .. 64; count is the table's group count (dense). rg_tick2_create_sparse: 1, and every G below reads `capacity`; rg_tick2_create_sparse_rounds: the greatest depth */
    const rg_ev_head_t   *head;             /* [rounds * G] */
    const rg_ev_quad32_t *abcd;             /* [rounds * G] */
    const int32_t        *entry_terms;      /* [entry_capacity] or NULL */
    uint64_t              entry_capacity;
    const int64_t        *now;              /* [rounds] clock of every round; now[rounds - 1] is "now" for expiry and readiness */
    const uint8_t        *heartbeat;        /* [G] rg_replicate's per-row flag, or NULL (all 0). Must be NULL on a table with RG_OPT_DEVICE_IN_FLIGHT */
    const uint16_t       *in_flight;        /* [(P - 1) * G] or NULL. Must be NULL on a table with RG_OPT_DEVICE_IN_FLIGHT */
    int32_t               critical_point;   /* rg_ready's availableCriticalPoint / recoveryCoolDownMills */
    int64_t               cool_down_ms;
    /* out */
    rg_out32_t           *row;              /* [rounds * G] */
    rg_persist32_t       *persist32;        /* [rounds * G] (a row is written iff its flags carry RG_F_PERSIST) */
    uint32_t             *expired_gid;      /* [expired_capacity] or NULL: no expiry step */
    uint32_t             *expired_epoch;    /* [expired_capacity] or NULL */
    uint32_t             *expired_count;    /* [1]: groups that expired (may exceed the capacity: then only the first were listed AND marked fired) */
    uint32_t              expired_capacity;
    rg_send_head_t       *send_head;        /* [G] or NULL: no send step */
    rg_send_t            *send;             /* [(P - 1) * G] */
    uint8_t              *ready;            /* [G] or NULL */
} rg_tick2_io_t;
typedef struct rg_tick2 rg_tick2_t;
int rg_tick2_create(rg_table_t *t, const rg_tick2_io_t *io, rg_tick2_t **tick);
/* THE SPARSE TICK: the same recording for a LIST of groups whose length changes from tick to tick. A node that ticks every ~100 us with 300 ms election timers
 * has an event for a small share of its groups; the dense tick reads and writes the state, a 24-byte event row, a 16-byte outcome row, a send head and P - 1 send
 * rows of ALL of them every time. Here only the listed groups are touched (plus 8 bytes of deadline per group of the table for the expiry).
 *   rows     gid[i] = the group of row i: the first n entries strictly ascending, each below the table's group count (trusted, like every list in device memory);
 *            n = min(*count, capacity) is READ when the graph runs, like the clocks: refill gid, count, rows and clock, launch, wait. gid and count must be
 *            device-visible like every other column. capacity (1 .. groups) is what every per-row column is sized for.
 *   io       rounds must be 1. The per-row columns are indexed by ROW: head, abcd, row, persist32, heartbeat, send_head, ready hold [capacity] rows; in_flight
 *            and send [(P - 1) * capacity], element (j, row) at j * capacity + row. expired_* are unchanged: they describe the whole table.
 * One run of the graph: (1) rows 0 .. n - 1 are decided as rg_submit32c_sparse decides them — rows >= n of every output column are NOT TOUCHED; (2) their flags
 * are folded into the deadlines and the followers' statistics of their groups at now[0], as rg_timers_update / rg_health_update do with that gid list; (3)
 * send_head[row] / send[j * capacity + row] are what rg_replicate(t, n, gid, heartbeat, in_flight, ..) gives for the row — a leader sends from onTimeout and
 * acceptCommand only (member/Leader.java:120-140), i.e. only where its group has a row; (4) ready[row] is Leader.isReady of gid[row] at now[0] (rg_ready still has
 * the whole column); (5) the tickets that fired by now[0] in the WHOLE TABLE, ascending, with their role epochs, marked fired — as in the dense tick. n = 0 is a
 * legal tick: only (5) happens. The handle is an ordinary rg_tick2_t: rg_tick2_launch / _wait / _destroy, the refusal after a change of options or index bases and
 * the behaviour of a tick that outlives its table are those of the dense tick. With the list gid[i] = i, n = capacity = groups, every column equals the dense
 * tick's. Which of the two to record is the caller's choice: it knows its fill. With RG_OPT_DEVICE_IN_FLIGHT step (3) is the derived one described above: heartbeat and
 * in_flight must be NULL, a listed leader sends only where a handler of its row sent, and the counts of the listed groups move. */
typedef struct {
    const uint32_t *gid;       /* [capacity] group of row i; the first n entries strictly ascending, each below the table's group count */
    const uint32_t *count;     /* [1] rows of THIS tick, read when the graph runs; n = min(*count, capacity) */
    uint32_t        capacity;  /* 1 .. groups: what every per-row column is sized for */
} rg_tick2_rows_t;
int rg_tick2_create_sparse(rg_table_t *t, const rg_tick2_io_t *io, const rg_tick2_rows_t *rows, rg_tick2_t **tick);
/* THE SPARSE TICK WITH A DEPTH: the same recording for a list of groups some of which have two or three events queued. Both the row count AND the depth of a run are
 * read when the graph runs: refill gid, count, rounds, the rows of rounds 0 .. R - 1 and their clocks, launch, wait — one launch where the one-round sparse tick
 * needs R (what that is worth in time: DESIGN.md section 6).
 *   io       rounds is the GREATEST depth (1 .. 64). head, abcd, row and persist32 are [io->rounds][capacity]: row i of round r lies at r * capacity + i — the stride
 *            is the capacity, whatever n and R are in a run. now holds io->rounds clocks. heartbeat, in_flight, send_head, send and ready stay per row
 *            ([capacity], [(P - 1) * capacity]); expired_* describe the whole table.
 *   rows     gid, count, capacity as rg_tick2_rows_t; rounds: [1], device-visible, R = clamp(*rounds, 1, io->rounds); NULL: every run has io->rounds rounds.
 * One run: (1) rows 0 .. n - 1 of rounds 0 .. R - 1 are decided as rg_submit32c_sparse_rounds decides them; (2) their flags are folded into the deadlines and the
 * followers' statistics of their groups, round by round at now[r] — what rg_timers_update / rg_health_update give with that gid list and R rounds; (3) send_head[row] /
 * send[j * capacity + row] are rg_replicate's answer for the row after round R - 1; (4) ready[row] is Leader.isReady at now[R - 1]; (5) the fired tickets of the whole
 * table are taken at now[R - 1]. Rows >= n of any round and rounds >= R are NOT TOUCHED in any output column. n = 0 is a legal tick: expiry only, at now[R - 1].
 * With rounds == NULL or *rounds == io->rounds, the list gid[i] = i and n = capacity = groups, every column equals the dense io->rounds-round tick's; with
 * io->rounds == 1 every column equals rg_tick2_create_sparse's. The handle is an ordinary rg_tick2_t: launch / wait / destroy, the refusal after a change of options or
 * index bases and a tick that outlives its table are all as above. Refused before anything is recorded, each with a message: a missing gid / count, a capacity of 0 or
 * above the group count, io->rounds outside 1 .. 64, a column or a `rounds` that is not device-visible, a cluster above RG_MAX_COMPACT_CLUSTER unless the table has
 * RG_OPT_COMPACT_ANY_CLUSTER; io->heartbeat or io->in_flight on a table with RG_OPT_DEVICE_IN_FLIGHT. With that option step (3) is the derived one described at
 * rg_tick2_io_t: the row's rounds 0 .. R - 1 are walked in order, one plan after round R - 1. */
typedef struct {
    const uint32_t *gid;       /* [capacity] as rg_tick2_rows_t */
    const uint32_t *count;     /* [1] rows of THIS tick, n = min(*count, capacity), read when the graph runs */
    const uint32_t *rounds;    /* [1] depth of THIS tick, R = clamp(*rounds, 1, io->rounds), read when the graph runs; NULL: always io->rounds */
    uint32_t        capacity;  /* 1 .. groups */
} rg_tick2_rounds_t;
int rg_tick2_create_sparse_rounds(rg_table_t *t, const rg_tick2_io_t *io, const rg_tick2_rounds_t *rows, rg_tick2_t **tick);
int rg_tick2_launch(rg_tick2_t *tick);      /* asynchronous on the table's stream. A launch issued before rg_tick2_wait of the previous one is ORDERED AFTER it
                                               on that stream and does not wait on the host: with every column in device memory a host can queue ticks whose rows
                                               another kernel produces; it reads `row`, the lists and `ready` of the LAST tick only after rg_tick2_wait */
int rg_tick2_wait(rg_tick2_t *tick);
int rg_tick2_destroy(rg_tick2_t *tick);

/* ---- ASSEMBLING A BATCH ON THE DEVICE (new symbols only; the ABI stays 6) -----------------------------------------------------------------
 * rg_submit32c_sparse_rounds and the sparse tick with a depth take ONE shape: a strictly ascending gid list, n and R, rows laid out [round][capacity], the k-th
 * queued event of a group in round k. A host receives events in ARRIVAL ORDER, for arbitrary groups, from many reader threads; and the tickets a tick listed in
 * expired_gid / expired_epoch / expired_count want one RG_EV_TIMEOUT row each in the next tick. rg_assemble32 turns the one into the other on the device: a reader
 * thread's whole job is to append (gid, head, abcd) to an arrival log, and a fired ticket gets its row without the host reading the list.
 *
 * THE SEQUENCE S of a run is the expired source first, then the arrival log:
 *   - entries j = 0 .. e - 1 of the expired source, e = min(*expired_count, expired_capacity); e = 0 when the source is absent (all three pointers NULL) and when
 *     *expired_count is 0xFFFFFFFF — the tick's mark for a look-back that ran into its bound, whose list is not to be used. Entry j becomes the row
 *     head = {RG_HDR_MAKE(RG_EV_TIMEOUT, 0, 0, 0), expired_epoch[j]} (the fenced onTimeout), abcd = {0, 0, 0, 0}, with the id 0x80000000 | j;
 *   - then the arrival events k = 0 .. m - 1, m = min(*count, capacity), with the id k. (A ticket fired at the END of the previous tick: its onTimeout precedes
 *     what has arrived since.)
 * An event whose gid is at or above the table's group count is counted in stats[2] and otherwise ignored, in both memspaces: the log is never trusted.
 *
 * THE RESULT. Let U be the ascending set of the distinct valid gids in S. n = min(|U|, C), C = out->capacity; gid[0 .. n) holds the n smallest gids of U. The events of
 * group gid[i], in S order, occupy rounds 0, 1, 2, .. of row i, packed from round 0 with no holes; those of rank >= D (D = out->max_rounds) are DEFERRED, and so is every
 * event of a group outside the list. R = the greatest number of rounds any listed row uses, 1 when n = 0. *count = n, *rounds = R. head / abcd / origin are [D][C]: row i
 * of round r at r * C + i — the stride is the capacity, as for the tick. A cell (r, i), r < R and i < n, that holds an event gets the event's head and abcd VERBATIM and
 * origin = its id; one that holds none gets head = {0, 0} (RG_EV_NONE), abcd = {0, 0, 0, 0}, origin = 0xFFFFFFFF. Rows >= n of any round and rounds >= R are NOT
 * TOUCHED in any column: the tick's own convention. deferred[] receives the deferred ids in S order, the first deferred_capacity of them; stats = {events placed,
 * events deferred (may exceed deferred_capacity), events with gid >= groups, 0}. A host puts the deferred events at the HEAD of its next arrival log (a deferred
 * ticket as a plain RG_EV_TIMEOUT row with the epoch it was listed with): per-group order then survives any overflow. `origin` routes outcome row (r, i) of the
 * launch that decides the batch back to the event it answers.
 * Every output is a function of the inputs alone, bit for bit, run after run: slots are claimed through atomics, ranks come from the ids.
 *
 * INDEX BASES: nothing is done and nothing needs doing. Rows are moved verbatim, so their indices stay relative to the bases of the launch that will decide them
 * (rg_batch32_pack_rel on the reader's side, as for any compact row); `aux` of an AppendEntries row still addresses the entry_terms array handed to that launch.
 *
 * MEMSPACES. RG_MEM_DEVICE: every pointer of both structs is device-visible (rg_dev_alloc / rg_host_alloc) and stays valid until the run has executed; the call is
 * asynchronous on the table's stream, synchronises nothing and decides nothing on the host from device data — its grids are sized from the capacities and leave
 * early on the counts they read when they run (the counts and the entries below them stand still from the call until the run has executed; a reader may append BEYOND *count). So a run can be followed on the same stream by rg_tick2_launch of a recording made over the very same gid / count /
 * rounds / head / abcd buffers (rg_tick2_create_sparse_rounds with capacity C and io->rounds D), with the previous tick's expired_* columns as the second source: the
 * host knows neither n nor R — and on a table with RG_OPT_DEVICE_IN_FLIGHT the send step of that tick needs no per-row column from it either. RG_MEM_HOST: host arrays, staged in and out, synchronous, after the pipeline has drained like every other entry point.
 * The assembler owns the scratch of its runs (about 8 bytes per group and 9 per event) and belongs to its table: destroy it before the table; one run at a time.
 * Refused (-1, with a message, before any launch): a missing column (deferred may be NULL with deferred_capacity 0), C = 0 or above the group count, D outside
 * 1 .. 64, an arrival or expired capacity above what the assembler was created for, an expired source given in part, an unknown memspace and, in RG_MEM_DEVICE, a
 * pointer that is neither device memory nor page-locked host memory. */
typedef struct {                       /* the arrival log of one run */
    const uint32_t       *count;       /* [1] events of THIS run, m = min(*count, capacity); read when the run executes */
    uint32_t              capacity;    /* what gid / head / abcd hold */
    const uint32_t       *gid;         /* [capacity] group of event k, ANY order, repeats allowed */
    const rg_ev_head_t   *head;        /* [capacity] compact rows exactly as rg_batch32_t carries them */
    const rg_ev_quad32_t *abcd;        /* [capacity] */
    const uint32_t       *expired_gid, *expired_epoch, *expired_count;   /* optional second source: the columns a tick wrote; all three or none */
    uint32_t              expired_capacity;
} rg_arrivals_t;
typedef struct {                       /* the columns rg_submit32c_sparse_rounds / rg_tick2_rounds_t + rg_tick2_io_t read, plus routing */
    uint32_t        capacity;          /* C: rows the per-row columns hold, 1 .. groups */
    uint32_t        max_rounds;        /* D: 1 .. 64 */
    uint32_t       *gid, *count, *rounds;         /* [C], [1] = n, [1] = R */
    rg_ev_head_t   *head;              /* [D][C] */
    rg_ev_quad32_t *abcd;              /* [D][C] */
    uint32_t       *origin;            /* [D][C] the id of the event a cell holds, 0xFFFFFFFF for none */
    uint32_t       *deferred;          /* [deferred_capacity] ids of the events that did not fit, in S order */
    uint32_t        deferred_capacity;
    uint32_t       *stats;             /* [4] */
} rg_assembled_t;
typedef struct rg_assembler rg_assembler_t;
int rg_assembler_create(rg_table_t *t, uint32_t max_events, uint32_t max_expired, rg_assembler_t **a);
int rg_assemble32(rg_assembler_t *a, const rg_arrivals_t *in, const rg_assembled_t *out, int memspace);
int rg_assembler_destroy(rg_assembler_t *a);

/* ---- ROUTING A DECIDED BATCH BACK TO ARRIVAL ORDER (new symbols only; the ABI stays 6) -----------------------------------------------------------
 * What a launch leaves of a batch rg_assemble32 made is in the launch's shape: outcome rows at [D][C] in ascending-group order, `origin` the only link back to the
 * event a cell answers, persist rows scattered under RG_F_PERSIST, a send table of [(P-1)][C] rows that is mostly RG_SEND_NONE, the rare RG_NEED_HOST row found
 * only by looking at every row. rg_route32 turns that into what the readers of a host want, on the device: the reader that appended event k finds its answer at
 * index k, the durability journal gets the list of the conversions, a sender thread per peer one contiguous run of the rows it has to ship.
 *
 * THE RUN IT ROUTES is the LAST run of assembler `a`: m (arrival events read) and e (expired entries used) are the values THAT run read — the assembler keeps both
 * in its own device scratch, because a tick that shares the expired_* buffers has overwritten expired_count by the time the route runs, and so that the host need
 * pass neither. e is 0 for an absent source and for the 0xFFFFFFFF mark. n = min(*count, C) and R = clamp(*rounds, 1, D) are read when the run executes, as the tick
 * reads them. cell = r * C + i names the cell of row i in round r.
 *
 * THE RESULT.
 *   - ARRIVAL ORDER: cell / row / persist32 of rg_routed_t hold [arrival_capacity] entries. For every k < m: cell[k] is ALWAYS written — the cell whose origin is k,
 *     RG_ROUTE_NONE for a deferred event and for one with a bad gid; row[k] is that cell's 16 bytes of the `row` column VERBATIM, written iff the event was placed;
 *     persist32[k] is the cell's persist row, written iff the event was placed and its flags carry RG_F_PERSIST. Entries >= m are NOT TOUCHED. The reader finds
 *     ready[i] and its send rows from i = cell[k] % C.
 *   - THE EXPIRED SOURCE: the same three columns, [expired_capacity], all three or none: entry j < e is addressed by the origin 0x80000000 | j, entries >= e are not
 *     touched.
 *   - persist_list: {cell, gid} of every cell (r < R, i < n) whose flags carry RG_F_PERSIST, in ascending cell order — round-major, so a group's conversions stay in
 *     order: what the durability journal consumes. attention: the same for every cell whose status is RG_NEED_HOST.
 *   - send_list, built only when the send table was given: {row, gid} of every (j, i < n) whose send[j * C + i].kind is RG_SEND_APPEND, RG_SEND_SNAPSHOT or
 *     RG_SEND_NEED_HOST, follower j ascending, then row ascending; follower j's items are [send_offset[j], send_offset[j + 1]), send_offset[P - 1] is the total: a
 *     sender thread per peer takes one contiguous run. Rows >= n of the send table were not written by the tick and are not read. Without a send table send_offset is
 *     not touched and counts[2] is 0.
 *   - counts[4] = {persist items, attention items, send items, 0}. A count may exceed its list's capacity: the first `capacity` items in the stated order are then
 *     written and the offsets stay the true ones. List entries beyond what was written are NOT TOUCHED; a capacity of 0 with a NULL list is legal.
 * Every output is a function of the inputs alone, bit for bit, run after run: the lists are compacted by ballot, popcount and prefix sum, nothing is appended
 * through an atomic. `origin` must be the column the assembler's last run wrote, unchanged: that no two cells name one event is what makes every routed entry the
 * store of exactly one lane. An origin column that names an event twice is not refused (RG_MEM_DEVICE does not read it on the host); which of the two cells such an entry
 * then shows is not defined, and nothing outside the routed columns is written.
 *
 * MEMSPACES. RG_MEM_DEVICE: every pointer of both structs is device-visible (rg_dev_alloc / rg_host_alloc); the call is asynchronous on the table's stream,
 * synchronises nothing and decides nothing on the host from device data — its grids are sized from the capacities and leave early on the n / R / m / e they read.
 * So rg_assemble32 -> rg_tick2_launch -> rg_route32 queue back to back with no host step between them (the first run of a shape allocates the route's scratch, a
 * few KiB of per-wavefront counts). RG_MEM_HOST: host arrays, staged in and out, synchronous; only what the run wrote is copied back.
 * Refused (-1, with a message, before any launch): NULL structs or required columns (gid, count, rounds, origin, row, persist32; cell, row, persist32 of the
 * arrival order unless arrival_capacity is 0; counts; a list unless its capacity is 0; send_offset with a send table), C = 0 or above the group count, D outside
 * 1 .. 64, C, D or an arrival / expired capacity that differs from those of the assembler's last run, an assembler that has not run yet, a send table or an
 * expired triple given in part, an unknown memspace and, in RG_MEM_DEVICE, a pointer that is neither device memory nor page-locked host memory. */
#define RG_ROUTE_NONE 0xFFFFFFFFu
typedef struct { uint32_t cell; uint32_t gid; } rg_route_item_t;   /* persist_list, attention */
typedef struct { uint32_t row;  uint32_t gid; } rg_send_item_t;    /* send_list */
typedef struct {                       /* the batch rg_assemble32 made, and what the launch that decided it wrote over it */
    uint32_t              capacity;    /* C */
    uint32_t              max_rounds;  /* D */
    const uint32_t       *gid, *count, *rounds, *origin;   /* the assembler's columns: [C], [1], [1], [D][C] */
    const rg_out32_t     *row;         /* [D][C] */
    const rg_persist32_t *persist32;   /* [D][C] */
    const rg_send_head_t *send_head;   /* [C] or NULL */
    const rg_send_t      *send;        /* [(P-1) * C] or NULL: both or neither */
} rg_decided_t;
typedef struct {
    uint32_t         arrival_capacity;                       /* that of the assembler's last run */
    uint32_t        *cell;                                   /* [arrival_capacity] */
    rg_out32_t      *row;                                    /* [arrival_capacity] */
    rg_persist32_t  *persist32;                              /* [arrival_capacity] */
    uint32_t         expired_capacity;                       /* with the three columns below: that of the assembler's last run (0 with no expired source) */
    uint32_t        *expired_cell;                           /* [expired_capacity] or NULL: all three or none (none: a cell that answers a fired ticket is routed nowhere) */
    rg_out32_t      *expired_row;
    rg_persist32_t  *expired_persist32;
    rg_route_item_t *persist_list;  uint32_t persist_capacity;
    rg_route_item_t *attention;     uint32_t attention_capacity;
    rg_send_item_t  *send_list;     uint32_t send_capacity;
    uint32_t        *send_offset;                            /* [P] */
    uint32_t        *counts;                                 /* [4] */
} rg_routed_t;
int rg_route32(rg_assembler_t *a, const rg_decided_t *in, const rg_routed_t *out, int memspace);

/* ---- CARRYING DEFERRED EVENTS INTO THE NEXT RUN (new symbols only; the ABI stays 6) ---------------------------------------------------------------
 * An event is DEFERRED when its group already has max_rounds events in the batch or falls outside the `capacity` smallest groups of the run. Above, the host
 * puts such events at the head of its next arrival log by hand — which means waiting for the run, reading stats and deferred[], copying rows and shifting every
 * reader's index. A CARRY moves that recipe onto the device: the assembler keeps what it deferred, the next run takes it first, in order, and the route tells
 * every reader where its event went. It is OFF by default; with the carry off every entry point behaves exactly as described above, bit for bit.
 *
 * rg_assembler_carry_enable gives the assembler two carries of carry_capacity slots each, in its own device memory (0 takes them away again); it waits for the
 * table's stream, sizes the scratch for max_events + max_expired + carry_capacity positions and leaves both carries empty (if it runs out of memory, -2, the
 * assembler holds no scratch and rg_assemble32 refuses it until an enable succeeds). A slot holds a complete compact row
 * (gid, head, abcd). The two carries alternate: a run reads one and leaves the other; which is which follows the host's count of the calls and is never device data.
 *
 * THE SEQUENCE S of a run on a carrying assembler: the expired source as above; then the carry, slots c = 0 .. q - 1 — q is the count the previous run left, 0
 * after enable and after reset, read on the device —; then the arrival log as above. A slot moves into its cell verbatim; its id, in origin and in deferred[], is
 * RG_ASM_CARRIED | c. For the same inputs the columns gid, count, rounds, head and abcd equal, bit for bit, what a run without a carry produces when the host
 * prepends the deferred rows to its log by hand; origin and deferred differ by that relabelling of the ids only.
 *
 * AFTER THE RUN the events it deferred, in S order, are the next carry: slot p holds the event at position p of the run's deferred sequence — what deferred[p]
 * names, whatever deferred_capacity is (deferred may be NULL with a capacity of 0) —, a fired ticket as the row the assembler would have made of it,
 * {RG_HDR_MAKE of RG_EV_TIMEOUT, epoch} with a zero quad. The carry takes the first min(stats[1], carry_capacity) of them; stats[3], 0 on an assembler without a
 * carry, is the number that did not fit, the SPILLED events. Spilled arrivals and tickets are still with the host, their ids are deferred[p] for p >=
 * carry_capacity; a spilled event that was itself carried can be fetched with rg_assembler_carry_read of RG_CARRY_LAST until the next run. An event with a bad
 * gid is never carried. Every output and the new carry are a function of the inputs and the old carry alone, bit for bit, run after run.
 *
 * rg_assembler_carry_reset empties the carry the next run will read (asynchronous on the table's stream). rg_assembler_carry_read copies a carry to host arrays:
 * *count = its slots, of which the first min(*count, capacity) are written; it waits for the stream: for draining, recovery and tests.
 *
 * rg_route32_carry does everything rg_route32 does, for the last run of a carrying assembler, and on top of it:
 *   - carried->cell / row / persist32 hold [carry_capacity] entries. For every slot c < q that the routed run read, cell[c] is ALWAYS written; row[c] and
 *     persist32[c] are written iff the slot was placed, and iff its flags carry RG_F_PERSIST, as for an arrival. Entries >= q are NOT TOUCHED.
 *   - every event the run read has ONE of four values in its cell entry — cell[k], expired_cell[j], carried->cell[c] —: the cell index (below 2^31);
 *     RG_ROUTE_CARRIED | s, the event was deferred into slot s of the carry the NEXT run reads; RG_ROUTE_SPILLED, it was deferred and the carry had no room: the
 *     host still owns it; RG_ROUTE_NONE, its gid was bad.
 *   - a reader follows k -> RG_ROUTE_CARRIED | s -> carried->cell[s] of the NEXT run's route, and so on, until it reads a cell.
 * Plain rg_route32 on a carrying assembler stays what it is: a deferred event gets RG_ROUTE_NONE, a cell that answers a carried slot is routed nowhere.
 *
 * HOST DUTIES. rg_index_base_set on a group that has carried rows is the host's error: the rows stay relative to the old base. An entry-terms slot that a
 * carried AppendEntries row addresses through `aux` must stay in place in the array handed to later launches until that row's cell is routed; a row with
 * RG_HDR_SAME_TERM needs nothing.
 *
 * MEMSPACES as for the two calls above. The carry always lives in the assembler's device memory: an RG_MEM_HOST run reads it and leaves it there. In
 * RG_MEM_DEVICE everything is asynchronous on the table's stream, grids are sized from the capacities — carry_capacity among them — and leave early on the counts
 * they read; no kernel waits for another workgroup.
 * Refused (-1, with a message, before any launch): enabling a carry with max_events, max_expired or carry_capacity at or above 2^30 (bit 30 marks a carried id);
 * rg_assembler_carry_reset, rg_assembler_carry_read and rg_route32_carry on an assembler without a carry; a carried->capacity that differs from the carry's; a
 * missing carried column; C x D above 2^31 (the RG_ROUTE_CARRIED bit must stay free); an unknown `which`; and rg_assemble32 on a carrying assembler whose table
 * has RG_OPT_AUTO_INDEX_BASE set: a base that a decided RG_EV_LOG_FLUSH row moves would leave the same group's carried rows relative to the old base. */
#define RG_ASM_CARRIED   0x40000000u   /* origin / deferred id of carry slot c: RG_ASM_CARRIED | c */
#define RG_ROUTE_CARRIED 0x80000000u   /* a routed `cell` entry: the event was deferred into slot (value & 0x3FFFFFFF) of the carry the NEXT run reads */
#define RG_ROUTE_SPILLED 0xFFFFFFFEu   /* deferred, and the carry had no room: the host still owns this event */
#define RG_CARRY_NEXT 0                /* the carry the next run will read */
#define RG_CARRY_LAST 1                /* the carry the last run read (intact until the next run) */
int rg_assembler_carry_enable(rg_assembler_t *a, uint32_t carry_capacity);   /* 0 disables; (re)sizes scratch, empties the carry */
int rg_assembler_carry_reset(rg_assembler_t *a);                             /* empties RG_CARRY_NEXT; asynchronous on the table's stream */
int rg_assembler_carry_read(rg_assembler_t *a, int which, uint32_t capacity, uint32_t *count,
                            uint32_t *gid, rg_ev_head_t *head, rg_ev_quad32_t *abcd);   /* host arrays, synchronous: draining, recovery, tests */
typedef struct { uint32_t capacity; uint32_t *cell; rg_out32_t *row; rg_persist32_t *persist32; } rg_routed_carry_t;   /* [capacity] each */
int rg_route32_carry(rg_assembler_t *a, const rg_decided_t *in, const rg_routed_t *out, const rg_routed_carry_t *carried, int memspace);

/* ---- WHICH GROUPS NEED THE HOST, AND STATE BY A LIST OF GROUPS (new symbols only; the ABI stays 6) ---------------------------------------------------
 * A host with 65 536 to a million groups asks the table two things that rg_read_state over the whole table — some 200 bytes a group at five nodes, through
 * 5 + K + 2(P-1) copies — answers far too dearly: WHICH groups are in a given condition, and the state of EXACTLY these groups, out or in. Both are plain device
 * work and touch no decision.
 *
 * rg_scan: ONE STREAMING PASS OVER THE TABLE. Every group gets a CLASS WORD, the bits below, from its state, its timer ticket, its index base and the three
 * thresholds of the query. A group is SELECTED iff (any == 0 || (word & any) != 0) && (word & all) == all && (word & none) == 0.
 *   - bits (optional, [groups]): the class word of EVERY group.
 *   - list: the gids of the first min(selected, list_capacity) selected groups, ASCENDING. Entries beyond that are NOT TOUCHED; NULL with a capacity of 0 is legal.
 *   - summary[RG_SCAN_SUMMARY] (required): [b], b < 16, the number of groups with bit b set; [16] the number of selected groups — the true count, which may exceed
 *     list_capacity; [17] the largest current_term; [18] the largest and [19] the sum of last_index - commit_index over the groups with a log, a negative
 *     difference counting as 0; [20] the largest last_index - match_index[j] over the followers of prepared leaders with a log, likewise; [21 .. 23] are 0.
 * Every output is a function of the table and the query alone, bit for bit, run after run: the list is compacted by ballot, popcount and prefix sum, nothing is
 * appended through an atomic, and no kernel waits for another workgroup. It works for every cluster size a table takes, with no option.
 *
 * RG_SCAN_OFF_IMAGE says that a compact-row launch (rg_submit32, rg_submit32c*, the ticks) cannot START this group's workgroup on the 32-bit body: the 64 groups
 * it shares a workgroup with are then decided in 64 bits, which rg_wide_body_workgroups counts and this bit locates. It is the state's half of that check — a term
 * or an index (relative to the group's index base: "the index base of the compact formats") outside [0, 2^30), a role epoch, vote count or node slot outside its
 * domain, an epoch.index at or below a non-zero base, a negative base, a follower record of a prepared group without an image — on the words the step kernel
 * itself loads: for a group whose log is EMPTY that includes the window and run slot 0 the log's last flush left behind in the table, which rg_read_state reports
 * as zeros. The peer columns of an UNPREPARED group are not looked at, whatever they hold, as the step kernel does not stage them. What belongs to a launch — a
 * table built with RG_FORCE_WIDE=1, a row outside the format's domain, a value that leaves the image while the launch runs — is not the state's and is not here.
 *
 * MEMSPACES, as the route's. RG_MEM_DEVICE: bits, list and summary are device-visible (rg_dev_alloc / rg_host_alloc); the call is asynchronous on the table's
 * stream, synchronises nothing and decides nothing on the host from device data — its grids are sized from the group count, so a scan queues right behind
 * rg_tick2_launch. Its scratch, 12 bytes per wavefront of groups and 192 per workgroup, is the table's: allocated by the first scan, freed with the table.
 * RG_MEM_HOST: host arrays, staged out, synchronous; of the list only what was written is copied back.
 * Refused (-1, with a message, before any launch): a NULL query, result or summary; a NULL list with a capacity other than 0; reserved != 0; a mask bit above 15;
 * backlog or lag outside [0, 2^62]; an unknown memspace and, in RG_MEM_DEVICE, a pointer that is neither device memory nor page-locked host memory. */
#define RG_SCAN_FOLLOWER         (1u << 0)
#define RG_SCAN_CANDIDATE        (1u << 1)
#define RG_SCAN_LEADER           (1u << 2)
#define RG_SCAN_NO_LEADER        (1u << 3)   /* Follower and current_leader == RG_NO_NODE */
#define RG_SCAN_TIMEOUT_DETECTED (1u << 4)
#define RG_SCAN_EMPTY_LOG        (1u << 5)   /* run_count == 0 */
#define RG_SCAN_RUNS_FULL        (1u << 6)   /* run_count == RG_TERM_RUNS: the next run pushes the oldest out, a lookup into it answers RG_NEED_HOST */
#define RG_SCAN_BACKLOG          (1u << 7)   /* log not empty and last_index - commit_index > backlog */
#define RG_SCAN_UNPREPARED       (1u << 8)   /* Leader and !repl_prepared */
#define RG_SCAN_PENDING_INSTALL  (1u << 9)   /* prepared Leader, some follower's pendingInstallation set */
#define RG_SCAN_LAGGING          (1u << 10)  /* prepared Leader, log not empty, some follower j: last_index - match_index[j] > lag */
#define RG_SCAN_OFF_IMAGE        (1u << 11)  /* the group's state cannot START a compact launch on the 32-bit body (above) */
#define RG_SCAN_HAS_BASE         (1u << 12)  /* index base != 0 */
#define RG_SCAN_NO_TICKET        (1u << 13)  /* timer deadline == 0 */
#define RG_SCAN_TICKET_FIRED     (1u << 14)  /* timer deadline == -1 */
#define RG_SCAN_OVERDUE          (1u << 15)  /* deadline > 0 and deadline <= now */
#define RG_SCAN_SUMMARY 24
typedef struct { uint32_t any, all, none; uint32_t reserved; int64_t backlog, lag, now; } rg_scan_query_t;
typedef struct {
    uint32_t *bits;                              /* optional [groups]: the class word of every group */
    uint32_t *list; uint32_t list_capacity;      /* gids of the selected groups, ASCENDING; NULL with capacity 0 is legal */
    uint64_t *summary;                           /* [RG_SCAN_SUMMARY], required */
} rg_scan_result_t;
int rg_scan(rg_table_t *t, const rg_scan_query_t *q, const rg_scan_result_t *out, int memspace);

/* STATE BY LIST: rg_read_state / rg_load_state for the n groups gid[0 .. n), host arrays, synchronous. Element i of every column is group gid[i], in exactly the
 * layout the range calls have for count = n: run_offset[i] = i * RG_TERM_RUNS on read, the peers of element i at i * (P - 1) + j. A gather (scatter) kernel packs
 * the listed groups' columns into (out of) one contiguous image in device memory — the table's, grown on demand, freed with the table; running out answers -2 — so
 * the number of copies does not depend on n or on how the gids are scattered: two per call. n = 0 returns 0; n above the group count is refused.
 * READ takes the gids in any order, repeats included; a gid at or above the group count is refused, the message names its index, and nothing is written.
 * LOAD wants DISTINCT gids — a repeat is refused and named — and validates every row as rg_load_state does, the group number in the message being the gid, BEFORE
 * anything reaches the device: a refused call changes nothing. The listed groups get exactly what rg_load_state gives them — the state, no timer ticket, the
 * timers' role epoch, zeroed health statistics and, with RG_OPT_DEVICE_IN_FLIGHT, nothing in flight — and every other group of every column stays bit for bit
 * what it was. */
int rg_read_state_list(rg_table_t *t, uint32_t n, const uint32_t *gid, rg_group_state_t *dst);
int rg_load_state_list(rg_table_t *t, uint32_t n, const uint32_t *gid, const rg_group_state_t *src);

/* ---- WHAT A LAUNCH ASKS THE HOST TO DO, AS LISTS (new symbols only; the ABI stays 6) ---------------------------------------------------------------
 * rg_submit32c, rg_submit32c_sparse(_rounds) and a rg_tick2_* tick write rg_out32_t row[D][C], and three consumers of a host then each walk all D x C rows to find
 * the few that carry an instruction for them: the log writer wants the cells with RG_F_LOG_APPEND or RG_F_LOG_TRUNC (RaftLog.truncate / append), the applier
 * wants one line per group whose commitIndex moved (RaftContext.commitLog -> RaftRoutine.commitState), the repair path wants the RG_NEED_HOST cells. rg_route32
 * builds such lists only behind an assembler, and neither of the first two. rg_effects32 builds all three from the rows alone, on the device, whatever wrote them.
 *
 * THE ROWS. C = capacity is the row stride of a round, D = max_rounds; cell = r * C + i names row i of round r. n = min(*count, C) and R = clamp(*rounds, 1, D) are
 * read when the run executes, as the tick reads them; a NULL count means n = C, a NULL rounds R = D. Row i belongs to group gid[i], or to group i when gid is NULL
 * (a dense batch): that is the `gid` of every item below.
 *
 * THE RESULT.
 *   - log_list: {cell, gid} of every cell (r < R, i < n) whose flags carry RG_F_LOG_APPEND or RG_F_LOG_TRUNC, in ascending cell order — round-major, so one group's
 *     log writes stay in their order. The reader takes log_from and the two flags from row[cell].
 *   - attention: the same for every cell whose status is RG_NEED_HOST.
 *   - commit_list: ONE item per row i < n that has at least one round r < R with RG_F_COMMIT, in ascending i. cell is the cell of the LAST such round;
 *     commit_index and flags are that cell's two words VERBATIM. commit_index is relative to the index base the launch STARTED with, as the rows are: the call does
 *     not convert it, because the table's base may already have moved (RG_OPT_AUTO_INDEX_BASE). flags lets the reader see RG_F_WIDE_VALUES and go to the overflow
 *     columns by `cell`.
 *   - counts[4] = {log items, commit items, attention items, 0}: the true numbers. A count may exceed its list's capacity: the first `capacity` items in the
 *     stated order are then written. List entries beyond what was written are NOT TOUCHED; a NULL list with a capacity of 0 is legal. Rows >= n and rounds >= R
 *     are not read.
 * Every output is a function of the inputs alone, bit for bit, run after run: the lists are compacted by ballot, popcount and prefix sum, nothing is appended
 * through an atomic, no kernel waits for another workgroup, and every loop is bounded by R or by a span computed on the host.
 *
 * MEMSPACES, as the route's. RG_MEM_DEVICE: every pointer of both structs is device-visible (rg_dev_alloc / rg_host_alloc); the call is asynchronous on the
 * table's stream, synchronises nothing and decides nothing on the host from device data — its grids are sized from C and D and leave early on the n and R they
 * read. So it queues right behind rg_submit32c*(RG_MEM_DEVICE), or behind rg_tick2_launch with the tick's own count / rounds words, with no host step in between.
 * Its scratch, three words per wavefront of cells or rows, is the table's: allocated by the first call of a shape, freed with the table. RG_MEM_HOST: host
 * arrays, staged in (rows 0 .. n - 1 of rounds 0 .. R - 1) and out, synchronous; of the lists only what was written is copied back.
 * Refused (-1, with a message, before any launch): NULL structs, a NULL row or counts; a NULL list with a capacity other than 0; C = 0 or above the group count;
 * D = 0 or at or above 2^24 (the rounds of one compact launch, rg_submit32); D x C at or above 2^32; an unknown memspace; in RG_MEM_DEVICE a pointer that is
 * neither device memory nor page-locked host memory; in RG_MEM_HOST a gid[i], i < n, at or above the group count — the message names it. RG_MEM_DEVICE trusts the
 * list, as the sparse submit does. Wide rows (rg_outcome_t) are not taken. */
typedef struct { uint32_t cell; uint32_t gid; int32_t commit_index; uint32_t flags; } rg_commit_item_t;   /* 16 B: commit_list */
typedef struct {
    uint32_t          capacity;    /* C: the row stride of a round, 1 .. groups */
    uint32_t          max_rounds;  /* D */
    const uint32_t   *gid;         /* [C], or NULL: row i is group i (a dense batch) */
    const uint32_t   *count;       /* [1], or NULL: n = C */
    const uint32_t   *rounds;      /* [1], or NULL: R = D */
    const rg_out32_t *row;         /* [D][C] */
} rg_effects_in_t;
typedef struct {
    rg_route_item_t  *log_list;    uint32_t log_capacity;
    rg_commit_item_t *commit_list; uint32_t commit_capacity;
    rg_route_item_t  *attention;   uint32_t attention_capacity;
    uint32_t         *counts;      /* [4] = {log items, commit items, attention items, 0}, required */
} rg_effects_t;
int rg_effects32(rg_table_t *t, const rg_effects_in_t *in, const rg_effects_t *out, int memspace);

/* ---- device memory helpers (so a host without its own HIP binding can keep batches in HBM) --- */
/* Page-locked host memory for RG_MEM_HOST batches (JNI: wrap it with NewDirectByteBuffer): staging then runs at PCIe
 * speed instead of through the driver's pageable bounce buffers. */
int rg_host_alloc(rg_table_t *t, size_t bytes, void **hptr);
int rg_host_free(rg_table_t *t, void *hptr);
int rg_dev_alloc(rg_table_t *t, size_t bytes, void **dptr);
int rg_dev_free(rg_table_t *t, void *dptr);
int rg_copy_to_device(rg_table_t *t, void *dst, const void *src, size_t bytes);
int rg_copy_to_host(rg_table_t *t, void *dst, const void *src, size_t bytes);
void *rg_stream(rg_table_t *t);   /* the table's hipStream_t */

/* ---- measurement ---------------------------------------------------------------------------- */
/* When enabled every rg_submit brackets its step kernel with HIP events on the table's stream. */
int rg_timing_enable(rg_table_t *t, int on);
/* Sum and count of step-kernel durations since the last reset (synchronises the stream). */
int rg_timing_read(rg_table_t *t, uint64_t *launches, double *total_ms, int reset);
/* One event pair around a whole REGION of submissions on the table's stream (cheaper than per-launch pairs, which
 * put two timestamp packets between consecutive kernels): rg_timing_begin records the start event,
 * rg_timing_end records the stop event, synchronises, and returns the elapsed milliseconds. */
int rg_timing_begin(rg_table_t *t);
int rg_timing_end(rg_table_t *t, double *elapsed_ms);
/* Device-side decision counters accumulated by the step kernel (per-lane tallies, summed over the wavefront with a
 * shuffle butterfly at the end of the launch and added to the wavefront's own slot of a table — no atomics): [0]=rows with kind!=NONE, [1]=replied, [2]=role conversions, [3]=commit advances,
 * [4]=assert statuses, [5]=NEED_HOST, [6]=dropped stale, [7]=log appends. */
#define RG_NUM_COUNTERS 8
int rg_counters_read(rg_table_t *t, uint64_t counters[RG_NUM_COUNTERS], int reset);
/* Workgroups (64 groups each) of compact-row launches (rg_submit32 / rg_submit32c / rg_submit_async_packed) that were decided by the 64-bit body since the
 * last reset: a value of theirs left the 32-bit image (include/raftgpu.h, rg_submit32; with index bases: "the index base of the compact formats"). Results
 * are the same either way; the count tells a host that groups have outgrown their bases. Waits for the stream.
 * WHICH groups: rg_scan with RG_SCAN_OFF_IMAGE in `any` lists them. */
int rg_wide_body_workgroups(rg_table_t *t, uint64_t *count, int reset);
/* Plain streaming-copy kernel over `bytes` of scratch on this device: returns achieved GB/s
 * (read+write) — the measured-copy roofline reported next to the 8 TB/s spec. */
int rg_copy_bandwidth(rg_table_t *t, size_t bytes, int iters, double *gbps);

#ifdef __cplusplus
}
#endif
#endif /* RAFTGPU_H */
