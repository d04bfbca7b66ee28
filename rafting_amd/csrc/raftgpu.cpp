// raftgpu.cpp — host side of libraftgpu.so: the C-ABI of include/raftgpu.h over the gfx950 kernels.
//
// Owns, per table: the HBM structure-of-structs state (rg_device.hpp DevTable), one HIP stream, grow-only
// staging buffers for RG_MEM_HOST submissions, device decision counters and a pool of HIP event pairs for
// kernel timing.  There is no CPU fallback: every entry point that needs the GPU fails with a HIP error
// string when no device is present.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "rg_device.hpp"
#include "rg_assemble.hpp"
#include "rg_route.hpp"
#include "rg_scan.hpp"
#include "rg_effects.hpp"

using rg::DevTable;
using rg::I64x2;

struct Staging {
    void *ptr = nullptr;
    size_t cap = 0;
};

// the columns of one batch on the device (RG_MEM_HOST): the wide rows, the compact rows, the outcome in both forms, the per-wavefront list counts of the packed
// outcome. One set per owner — the table's serial path, every pipeline slot, a recorded tick — freed by walking it
enum Col { C_GID, C_HEAD, C_AB, C_CD, C_HINT, C_TERMS, C_ABCD32, C_TERMS32, C_REPLY, C_LOGFX, C_PERSIST, C_OUT32, C_PERSIST32, C_COUNTS, C_COLUMNS };
struct BatchCols {
    Staging col[C_COLUMNS];
    Staging &operator[](Col c) { return col[c]; }
};

// the table's buffers of the small entry points: rg_replicate (heartbeat, in-flight, send heads, send rows), rg_timers_expired, rg_health_failure, rg_ready
enum Aux { X_HB, X_FL, X_SH, X_SS, X_TGID, X_HGID, X_HSLOT, X_HFLAG, X_HDONE, X_READY, X_COLUMNS };
// ... of rg_scan (its scratch: per-wavefront counts and ballots, per-workgroup partial summaries; RG_MEM_HOST: the three outputs) and of the state lists (the
// gids and the image of their columns)
enum Scan { S_WC, S_SEL, S_PART, S_BITS, S_LIST, S_SUMMARY, L_GID, L_IMAGE, S_COLUMNS };
// ... of rg_effects32 (its scratch: the per-wavefront counts of the three lists; RG_MEM_HOST: the words n and R, the batch's gid and row columns, the outputs)
enum Effects { E_LC, E_AC, E_CC, E_WORDS, E_GID, E_ROW, E_LOG, E_COMMIT, E_ATTENTION, E_COUNTS, E_COLUMNS };

struct PipeSlot {                               // one batch in flight on the pipelined host-memory path (rg_submit_async)
    BatchCols c;
    hipEvent_t up = nullptr, done = nullptr, down = nullptr;
};

struct rg_table {
    int device = 0;
    uint32_t G = 0, P = 0, self = 0, F = 0;
    int pre_vote = 0;
    hipStream_t stream = nullptr;
    DevTable dt{};
    unsigned long long *counters = nullptr;     // [counter_slots][RG_NUM_COUNTERS], one slot per wave of a dense launch
    unsigned long long *wide_bodies = nullptr;  // one word (rg_wide_body_workgroups)
    size_t counter_slots = 0;
    int fast_paths = 1;                         // RG_FAST=0: general handlers only (differential tests)
    int force_wide = 0;                         // RG_FORCE_WIDE=1: the compact-format kernel skips its 32-bit body (differential tests)
    int require_fence = 0;                      // rg_table_option(RG_OPT_REQUIRE_FENCED_TIMEOUTS)
    int has_bases = 0;                          // rg_index_base_set has stored a non-zero base at some time (or RG_OPT_AUTO_INDEX_BASE was switched on)
    int auto_window = 0;                        // rg_table_option(RG_OPT_AUTO_INDEX_BASE): 0 = off
    int compact_any_cluster = 0;                // rg_table_option(RG_OPT_COMPACT_ANY_CLUSTER): the compact formats and the ticks take a cluster above RG_MAX_COMPACT_CLUSTER
    int lanes = -1;                             // -1: pick per launch; 0: split kernel; 64: single-wavefront kernel (RG_SPLIT env forces one)
    uint32_t simds = 1024;                      // SIMDs of the device (CUs x 4)
    BatchCols st;                               // the serial RG_MEM_HOST path: one batch at a time, shared by every entry point that stages one of its columns
    Staging aux[X_COLUMNS];
    Staging scan[S_COLUMNS];
    Staging fx[E_COLUMNS];
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    uint64_t t_launches = 0;
    double t_total_ms = 0.0;
    hipEvent_t region0 = nullptr, region1 = nullptr;
    int64_t *timer_deadline = nullptr;          // [G] N4
    uint32_t *timer_epoch = nullptr;            // [G] role epoch after the last batch the timers saw (rg_timers_update32 chains compact rows from it)
    unsigned long long *tick_masks = nullptr;   // [ceil(G / 256) * 4 >= workgroups of any tick kernel] status words of the expiry's look-back (rg_kernels.hip: expire_tail)
    uint32_t *tick_ticket = nullptr;            // [1] their generation
    uint64_t config_gen = 0;                    // bumped by whatever changes what a recorded launch has baked in (options, the first index base)
    std::vector<struct rg_tick *> ticks;        // live recordings: invalidated when the table goes
    std::vector<struct rg_tick2 *> ticks2;
    std::vector<struct rg_assembler *> assemblers;   // live assemblers (rg_assembler_create): their scratch goes with the table
    uint32_t *timer_counts = nullptr;           // [waves + 1]: per-wave counts / offsets, last = total
    int64_t election_ms = 900, heartbeat_ms = 300;   // raft1.xml:10-13
    uint64_t timer_seed = 0;
    int64_t *health_ok = nullptr, *health_fail = nullptr;   // [F][G] N4b
    int32_t *health_recent = nullptr;
    uint16_t *in_flight = nullptr;              // [F][G] State.requestInFlight; allocated while rg_table_option(RG_OPT_DEVICE_IN_FLIGHT) is 1, nullptr otherwise
    hipStream_t s_in = nullptr, s_out = nullptr; // copy-in / copy-out streams of the pipelined path
    PipeSlot pipe[RG_PIPELINE_DEPTH];
    uint64_t pipe_head = 0, pipe_tail = 0;       // batches submitted / waited for
    std::string err;
};

static thread_local std::string g_create_err;

static int fail(rg_table *t, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (t) t->err = buf; else g_create_err = buf;
    return code;
}

#define HIP_TRY(t, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail((t), -2, "%s failed: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

static int wait_oldest(rg_table *t)
{
    if (t->pipe_tail == t->pipe_head) return 1;
    HIP_TRY(t, hipEventSynchronize(t->pipe[t->pipe_tail % RG_PIPELINE_DEPTH].down));
    t->pipe_tail += 1;
    return 0;
}

// every entry point starts here: select the device and (unless the caller IS the pipeline) let batches in flight land first
static int bind(rg_table *t, bool drain = true)
{
    HIP_TRY(t, hipSetDevice(t->device));
    while (drain && t->pipe_tail != t->pipe_head)
        if (int rc = wait_oldest(t); rc < 0) return rc;
    return 0;
}

static int reserve(rg_table *t, Staging &s, size_t bytes)
{
    if (bytes <= s.cap) return 0;
    if (s.ptr) HIP_TRY(t, hipFree(s.ptr));
    s.ptr = nullptr; s.cap = 0;
    size_t cap = bytes + bytes / 4 + 4096;
    HIP_TRY(t, hipMalloc(&s.ptr, cap));
    s.cap = cap;
    return 0;
}

// every buffer of an owner, by walking its array (called with the table's device current and its stream idle)
static void release(Staging *s, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        if (s[i].ptr) (void)hipFree(s[i].ptr);
        s[i] = Staging{};
    }
}

// The typed forms of staging. T is the header's type of an element, D the device code's: the same bytes under two names (rg_ev_pair_t and I64x2, ...).
// col_up / col_down move `n` elements, from element `at` on, between a host column and the same place of its staging buffer; n == 0 copies nothing. They return
// the HIP error: a chain recorded under a stream capture, which must always be ended, uses them as they are.
template <class T>
static hipError_t col_up(const Staging &s, const T *src, size_t at, size_t n, hipStream_t st)
{
    return n ? hipMemcpyAsync((T *)s.ptr + at, src + at, n * sizeof(T), hipMemcpyHostToDevice, st) : hipSuccess;
}

template <class T>
static hipError_t col_down(const Staging &s, T *dst, size_t at, size_t n, hipStream_t st)
{
    return n ? hipMemcpyAsync(dst + at, (const T *)s.ptr + at, n * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
}

// "this host column of n elements, on the device, on this stream": reserve, copy, the typed device pointer
template <class D, class T>
static int stage_in(rg_table *t, Staging &s, const T *src, size_t n, hipStream_t st, const D **dev)
{
    static_assert(sizeof(D) == sizeof(T), "one element under two names");
    if (reserve(t, s, n * sizeof(T))) return -2;
    HIP_TRY(t, col_up(s, src, 0, n, st));
    *dev = (const D *)s.ptr;
    return 0;
}

// an output-only column of n elements: reserve, the typed device pointer
template <class D>
static int stage_out(rg_table *t, Staging &s, size_t n, D **dev)
{
    if (reserve(t, s, n * sizeof(D))) return -2;
    *dev = (D *)s.ptr;
    return 0;
}

// ... or a column the device only reads, whose copy comes later (a recorded one)
template <class D>
static int stage_out(rg_table *t, Staging &s, size_t n, const D **dev) { return stage_out(t, s, n, const_cast<D **>(dev)); }

// "bring n elements back"
template <class T>
static int stage_back(rg_table *t, const Staging &s, T *dst, size_t n, hipStream_t st)
{
    HIP_TRY(t, col_down(s, dst, 0, n, st));
    return 0;
}

static int drain_timing(rg_table *t)
{
    if (t->ev_used == 0) return 0;
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    for (size_t i = 0; i < t->ev_used; i++) {
        float ms = 0.f;
        HIP_TRY(t, hipEventElapsedTime(&ms, t->ev_pool[i].first, t->ev_pool[i].second));
        t->t_total_ms += ms;
        t->t_launches += 1;
    }
    t->ev_used = 0;
    return 0;
}

/* a recorded launch: what the once-per-tick path (rg_tick_*) and the device-resident tick (rg_tick2_*) have in common: see include/raftgpu.h */
struct Recording {
    rg_table *t = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    uint64_t config_gen = 0;         // the table's at creation: has_bases, require_fence, fast_paths, force_wide are baked into the recorded kernel node
    bool in_flight = false;

    // everything a recording holds on the device; afterwards it knows no table (called with the table's device current and its stream idle)
    void release()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr; graph = nullptr;
        t = nullptr;
    }
};

struct rg_tick : Recording {         // owns the staging its recorded copies go through
    BatchCols c;
    void release() { ::release(c.col, C_COLUMNS); Recording::release(); }
};

struct rg_tick2 : Recording {};      // owns none: its rows are device-visible where they lie

template <class K>
static int recording_destroy(K *k, std::vector<K *> rg_table::*list)
{
    if (!k) return 0;
    if (rg_table *t = k->t) {
        (void)hipSetDevice(t->device);
        if (t->stream) (void)hipStreamSynchronize(t->stream);
        std::vector<K *> &live = t->*list;
        live.erase(std::remove(live.begin(), live.end(), k), live.end());
        k->release();
    }
    delete k;
    return 0;
}

static int recording_wait(Recording *k)
{
    if (!k || !k->t) return -1;
    rg_table *t = k->t;
    HIP_TRY(t, hipSetDevice(t->device));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    k->in_flight = false;
    return 0;
}

// a recording is launched under the configuration it was created under; then the table is bound (every batch in flight lands first)
static int recording_bind(Recording *k, const char *launch, const char *create)
{
    if (!k || !k->t) return -1;
    rg_table *t = k->t;
    if (k->config_gen != t->config_gen)
        return fail(t, -1, "%s: the table's options or index bases changed after %s (they are part of the recording): create the tick again", launch, create);
    return bind(t) ? -2 : 0;
}

// the tail of a capture on the table's stream, e being what the recorded chain gave: end it (always: an open capture would poison the stream), take the first
// error, instantiate. On failure the sticky error is cleared; the caller destroys the recording
static hipError_t recording_finish(Recording *k, hipError_t e)
{
    hipGraph_t g = nullptr;
    const hipError_t e2 = hipStreamEndCapture(k->t->stream, &g);
    k->graph = g;
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess) e = hipGraphInstantiate(&k->exec, k->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

// the shape of a submission, whatever the format of its rows: what the shape rules and step_params read
struct Shape {
    uint32_t rounds, count;
    const uint32_t *gid;            // nullptr: a dense batch
    uint64_t entry_count;
    bool entry_terms;               // the column is there
};

template <class Batch>
static Shape shape_of(const Batch *in) { return Shape{in->rounds, in->count, in->gid, in->entry_count, in->entry_terms != nullptr}; }

// At most 64 clock values travel in the kernel arguments of one launch: the rounds of a timer or health update go in chunks of 64. `base` holds what every
// chunk shares; launch(p, r0) points p at the rows from round r0 on and launches it
template <class Params, class Launch>
static int clock_chunks(rg_table *t, uint32_t rounds, const int64_t *now, const Params &base, Launch launch)
{
    for (uint32_t r0 = 0; r0 < rounds; r0 += 64) {
        Params p = base;
        p.rounds = rounds - r0 < 64 ? rounds - r0 : 64;
        for (uint32_t k = 0; k < p.rounds; k++) p.now[k] = now[r0 + k];
        HIP_TRY(t, launch(p, r0));
    }
    return 0;
}

extern "C" {

int rg_abi_version(void) { return RG_ABI_VERSION; }

const char *rg_last_error(const rg_table_t *t) { return t ? t->err.c_str() : g_create_err.c_str(); }
uint32_t rg_table_groups(const rg_table_t *t) { return t ? t->G : 0; }
uint32_t rg_table_cluster(const rg_table_t *t) { return t ? t->P : 0; }

int rg_table_option(rg_table_t *t, int option, int value)
{
    if (!t) return -1;
    switch (option) {
    case RG_OPT_REQUIRE_FENCED_TIMEOUTS:
        if (t->require_fence != (value != 0)) t->config_gen += 1;       // (a recorded tick has the old value baked in: rg_tick_launch refuses it)
        t->require_fence = value != 0;
        return 0;
    case RG_OPT_AUTO_INDEX_BASE:
        if (value < 0 || value >= (1 << 30)) return fail(t, -1, "rg_table_option: RG_OPT_AUTO_INDEX_BASE window %d outside [0, 2^30)", value);
        if (t->auto_window != value) t->config_gen += 1;                // (the window is baked into a recorded launch like every option)
        if (value != 0 && !t->has_bases) t->has_bases = 1;              // (the kernels read the base column from now on)
        t->auto_window = value;
        return 0;
    case RG_OPT_COMPACT_ANY_CLUSTER:
        if (value != 0 && value != 1) return fail(t, -1, "rg_table_option: RG_OPT_COMPACT_ANY_CLUSTER takes 0 or 1 (%d given)", value);
        if (t->compact_any_cluster != value) t->config_gen += 1;        // (a tick recorded under one setting does not launch under the other)
        t->compact_any_cluster = value;
        return 0;
    case RG_OPT_DEVICE_IN_FLIGHT: {
        if (value != 0 && value != 1) return fail(t, -1, "rg_table_option: RG_OPT_DEVICE_IN_FLIGHT takes 0 or 1 (%d given)", value);
        if ((t->in_flight != nullptr) == (value == 1)) return 0;
        if (bind(t)) return -2;
        HIP_TRY(t, hipStreamSynchronize(t->stream));
        if (value == 1) {
            const size_t bytes = (size_t)t->G * t->F * sizeof(uint16_t);
            uint16_t *c = nullptr;
            HIP_TRY(t, hipMalloc((void **)&c, bytes));
            if (hipError_t e = hipMemsetAsync(c, 0, bytes, t->stream); e != hipSuccess || (e = hipStreamSynchronize(t->stream)) != hipSuccess) {
                (void)hipFree(c);
                return fail(t, -2, "rg_table_option: RG_OPT_DEVICE_IN_FLIGHT: %s", hipGetErrorString(e));
            }
            t->in_flight = c;
        } else {
            HIP_TRY(t, hipFree(t->in_flight));
            t->in_flight = nullptr;
        }
        t->config_gen += 1;                                             // (a recorded tick has the column, or its absence, baked in)
        return 0;
    }
    default: return fail(t, -1, "rg_table_option: unknown option %d", option);
    }
}

static void assembler_release(struct rg_assembler *a);

int rg_table_destroy(rg_table_t *t)
{
    if (!t) return 0;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    // recordings that outlive their table keep no pointer into it: their launch / wait fail with -1, their destroy only frees the handle
    for (rg_tick *k : t->ticks) k->release();
    for (rg_tick2 *k : t->ticks2) k->release();
    for (struct rg_assembler *a : t->assemblers) assembler_release(a);
    t->ticks.clear(); t->ticks2.clear(); t->assemblers.clear();
    void *cols[] = {t->dt.term_commit, t->dt.epoch, t->dt.window, t->dt.ident, t->dt.elect, t->dt.runs, t->dt.peer_en, t->dt.peer_m, t->dt.ibase, t->wide_bodies,
                    t->counters, t->timer_deadline, t->timer_epoch, t->tick_masks, t->tick_ticket, t->timer_counts, t->health_ok, t->health_fail, t->health_recent,
                    t->in_flight};
    for (void *c : cols) if (c) (void)hipFree(c);
    release(t->st.col, C_COLUMNS);
    release(t->aux, X_COLUMNS);
    release(t->scan, S_COLUMNS);
    release(t->fx, E_COLUMNS);
    for (PipeSlot &sl : t->pipe) {
        if (sl.down) (void)hipEventSynchronize(sl.down);
        release(sl.c.col, C_COLUMNS);
        for (hipEvent_t ev : {sl.up, sl.done, sl.down}) if (ev) (void)hipEventDestroy(ev);
    }
    if (t->s_in) (void)hipStreamDestroy(t->s_in);
    if (t->s_out) (void)hipStreamDestroy(t->s_out);
    for (auto &e : t->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (t->region0) { (void)hipEventDestroy(t->region0); (void)hipEventDestroy(t->region1); }
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
    return 0;
}

int rg_table_create(int device, uint32_t groups, uint32_t cluster, uint32_t self_slot, int pre_vote, rg_table_t **out)
{
    if (!out) return fail(nullptr, -1, "rg_table_create: out is NULL");
    *out = nullptr;
    if (groups == 0) return fail(nullptr, -1, "rg_table_create: groups must be > 0");
    if (cluster < RG_MIN_CLUSTER || cluster > RG_MAX_CLUSTER)
        return fail(nullptr, -1, "rg_table_create: cluster size %u outside [%d, %d]", cluster, RG_MIN_CLUSTER, RG_MAX_CLUSTER);
    if (self_slot >= cluster) return fail(nullptr, -1, "rg_table_create: self_slot %u >= cluster %u", self_slot, cluster);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, -2, "rg_table_create: no HIP device (%s) — libraftgpu has no CPU path", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, -1, "rg_table_create: device %d of %d", device, ndev);

    rg_table *t = new rg_table();
    t->device = device; t->G = groups; t->P = cluster; t->self = self_slot; t->F = cluster - 1;
    t->pre_vote = pre_vote != 0;
#define CREATE_TRY(expr)                                                                   \
    do {                                                                                   \
        hipError_t e2_ = (expr);                                                           \
        if (e2_ != hipSuccess) {                                                           \
            fail(nullptr, -2, "%s failed: %s", #expr, hipGetErrorString(e2_));             \
            rg_table_destroy(t);                                                           \
            return -2;                                                                     \
        }                                                                                  \
    } while (0)
    CREATE_TRY(hipSetDevice(device));
    CREATE_TRY(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    const size_t G = groups, F = t->F;
    CREATE_TRY(hipMalloc((void **)&t->dt.term_commit, G * sizeof(I64x2)));
    CREATE_TRY(hipMalloc((void **)&t->dt.epoch, G * sizeof(I64x2)));
    CREATE_TRY(hipMalloc((void **)&t->dt.window, G * sizeof(I64x2)));
    CREATE_TRY(hipMalloc((void **)&t->dt.ident, G * sizeof(rg::Ident)));
    CREATE_TRY(hipMalloc((void **)&t->dt.elect, G * sizeof(rg::Elect)));
    CREATE_TRY(hipMalloc((void **)&t->dt.runs, G * rg::K * sizeof(I64x2)));
    CREATE_TRY(hipMalloc((void **)&t->dt.peer_en, G * F * sizeof(I64x2)));
    CREATE_TRY(hipMalloc((void **)&t->dt.peer_m, G * F * sizeof(rg::Match)));
    CREATE_TRY(hipMalloc((void **)&t->dt.ibase, G * sizeof(int64_t)));
    CREATE_TRY(hipMalloc((void **)&t->wide_bodies, sizeof(unsigned long long)));
    CREATE_TRY(hipMemsetAsync(t->wide_bodies, 0, sizeof(unsigned long long), t->stream));
    {
        hipDeviceProp_t prop;
        CREATE_TRY(hipGetDeviceProperties(&prop, device));
        t->simds = (uint32_t)prop.multiProcessorCount * 4u;
    }
    t->lanes = -1;
    if (const char *e = getenv("RG_SPLIT")) t->lanes = atoi(e) != 0 ? 0 : 64;   // force either kernel
    if (const char *e = getenv("RG_FAST")) t->fast_paths = atoi(e) != 0;
    if (const char *e = getenv("RG_FORCE_WIDE")) t->force_wide = atoi(e) != 0;
    t->counter_slots = (G + 63) / 64 + 1;       // one slot per workgroup of a dense launch
    CREATE_TRY(hipMalloc((void **)&t->counters, t->counter_slots * RG_NUM_COUNTERS * sizeof(unsigned long long)));
    t->dt.groups = groups;
    CREATE_TRY(hipMalloc((void **)&t->timer_deadline, G * sizeof(int64_t)));
    // timers_count_kernel runs whole 256-lane workgroups: every one of their wavefronts stores a count, also those past the
    // last group, so the array covers the grid (found by the host emulation: ceil(G/64) + 1 entries were 2 short at G = 300)
    CREATE_TRY(hipMalloc((void **)&t->timer_counts, ((G + 255) / 256 * 4 + 1) * sizeof(uint32_t)));
    CREATE_TRY(hipMemsetAsync(t->timer_deadline, 0, G * sizeof(int64_t), t->stream));
    CREATE_TRY(hipMalloc((void **)&t->tick_masks, ((G + 255) / 256 * 4) * sizeof(unsigned long long)));
    CREATE_TRY(hipMemsetAsync(t->tick_masks, 0, ((G + 255) / 256 * 4) * sizeof(unsigned long long), t->stream));      // (status words of the expiry's look-back: state 0 = none)
    CREATE_TRY(hipMalloc((void **)&t->tick_ticket, sizeof(uint32_t)));
    CREATE_TRY(hipMemsetAsync(t->tick_ticket, 0, sizeof(uint32_t), t->stream));
    CREATE_TRY(hipMalloc((void **)&t->timer_epoch, G * sizeof(uint32_t)));
    CREATE_TRY(hipMemsetAsync(t->timer_epoch, 0, G * sizeof(uint32_t), t->stream));
    CREATE_TRY(hipMalloc((void **)&t->health_ok, G * F * sizeof(int64_t)));
    CREATE_TRY(hipMalloc((void **)&t->health_fail, G * F * sizeof(int64_t)));
    CREATE_TRY(hipMalloc((void **)&t->health_recent, G * F * sizeof(int32_t)));
    CREATE_TRY(hipMemsetAsync(t->health_ok, 0, G * F * sizeof(int64_t), t->stream));
    CREATE_TRY(hipMemsetAsync(t->health_fail, 0, G * F * sizeof(int64_t), t->stream));
    CREATE_TRY(hipMemsetAsync(t->health_recent, 0, G * F * sizeof(int32_t), t->stream));
    CREATE_TRY(hipMemsetAsync(t->dt.term_commit, 0, G * sizeof(I64x2), t->stream));
    CREATE_TRY(hipMemsetAsync(t->dt.epoch, 0, G * sizeof(I64x2), t->stream));
    CREATE_TRY(hipMemsetAsync(t->dt.window, 0, G * sizeof(I64x2), t->stream));
    CREATE_TRY(hipMemsetAsync(t->dt.runs, 0, G * rg::K * sizeof(I64x2), t->stream));
    CREATE_TRY(hipMemsetAsync(t->dt.peer_en, 0, G * F * sizeof(I64x2), t->stream));
    CREATE_TRY(hipMemsetAsync(t->dt.peer_m, 0, G * F * sizeof(rg::Match), t->stream));
    CREATE_TRY(hipMemsetAsync(t->dt.ibase, 0, G * sizeof(int64_t), t->stream));
    CREATE_TRY(hipMemsetAsync(t->counters, 0, t->counter_slots * RG_NUM_COUNTERS * sizeof(unsigned long long), t->stream));
    {   // fresh groups = what RaftContext.initialize leaves: Follower, term 0, no vote, empty log
        std::vector<rg::Ident> id(G, rg::Ident{RG_NO_NODE, RG_NO_NODE, 1u, 0u});
        std::vector<rg::Elect> el(G, rg::Elect{0, 0u, 1});
        CREATE_TRY(hipMemcpyAsync(t->dt.ident, id.data(), G * sizeof(rg::Ident), hipMemcpyHostToDevice, t->stream));
        CREATE_TRY(hipMemcpyAsync(t->dt.elect, el.data(), G * sizeof(rg::Elect), hipMemcpyHostToDevice, t->stream));
        CREATE_TRY(hipStreamSynchronize(t->stream));
    }
#undef CREATE_TRY
    *out = t;
    return 0;
}

/* ---- state ------------------------------------------------------------------------------------ */

// 0 = step_split_kernel, otherwise the raft groups per wavefront of step_kernel
static int step_lanes(const rg_table *t, uint32_t count)
{
    if (t->lanes >= 0) return t->lanes;
    const uint32_t wavefronts = (count + 63u) / 64u;
    return wavefronts <= t->simds ? 0 : 64;
}

extern "C++" {
// The image of n groups as rg_load_state / rg_read_state move it: (5 + K + 2F) columns of n 16-byte elements, in this order. The range calls copy column by column
// between it and the table; the list calls (rg_read_state_list / rg_load_state_list) move it whole, to and from the one a gather / scatter kernel packs (rg_scan.hpp).
struct StateImage {
    std::vector<I64x2> cells;                       // one allocation: column c at c * n
    I64x2 *tc, *ep, *win, *runs, *en;
    rg::Ident *id;
    rg::Elect *el;
    rg::Match *pm;
    StateImage(size_t n, size_t F) : cells((5 + rg::K + 2 * F) * (n ? n : 1))
    {
        static_assert(sizeof(rg::Ident) == 16 && sizeof(rg::Elect) == 16 && sizeof(rg::Match) == 16, "16-byte columns");
        I64x2 *b = cells.data();
        tc = b; ep = b + n; win = b + 2 * n; id = reinterpret_cast<rg::Ident *>(b + 3 * n); el = reinterpret_cast<rg::Elect *>(b + 4 * n);
        runs = b + 5 * n; en = runs + (size_t)rg::K * n; pm = reinterpret_cast<rg::Match *>(en + F * n);
    }
    size_t bytes() const { return cells.size() * sizeof(I64x2); }
};

// rows 0 .. n - 1 of `s`, validated, into the image; row i is group first + i, or gid[i] (the number the messages name)
static int pack_state(rg_table *t, const char *who, const rg_group_state_t *s, size_t n, uint32_t first, const uint32_t *gid, StateImage &im)
{
    const size_t F = t->F;
    auto group = [&](size_t i) { return gid ? (size_t)gid[i] : first + i; };
    for (size_t i = 0; i < n; i++) {
        const int32_t role = s->role[i];
        if (role < RG_FOLLOWER || role > RG_LEADER) return fail(t, -1, "%s: group %zu role %d", who, group(i), role);
        if (s->voted_for[i] < RG_NO_NODE || s->voted_for[i] >= (int32_t)t->P || s->current_leader[i] < RG_NO_NODE ||
            s->current_leader[i] >= (int32_t)t->P)
            return fail(t, -1, "%s: group %zu node slot out of range", who, group(i));
        const uint32_t total = s->run_count[i], off = s->run_offset[i];
        const uint32_t rc = total > (uint32_t)rg::K ? (uint32_t)rg::K : total;
        int64_t fi = 0, la = 0;
        if (total) {
            fi = s->first_index[i]; la = s->last_index[i];
            if (s->run_start[off] != fi || la < s->run_start[off + total - 1])
                return fail(t, -1, "%s: group %zu runs do not span [first,last]", who, group(i));
            if (fi != s->epoch_index[i] && fi != s->epoch_index[i] + 1)
                return fail(t, -1, "%s: group %zu first index %lld is neither epoch.index nor epoch.index+1",
                            who, group(i), (long long)fi);
            for (uint32_t k = 1; k < total; k++)
                if (s->run_start[off + k] <= s->run_start[off + k - 1] || s->run_term[off + k] == s->run_term[off + k - 1])
                    return fail(t, -1, "%s: group %zu runs are not maximal ascending runs", who, group(i));
        }
        im.tc[i] = I64x2{s->current_term[i], s->commit_index[i]};
        im.ep[i] = I64x2{s->epoch_index[i], s->epoch_term[i]};
        im.win[i] = I64x2{fi, la};
        uint32_t pend = 0;
        for (size_t j = 0; j < F; j++) {
            im.en[j * n + i] = I64x2{s->peer_last_epoch[i * F + j], s->peer_next_index[i * F + j]};
            im.pm[j * n + i] = rg::Match{s->peer_match_index[i * F + j], s->peer_rejection[i * F + j], 0};
            if (s->peer_pending[i * F + j]) pend |= 1u << j;
        }
        for (uint32_t k = 0; k < (uint32_t)rg::K; k++) {
            const bool have = k < rc;
            im.runs[(size_t)k * n + i] = have ? I64x2{s->run_start[off + total - rc + k], s->run_term[off + total - rc + k]} : I64x2{0, 0};
        }
        const uint32_t meta = (uint32_t)role | (s->timeout_detected[i] ? rg::META_TD : 0u) |
                              (s->repl_prepared[i] ? rg::META_PREP : 0u) | (rc << rg::META_RC_SHIFT) |
                              (pend << rg::META_PEND_SHIFT);
        im.id[i] = rg::Ident{s->voted_for[i], s->current_leader[i], s->role_epoch[i], meta};
        im.el[i] = rg::Elect{s->elected_term[i], s->elected_epoch[i], s->votes[i]};
    }
    return 0;
}

// ... and back: the image into rows 0 .. n - 1 of `d`
static void unpack_state(const StateImage &im, size_t n, size_t F, rg_group_state_t *d)
{
    const I64x2 *tc = im.tc, *ep = im.ep, *win = im.win, *runs = im.runs, *en = im.en;
    const rg::Ident *id = im.id;
    const rg::Elect *el = im.el;
    const rg::Match *pm = im.pm;
    for (size_t i = 0; i < n; i++) {
        const uint32_t meta = id[i].meta;
        const uint32_t rc = (meta >> rg::META_RC_SHIFT) & 7u;
        d->current_term[i] = tc[i].x; d->commit_index[i] = tc[i].y;
        d->epoch_index[i] = ep[i].x; d->epoch_term[i] = ep[i].y;
        d->first_index[i] = rc ? win[i].x : 0; d->last_index[i] = rc ? win[i].y : 0;
        d->voted_for[i] = id[i].voted_for; d->current_leader[i] = id[i].leader; d->role_epoch[i] = id[i].role_epoch;
        d->role[i] = (int32_t)(meta & rg::META_ROLE);
        d->timeout_detected[i] = (meta & rg::META_TD) ? 1 : 0;
        d->repl_prepared[i] = (meta & rg::META_PREP) ? 1 : 0;
        d->elected_term[i] = el[i].elected_term; d->elected_epoch[i] = el[i].elected_epoch; d->votes[i] = el[i].votes;
        d->run_count[i] = rc;
        d->run_offset[i] = (uint32_t)(i * rg::K);
        for (uint32_t k = 0; k < (uint32_t)rg::K; k++) {
            d->run_start[i * rg::K + k] = k < rc ? runs[(size_t)k * n + i].x : 0;
            d->run_term[i * rg::K + k] = k < rc ? runs[(size_t)k * n + i].y : 0;
        }
        const uint32_t pend = (meta >> rg::META_PEND_SHIFT) & rg::META_PEND_MASK;
        for (size_t j = 0; j < F; j++) {
            d->peer_last_epoch[i * F + j] = en[j * n + i].x;
            d->peer_next_index[i * F + j] = en[j * n + i].y;
            d->peer_match_index[i * F + j] = pm[j * n + i].match_index;
            d->peer_rejection[i * F + j] = pm[j * n + i].rejection;
            d->peer_pending[i * F + j] = (pend >> j) & 1u;
        }
    }
}

}

static bool state_complete(const rg_group_state_t *s)
{
    return s->current_term && s->voted_for && s->role && s->current_leader && s->timeout_detected && s->repl_prepared &&
           s->role_epoch && s->votes && s->elected_epoch && s->elected_term && s->commit_index && s->epoch_index &&
           s->epoch_term && s->first_index && s->last_index && s->run_count && s->run_offset && s->run_start && s->run_term &&
           s->peer_last_epoch && s->peer_next_index && s->peer_match_index && s->peer_rejection && s->peer_pending;
}

int rg_load_state(rg_table_t *t, uint32_t first, uint32_t count, const rg_group_state_t *s)
{
    if (!t) return -1;
    if (!s || !state_complete(s)) return fail(t, -1, "rg_load_state: src or one of its columns is NULL");
    if ((uint64_t)first + count > t->G) return fail(t, -1, "rg_load_state: range [%u, %u) exceeds %u groups", first, first + count, t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    const size_t n = count, F = t->F, G = t->G;
    StateImage im(n, F);
    if (int rc = pack_state(t, "rg_load_state", s, n, first, nullptr, im)) return rc;
    I64x2 *tc = im.tc, *ep = im.ep, *win = im.win, *runs = im.runs, *en = im.en;
    rg::Ident *id = im.id;
    rg::Elect *el = im.el;
    rg::Match *pm = im.pm;
    hipStream_t st = t->stream;
    HIP_TRY(t, hipMemcpyAsync(t->dt.term_commit + first, tc, n * sizeof(I64x2), hipMemcpyHostToDevice, st));
    HIP_TRY(t, hipMemcpyAsync(t->dt.epoch + first, ep, n * sizeof(I64x2), hipMemcpyHostToDevice, st));
    HIP_TRY(t, hipMemcpyAsync(t->dt.window + first, win, n * sizeof(I64x2), hipMemcpyHostToDevice, st));
    HIP_TRY(t, hipMemcpyAsync(t->dt.ident + first, id, n * sizeof(rg::Ident), hipMemcpyHostToDevice, st));
    HIP_TRY(t, hipMemcpyAsync(t->dt.elect + first, el, n * sizeof(rg::Elect), hipMemcpyHostToDevice, st));
    for (size_t k = 0; k < (size_t)rg::K; k++)
        HIP_TRY(t, hipMemcpyAsync(t->dt.runs + k * G + first, runs + k * n, n * sizeof(I64x2), hipMemcpyHostToDevice, st));
    for (size_t j = 0; j < F; j++) {
        HIP_TRY(t, hipMemcpyAsync(t->dt.peer_en + j * G + first, en + j * n, n * sizeof(I64x2), hipMemcpyHostToDevice, st));
        HIP_TRY(t, hipMemcpyAsync(t->dt.peer_m + j * G + first, pm + j * n, n * sizeof(rg::Match), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(t, hipMemsetAsync(t->timer_deadline + first, 0, n * sizeof(int64_t), st));   // loaded groups hold no timer ticket yet
    HIP_TRY(t, hipMemcpyAsync(t->timer_epoch + first, s->role_epoch, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    for (size_t j = 0; j < F; j++) {                                                       // ... and fresh health statistics
        HIP_TRY(t, hipMemsetAsync(t->health_ok + j * G + first, 0, n * sizeof(int64_t), st));
        HIP_TRY(t, hipMemsetAsync(t->health_fail + j * G + first, 0, n * sizeof(int64_t), st));
        HIP_TRY(t, hipMemsetAsync(t->health_recent + j * G + first, 0, n * sizeof(int32_t), st));
        if (t->in_flight) HIP_TRY(t, hipMemsetAsync(t->in_flight + j * G + first, 0, n * sizeof(uint16_t), st));   // ... with nothing in flight
    }
    HIP_TRY(t, hipStreamSynchronize(st));
    return 0;
}

int rg_read_state(rg_table_t *t, uint32_t first, uint32_t count, rg_group_state_t *d)
{
    if (!t) return -1;
    if (!d || !state_complete(d)) return fail(t, -1, "rg_read_state: dst or one of its columns is NULL");
    if ((uint64_t)first + count > t->G) return fail(t, -1, "rg_read_state: range exceeds %u groups", t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    const size_t n = count, F = t->F, G = t->G;
    StateImage im(n, F);
    I64x2 *tc = im.tc, *ep = im.ep, *win = im.win, *runs = im.runs, *en = im.en;
    rg::Ident *id = im.id;
    rg::Elect *el = im.el;
    rg::Match *pm = im.pm;
    hipStream_t st = t->stream;
    HIP_TRY(t, hipMemcpyAsync(tc, t->dt.term_commit + first, n * sizeof(I64x2), hipMemcpyDeviceToHost, st));
    HIP_TRY(t, hipMemcpyAsync(ep, t->dt.epoch + first, n * sizeof(I64x2), hipMemcpyDeviceToHost, st));
    HIP_TRY(t, hipMemcpyAsync(win, t->dt.window + first, n * sizeof(I64x2), hipMemcpyDeviceToHost, st));
    HIP_TRY(t, hipMemcpyAsync(id, t->dt.ident + first, n * sizeof(rg::Ident), hipMemcpyDeviceToHost, st));
    HIP_TRY(t, hipMemcpyAsync(el, t->dt.elect + first, n * sizeof(rg::Elect), hipMemcpyDeviceToHost, st));
    for (size_t k = 0; k < (size_t)rg::K; k++)
        HIP_TRY(t, hipMemcpyAsync(runs + k * n, t->dt.runs + k * G + first, n * sizeof(I64x2), hipMemcpyDeviceToHost, st));
    for (size_t j = 0; j < F; j++) {
        HIP_TRY(t, hipMemcpyAsync(en + j * n, t->dt.peer_en + j * G + first, n * sizeof(I64x2), hipMemcpyDeviceToHost, st));
        HIP_TRY(t, hipMemcpyAsync(pm + j * n, t->dt.peer_m + j * G + first, n * sizeof(rg::Match), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(t, hipStreamSynchronize(st));
    unpack_state(im, n, F, d);
    return 0;
}

/* ---- the hot path ----------------------------------------------------------------------------- */

static int launch(rg_table *t, const rg::StepParams &p, bool sparse)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (t->timing) {
        if (t->ev_used == t->ev_pool.size()) {
            if (t->ev_pool.size() >= 4096) {
                if (drain_timing(t)) return -2;
            } else {
                hipEvent_t a, b;
                HIP_TRY(t, hipEventCreate(&a));
                HIP_TRY(t, hipEventCreate(&b));
                t->ev_pool.emplace_back(a, b);
            }
        }
        e0 = t->ev_pool[t->ev_used].first; e1 = t->ev_pool[t->ev_used].second;
        HIP_TRY(t, hipEventRecord(e0, t->stream));
    }
    // Up to one wavefront of groups per SIMD, a lone deciding wavefront leaves half of its SIMD's issue slots empty:
    // give it an I/O partner (step_split_kernel). With more groups the SIMDs are shared by several deciding
    // wavefronts anyway and the single-wavefront kernel is the faster one.
    HIP_TRY(t, rg::launch_step(p, (int)t->F, sparse, p.abcd32 ? 32 : step_lanes(t, p.count), t->stream));
    if (t->timing) {
        HIP_TRY(t, hipEventRecord(e1, t->stream));
        t->ev_used += 1;
    }
    return 0;
}

// the compact formats and the ticks belong to clusters of up to RG_MAX_COMPACT_CLUSTER nodes, or to a table with RG_OPT_COMPACT_ANY_CLUSTER (include/raftgpu.h)
static int compact_ok(rg_table *t, const char *who)
{
    if (t->P > RG_MAX_COMPACT_CLUSTER && !t->compact_any_cluster)
        return fail(t, -1, "%s: a cluster of %u nodes is decided on wide rows (rg_submit, rg_submit_async); the compact formats end at %d nodes unless the table has "
                           "RG_OPT_COMPACT_ANY_CLUSTER (rg_table_option), which lifts the limit", who, t->P, RG_MAX_COMPACT_CLUSTER);
    return 0;
}

// a list of groups in host memory names groups of the table, strictly ascending -> 0, or the rule the first offending row breaks: 1 = out of range,
// 2 = not ascending; *row is that row. (Each entry point words the refusal itself.)
static int bad_gid_list(const uint32_t *gid, uint32_t count, uint32_t groups, uint32_t *row)
{
    for (uint32_t i = 0; i < count; i++) {
        const int why = gid[i] >= groups ? 1 : (i && gid[i] <= gid[i - 1]) ? 2 : 0;
        if (why) { *row = i; return why; }
    }
    return 0;
}

// the same shape rules for every submission (rounds, count, gid list, entry bound); the refusals say rg_submit whichever entry point was called
// list_rounds: the caller takes a list of groups with any number of rounds (rg_submit32c_sparse_rounds, rg_tick2_create_sparse_rounds)
static int check_shape(rg_table *t, const Shape &in, bool host_memory, bool list_rounds = false)
{
    if (in.rounds == 0) return fail(t, -1, "rg_submit: rounds must be >= 1");
    const bool sparse = in.gid != nullptr;
    if (sparse) {
        if (in.rounds != 1 && !list_rounds) return fail(t, -1, "rg_submit: sparse batches carry exactly one round");
        if (in.count > t->G) return fail(t, -1, "rg_submit: %u rows for %u groups", in.count, t->G);
    } else if (in.count != t->G) {
        return fail(t, -1, "rg_submit: dense batch has %u rows per round, table has %u groups", in.count, t->G);
    }
    if (in.entry_count && !in.entry_terms) return fail(t, -1, "rg_submit: entry_count without entry_terms");
    if (in.entry_count > (1ull << 29)) return fail(t, -1, "rg_submit: at most 2^29 entry terms per batch (%llu given)", (unsigned long long)in.entry_count);
    uint32_t i = 0;
    if (sparse && host_memory)
        if (const int why = bad_gid_list(in.gid, in.count, t->G, &i))
            return why == 1 ? fail(t, -1, "rg_submit: gid[%u]=%u out of range", i, in.gid[i]) : fail(t, -1, "rg_submit: gid must be strictly ascending (row %u)", i);
    return 0;
}

static int check_batch(rg_table *t, const rg_batch_t *in, const rg_outcome_t *out, bool host_memory)
{
    if (!in || !out) return fail(t, -1, "rg_submit: NULL batch or outcome");
    if (!in->head || !in->ab || !in->cd || !out->reply || !out->logfx || !out->persist)
        return fail(t, -1, "rg_submit: head/ab/cd/reply/logfx/persist are required");
    return check_shape(t, shape_of(in), host_memory);
}

static rg::StepParams step_params(rg_table *t, const Shape &in)
{
    rg::StepParams p{};
    p.t = t->dt;
    p.rounds = in.rounds; p.count = in.count; p.stride = in.count;
    p.entry_count = in.entry_count;
    p.counters = t->counters;
    p.wide_bodies = t->wide_bodies;
    p.self = (int32_t)t->self; p.cluster = (int32_t)t->P; p.majority = (int32_t)(t->P / 2 + 1); p.pre_vote = t->pre_vote;
    p.fast_paths = t->fast_paths;
    p.force_wide = t->force_wide;
    p.require_fence = t->require_fence;
    p.has_bases = t->has_bases;
    p.auto_window = t->auto_window;
    return p;
}

// A batch in host memory onto the device, on stream s, into the columns c of its owner (the table, a pipeline slot): the inputs are staged and p reads them.
// The wide rows: head / ab / cd, the gid list of a list of groups, the hint column and the entry terms where the batch has them ...
static int upload_wide(rg_table *t, BatchCols &c, const rg_batch_t *in, hipStream_t s, rg::StepParams &p)
{
    const size_t rows = (size_t)in->rounds * in->count;
    if (stage_in(t, c[C_HEAD], in->head, rows, s, &p.head) || stage_in(t, c[C_AB], in->ab, rows, s, &p.ab) || stage_in(t, c[C_CD], in->cd, rows, s, &p.cd)) return -2;
    if (in->gid && stage_in(t, c[C_GID], in->gid, in->count, s, &p.gid)) return -2;
    if (in->hint && stage_in(t, c[C_HINT], in->hint, rows, s, &p.hint)) return -2;
    if (in->entry_count && stage_in(t, c[C_TERMS], in->entry_terms, in->entry_count, s, &p.entry_terms)) return -2;
    return 0;
}

// ... and the compact rows: head / abcd, the gid list, the 32-bit entry terms. The compact-format kernel reads the rows as they arrived: no widening pass
static int upload_compact(rg_table *t, BatchCols &c, const rg_batch32_t *in, hipStream_t s, rg::StepParams &p)
{
    const size_t rows = (size_t)in->rounds * in->count;
    if (stage_in(t, c[C_HEAD], in->head, rows, s, &p.head) || stage_in(t, c[C_ABCD32], in->abcd, rows, s, &p.abcd32)) return -2;
    if (in->gid && stage_in(t, c[C_GID], in->gid, in->count, s, &p.gid)) return -2;
    if (in->entry_count && stage_in(t, c[C_TERMS32], in->entry_terms, in->entry_count, s, &p.entry_terms32)) return -2;
    return 0;
}

// the wide outcome columns of `rows` rows for p to write ...
static int outcome_wide(rg_table *t, BatchCols &c, size_t rows, rg::StepParams &p)
{
    return stage_out(t, c[C_REPLY], rows, &p.reply) || stage_out(t, c[C_LOGFX], rows, &p.logfx) || stage_out(t, c[C_PERSIST], rows, &p.persist) ? -2 : 0;
}

// ... and back into the caller's reply / logfx / persist, on stream s
static int download_wide(rg_table *t, BatchCols &c, const rg_outcome_t &out, size_t rows, hipStream_t s)
{
    return stage_back(t, c[C_REPLY], out.reply, rows, s) || stage_back(t, c[C_LOGFX], out.logfx, rows, s) || stage_back(t, c[C_PERSIST], out.persist, rows, s) ? -2 : 0;
}

static int pipeline_ready(rg_table *t);

/* the pipelined host-memory path: see include/raftgpu.h */
int rg_submit_async(rg_table_t *t, const rg_batch_t *in, const rg_outcome_t *out)
{
    if (!t) return -1;
    if (int rc = check_batch(t, in, out, true)) return rc;
    if (in->count == 0) return 0;
    if (bind(t, false)) return -2;
    if (int rc = pipeline_ready(t)) return rc;
    PipeSlot &sl = t->pipe[t->pipe_head % RG_PIPELINE_DEPTH];
    const bool sparse = in->gid != nullptr;
    const size_t rows = (size_t)in->rounds * in->count;
    rg::StepParams p = step_params(t, shape_of(in));
    hipStream_t si = t->s_in, so = t->s_out;
    if (int rc = outcome_wide(t, sl.c, rows, p)) return rc;
    if (int rc = upload_wide(t, sl.c, in, si, p)) return rc;
    HIP_TRY(t, hipEventRecord(sl.up, si));
    HIP_TRY(t, hipStreamWaitEvent(t->stream, sl.up, 0));                  // the kernel of this batch needs its upload ...
    if (int rc = launch(t, p, sparse)) return rc;                          // ... and, being on the table's stream, runs after the batch before it
    HIP_TRY(t, hipEventRecord(sl.done, t->stream));
    HIP_TRY(t, hipStreamWaitEvent(so, sl.done, 0));
    if (int rc = download_wide(t, sl.c, *out, rows, so)) return rc;
    HIP_TRY(t, hipEventRecord(sl.down, so));
    t->pipe_head += 1;
    return 0;
}

static int pipeline_ready(rg_table *t)
{
    if (!t->s_in) {
        HIP_TRY(t, hipStreamCreateWithFlags(&t->s_in, hipStreamNonBlocking));
        HIP_TRY(t, hipStreamCreateWithFlags(&t->s_out, hipStreamNonBlocking));
        for (PipeSlot &sl : t->pipe) {
            HIP_TRY(t, hipEventCreate(&sl.up)); HIP_TRY(t, hipEventCreate(&sl.done)); HIP_TRY(t, hipEventCreate(&sl.down));
        }
    }
    if (t->pipe_head - t->pipe_tail == RG_PIPELINE_DEPTH)
        if (int rc = wait_oldest(t); rc < 0) return rc;
    return 0;
}

/* the pipelined host-memory path with compact transfer formats: see include/raftgpu.h */
int rg_submit_async_packed(rg_table_t *t, const rg_batch32_t *in, const rg_outcome_packed_t *out)
{
    if (!t) return -1;
    if (int rc = compact_ok(t, "rg_submit_async_packed")) return rc;
    if (!in || !out) return fail(t, -1, "rg_submit_async_packed: null batch or outcome");
    if (!in->head || !in->abcd || !out->reply || !out->counts || (out->logfx_cap && !out->logfx) || (out->persist_cap && !out->persist))
        return fail(t, -1, "rg_submit_async_packed: head, abcd, reply, counts and every list with a capacity are required");
    if (in->entry_count && !in->entry_terms) return fail(t, -1, "rg_submit_async_packed: entry_count %llu without entry_terms", (unsigned long long)in->entry_count);
    if (int rc = check_shape(t, shape_of(in), true)) return rc;
    if (in->count == 0) { out->counts[0] = out->counts[1] = 0; return 0; }
    const size_t rows64 = (size_t)in->rounds * in->count;
    if (rows64 >= (1ull << 31)) return fail(t, -1, "rg_submit_async_packed: %zu rows in one batch (limit 2^31 - 1)", rows64);
    if (bind(t, false)) return -2;
    // the lists are written by the device into the caller's memory: it has to be page-locked and mapped
    void *d_logfx = nullptr, *d_persist = nullptr, *d_counts = nullptr;
    if (hipHostGetDevicePointer(&d_counts, out->counts, 0) != hipSuccess ||
        (out->logfx_cap && hipHostGetDevicePointer(&d_logfx, out->logfx, 0) != hipSuccess) ||
        (out->persist_cap && hipHostGetDevicePointer(&d_persist, out->persist, 0) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(t, -1, "rg_submit_async_packed: counts / logfx / persist must be page-locked memory from rg_host_alloc");
    }
    if (int rc = pipeline_ready(t)) return rc;
    PipeSlot &sl = t->pipe[t->pipe_head % RG_PIPELINE_DEPTH];
    const bool sparse = in->gid != nullptr;
    const uint32_t rows = (uint32_t)rows64, waves = (rows + 63u) / 64u;
    rg::StepParams p = step_params(t, shape_of(in));
    uint32_t *wave_counts = nullptr;
    hipStream_t si = t->s_in, so = t->s_out;
    if (int rc = outcome_wide(t, sl.c, rows64, p)) return rc;
    if (stage_out(t, sl.c[C_COUNTS], (size_t)2 * waves, &wave_counts)) return -2;
    if (int rc = upload_compact(t, sl.c, in, si, p)) return rc;
    HIP_TRY(t, hipEventRecord(sl.up, si));
    HIP_TRY(t, hipStreamWaitEvent(t->stream, sl.up, 0));
    if (int rc = launch(t, p, sparse)) return rc;
    HIP_TRY(t, rg::launch_outcome_count(p.reply, rows, wave_counts, (uint32_t *)d_counts, t->stream));
    HIP_TRY(t, hipEventRecord(sl.done, t->stream));
    HIP_TRY(t, hipStreamWaitEvent(so, sl.done, 0));
    // the scatter is link-bound (it writes host memory): on the copy-out stream, so the next batch's kernels do not queue behind it
    HIP_TRY(t, rg::launch_outcome_emit(p.reply, p.logfx, p.persist, rows, wave_counts, (I64x2 *)d_logfx, out->logfx_cap, (rg_persist_t *)d_persist, out->persist_cap, so));
    if (int rc = stage_back(t, sl.c[C_REPLY], out->reply, rows64, so)) return rc;
    HIP_TRY(t, hipEventRecord(sl.down, so));
    t->pipe_head += 1;
    return 0;
}

/* the once-per-tick path: see include/raftgpu.h */
int rg_tick_destroy(rg_tick_t *k) { return recording_destroy(k, &rg_table::ticks); }

// a buffer a recorded copy replays from / into must be page-locked: a pageable one is either rejected late by the capture with an opaque error, or
// captured with undefined semantics
static bool page_locked(const void *p)
{
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void *>(p), 0) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

int rg_tick_create(rg_table_t *t, const rg_batch32_t *in, const rg_outcome_packed_t *out, rg_tick_t **tick)
{
    if (!t) return -1;
    if (int rc = compact_ok(t, "rg_tick_create")) return rc;
    if (!tick) return fail(t, -1, "rg_tick_create: tick is NULL");
    *tick = nullptr;
    if (!in || !out) return fail(t, -1, "rg_tick_create: null batch or outcome");
    if (!in->head || !in->abcd || !out->reply || !out->counts || (out->logfx_cap && !out->logfx) || (out->persist_cap && !out->persist))
        return fail(t, -1, "rg_tick_create: head, abcd, reply, counts and every list with a capacity are required");
    if (in->entry_count && !in->entry_terms) return fail(t, -1, "rg_tick_create: entry_count %llu without entry_terms", (unsigned long long)in->entry_count);
    if (in->gid) {                                          // (a sparse gid list is read at every launch, not now: only the round and row counts are checked here)
        if (in->rounds != 1) return fail(t, -1, "rg_tick_create: sparse batches carry exactly one round");
        if (in->count > t->G || in->count == 0) return fail(t, -1, "rg_tick_create: %u rows for %u groups", in->count, t->G);
    } else if (int rc = check_shape(t, shape_of(in), true)) return rc;
    if (in->rounds == 0 || in->count == 0) return fail(t, -1, "rg_tick_create: an empty shape");
    const size_t rows64 = (size_t)in->rounds * in->count;
    if (rows64 >= (1ull << 31)) return fail(t, -1, "rg_tick_create: %zu rows in one batch (limit 2^31 - 1)", rows64);
    if (bind(t)) return -2;
    void *d_logfx = nullptr, *d_persist = nullptr, *d_counts = nullptr;
    if (hipHostGetDevicePointer(&d_counts, out->counts, 0) != hipSuccess ||
        (out->logfx_cap && hipHostGetDevicePointer(&d_logfx, out->logfx, 0) != hipSuccess) ||
        (out->persist_cap && hipHostGetDevicePointer(&d_persist, out->persist, 0) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(t, -1, "rg_tick_create: counts / logfx / persist must be page-locked memory from rg_host_alloc");
    }
    if (!page_locked(in->head) || !page_locked(in->abcd) || !page_locked(out->reply) || (in->gid && !page_locked(in->gid)) ||
        (in->entry_count && !page_locked(in->entry_terms)))
        return fail(t, -1, "rg_tick_create: head / abcd / gid / entry_terms / reply must be page-locked memory from rg_host_alloc (the recorded copies replay from them)");
    rg_tick *k = new rg_tick();
    k->t = t;
    k->config_gen = t->config_gen;
    const uint32_t rows = (uint32_t)rows64, waves = (rows + 63u) / 64u;
    const bool sparse = in->gid != nullptr;
    rg::StepParams p = step_params(t, shape_of(in));
    BatchCols &c = k->c;
    uint32_t *wave_counts = nullptr;
    if (outcome_wide(t, c, rows64, p) || stage_out(t, c[C_COUNTS], (size_t)2 * waves, &wave_counts) || stage_out(t, c[C_HEAD], rows64, &p.head) ||
        stage_out(t, c[C_ABCD32], rows64, &p.abcd32) || (sparse && stage_out(t, c[C_GID], in->count, &p.gid)) ||
        (in->entry_count && stage_out(t, c[C_TERMS32], in->entry_count, &p.entry_terms32))) {
        rg_tick_destroy(k);
        return -2;
    }
    // the copies are recorded: the chain keeps going to the end of the capture whatever fails, and carries the first error there
    hipStream_t s = t->stream;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) e = col_up(c[C_HEAD], in->head, 0, rows64, s);
    if (e == hipSuccess) e = col_up(c[C_ABCD32], in->abcd, 0, rows64, s);
    if (e == hipSuccess && sparse) e = col_up(c[C_GID], in->gid, 0, in->count, s);
    if (e == hipSuccess) e = col_up(c[C_TERMS32], in->entry_terms, 0, in->entry_count, s);
    if (e == hipSuccess) e = rg::launch_step(p, (int)t->F, sparse, 32, s);
    if (e == hipSuccess) e = rg::launch_outcome_count(p.reply, rows, wave_counts, (uint32_t *)d_counts, s);
    if (e == hipSuccess) e = rg::launch_outcome_emit(p.reply, p.logfx, p.persist, rows, wave_counts, (I64x2 *)d_logfx, out->logfx_cap, (rg_persist_t *)d_persist, out->persist_cap, s);
    if (e == hipSuccess) e = col_down(c[C_REPLY], out->reply, 0, rows64, s);
    if ((e = recording_finish(k, e)) != hipSuccess) {
        rg_tick_destroy(k);
        return fail(t, -2, "rg_tick_create: %s", hipGetErrorString(e));
    }
    t->ticks.push_back(k);
    *tick = k;
    return 0;
}

int rg_tick_launch(rg_tick_t *k)
{
    if (int rc = recording_bind(k, "rg_tick_launch", "rg_tick_create")) return rc;
    rg_table *t = k->t;
    if (k->in_flight) { HIP_TRY(t, hipStreamSynchronize(t->stream)); k->in_flight = false; }
    HIP_TRY(t, hipGraphLaunch(k->exec, t->stream));
    k->in_flight = true;
    return 0;
}

int rg_tick_wait(rg_tick_t *k) { return recording_wait(k); }

static rg::TimerParams timer_params(rg_table *t);
static rg::HealthParams health_params(rg_table *t);

/* the device-resident tick: see include/raftgpu.h */
int rg_tick2_destroy(rg_tick2_t *k) { return recording_destroy(k, &rg_table::ticks2); }

// the device's address of memory the caller says is device-visible: page-locked host memory is mapped, device memory is what it is; pageable host
// memory (which a kernel would fault on) is refused where the runtime can tell
static int device_visible(rg_table *t, const char *who, const void *p, const char *what, void **out)
{
    *out = nullptr;
    if (!p) return 0;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type == hipMemoryTypeUnregistered) {
        (void)hipGetLastError();
        return fail(t, -1, "%s: %s is neither device memory (rg_dev_alloc) nor page-locked host memory (rg_host_alloc)", who, what);
    }
    if (a.type == hipMemoryTypeHost) {
        if (hipHostGetDevicePointer(out, const_cast<void *>(p), 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(t, -1, "%s: %s is host memory the device cannot address", who, what);
        }
        return 0;
    }
    *out = const_cast<void *>(p);
    return 0;
}

// rows == nullptr: the dense tick (rg_tick2_create: every group has a row); else the sparse one (rg_tick2_create_sparse: row i belongs to group rows->gid[i], the
// rows of a run are counted by *rows->count, the per-row columns are sized for rows->capacity). deep: the sparse tick of rg_tick2_create_sparse_rounds — io->rounds is
// the greatest depth, every [round][row] column is laid out [io->rounds][capacity], and the depth of a run is read from *depth_now (nullptr: always io->rounds)
static int tick2_create(rg_table_t *t, const rg_tick2_io_t *io, const rg_tick2_rows_t *rows, rg_tick2_t **tick, const char *who, bool deep = false,
                        const uint32_t *depth_now = nullptr)
{
    if (!t) return -1;
    if (int rc = compact_ok(t, who)) return rc;
    if (!tick) return fail(t, -1, "%s: tick is NULL", who);
    *tick = nullptr;
    if (!io) return fail(t, -1, "%s: io is NULL", who);
    if (io->rounds == 0 || io->rounds > 64) return fail(t, -1, "%s: %u rounds (1 .. 64: one clock per round travels with the tick)", who, io->rounds);
    if (!io->head || !io->abcd || !io->now || !io->row || !io->persist32) return fail(t, -1, "%s: head, abcd, now, row and persist32 are required", who);
    if (io->entry_capacity && !io->entry_terms) return fail(t, -1, "%s: entry_capacity %llu without entry_terms", who, (unsigned long long)io->entry_capacity);
    if (io->expired_gid && (!io->expired_count || io->expired_capacity == 0)) return fail(t, -1, "%s: the expiry step needs expired_count and a capacity", who);
    if ((io->send_head == nullptr) != (io->send == nullptr)) return fail(t, -1, "%s: send_head and send come together", who);
    if (t->in_flight && (io->heartbeat || io->in_flight))
        return fail(t, -1, "%s: the table has RG_OPT_DEVICE_IN_FLIGHT: the send step derives heartbeat and in_flight from the tick's own rows, both columns must be NULL", who);
    if (rows) {
        if (io->rounds != 1 && !deep) return fail(t, -1, "%s: %u rounds (a list of groups carries exactly one round)", who, io->rounds);
        if (!rows->gid || !rows->count) return fail(t, -1, "%s: gid and count are required", who);
        if (rows->capacity == 0 || rows->capacity > t->G) return fail(t, -1, "%s: a capacity of %u rows for %u groups (1 .. groups)", who, rows->capacity, t->G);
    }
    const uint32_t R = rows ? rows->capacity : t->G;        // rows the per-row columns are sized for
    const Shape shape{io->rounds, R, rows ? rows->gid : nullptr, io->entry_capacity, io->entry_terms != nullptr};
    if (int rc = check_shape(t, shape, false, deep)) return rc;
    if (bind(t)) return -2;
    const auto visible = [t](const void *p, const char *what, void **out) { return device_visible(t, "rg_tick2_create", p, what, out); };      // (whichever constructor: the refusals have always said rg_tick2_create)
    void *d_head, *d_abcd, *d_terms, *d_now, *d_hb, *d_fl, *d_row, *d_per, *d_egid, *d_eep, *d_ecnt, *d_sh, *d_ss, *d_ready, *d_gid = nullptr, *d_cnt = nullptr, *d_depth = nullptr;
    if ((rows && (visible(rows->gid, "gid", &d_gid) || visible(rows->count, "count", &d_cnt) || visible(depth_now, "rounds", &d_depth))) ||
        visible(io->head, "head", &d_head) || visible(io->abcd, "abcd", &d_abcd) || visible(io->entry_terms, "entry_terms", &d_terms) ||
        visible(io->now, "now", &d_now) || visible(io->heartbeat, "heartbeat", &d_hb) || visible(io->in_flight, "in_flight", &d_fl) ||
        visible(io->row, "row", &d_row) || visible(io->persist32, "persist32", &d_per) || visible(io->expired_gid, "expired_gid", &d_egid) ||
        visible(io->expired_epoch, "expired_epoch", &d_eep) || visible(io->expired_count, "expired_count", &d_ecnt) ||
        visible(io->send_head, "send_head", &d_sh) || visible(io->send, "send", &d_ss) || visible(io->ready, "ready", &d_ready))
        return -1;
    rg_tick2 *k = new rg_tick2();
    k->t = t;
    k->config_gen = t->config_gen;
    // the decisions: rg_submit32c / rg_submit32c_sparse on device-visible rows
    rg::StepParams sp = step_params(t, shape);
    sp.gid = (const uint32_t *)d_gid;
    sp.head = (const rg_ev_head_t *)d_head; sp.abcd32 = (const rg::I32x4 *)d_abcd;
    sp.entry_terms32 = io->entry_capacity ? (const int32_t *)d_terms : nullptr;
    sp.out32 = (rg::I32x4 *)d_row; sp.persist32 = (rg::I32x4 *)d_per;
    // what the batch did to the timers and to the followers' health, from the compact rows where they lie
    rg::TimerParams tp = timer_params(t);
    tp.rounds = io->rounds; tp.count = R; tp.out32 = (const rg::I32x4 *)d_row; tp.persist32 = (const rg::I32x4 *)d_per; tp.now_mem = (const int64_t *)d_now;
    rg::HealthParams hp = health_params(t);
    hp.rounds = io->rounds; hp.count = R; hp.head = (const rg_ev_head_t *)d_head; hp.out32 = (const rg::I32x4 *)d_row; hp.now_mem = (const int64_t *)d_now;
    const int64_t *now_last = (const int64_t *)d_now + (io->rounds - 1);
    rg::HealthParams rp = health_params(t);
    rp.now_mem = now_last;
    rg::ReplicateParams qp{};
    qp.t = t->dt; qp.count = R; qp.gid = (const uint32_t *)d_gid; qp.heartbeat = (const uint8_t *)d_hb; qp.in_flight = (const uint16_t *)d_fl; qp.head = (rg_send_head_t *)d_sh; qp.send = (rg_send_t *)d_ss;
    if (t->in_flight) {                                      // RG_OPT_DEVICE_IN_FLIGHT: the send step reads the tick's own rows and the table's counts (rg_kernels.hip, replicate_wave)
        qp.counts = t->in_flight; qp.ev_head = (const rg_ev_head_t *)d_head; qp.ev_out32 = (const rg::I32x4 *)d_row; qp.ev_stride = R; qp.self = t->self;
    }
    hipStream_t s = t->stream;
    // What follows the decisions — what the batch did to the timers and to the followers' health, the list of the tickets that fired, the leaders' sends, the
    // readiness column — is one lane per group with same-group dependencies only, and a single-round tick is launch-bound (~14 us per graph node for ~10 us of
    // work in all at 65 536 groups). So the recording is ONE kernel node: rg_kernels.hip, tick_kernel — the workgroup that decided 64 groups does the rest for
    // them. RG_TICK_NODES=2 records step + tick_tail_kernel, RG_TICK_NODES=4 the step-by-step form (step, tick_fold, replicate, ready): same-box A/Bs and the
    // differential tests. timer_counts doubles as the per-wavefront masks of the expiry (64 bits each) + its ticket word.
    rg::TickFoldParams fp{};
    fp.tp = tp; fp.hp = hp; fp.now_last = now_last;
    fp.masks = (unsigned long long *)t->tick_masks; fp.ticket = t->tick_ticket;
    fp.out_gid = (uint32_t *)d_egid; fp.out_epoch = (uint32_t *)d_eep; fp.out_count = (uint32_t *)d_ecnt; fp.capacity = io->expired_capacity;
    fp.expire = io->expired_gid != nullptr;
    fp.rounds_now = (const uint32_t *)d_depth;
    rg::TickTailParams tt{};
    tt.fp = fp; tt.qp = qp; tt.rp = rp; tt.critical_point = io->critical_point; tt.cool_down = io->cool_down_ms; tt.ready = (uint8_t *)d_ready;
    const char *nodes_env = getenv("RG_TICK_NODES");
    int nodes = (nodes_env && (nodes_env[0] == '2' || nodes_env[0] == '4')) ? nodes_env[0] - '0' : (sp.force_wide != 0 ? 2 : 1);
    if (nodes == 4 && t->in_flight) nodes = 2;              // (the stand-alone replicate kernel has no rows to walk: include/raftgpu.h)
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (rows) {
        // the sparse tick has ONE recording: the rows' workgroups (rg_kernels.hip, tick_sparse_kernel), then — it covers the whole table, whatever the list — the expiry
        if (e == hipSuccess) e = rg::launch_tick_sparse(sp, tt, (const uint32_t *)d_cnt, (int)t->F, s);
        if (e == hipSuccess && fp.expire) e = rg::launch_tick_expire(fp, s);
    } else if (nodes == 1) {
        if (e == hipSuccess) e = rg::launch_tick(sp, tt, (int)t->F, s);
    } else {
        if (e == hipSuccess) e = rg::launch_step(sp, (int)t->F, false, 32, s);
        if (nodes == 2) {
            if (e == hipSuccess) e = rg::launch_tick_tail(tt, (int)t->F, s);
        } else {
            if (e == hipSuccess) e = rg::launch_tick_fold(fp, s);
            if (e == hipSuccess && io->send_head) e = rg::launch_replicate(qp, (int)t->F, s);
            if (e == hipSuccess && io->ready) e = rg::launch_ready(rp, 0, io->critical_point, io->cool_down_ms, (uint8_t *)d_ready, s);
        }
    }
    if ((e = recording_finish(k, e)) != hipSuccess) {
        rg_tick2_destroy(k);
        return fail(t, -2, "%s: %s", who, hipGetErrorString(e));
    }
    t->ticks2.push_back(k);
    *tick = k;
    return 0;
}

int rg_tick2_create(rg_table_t *t, const rg_tick2_io_t *io, rg_tick2_t **tick)
{
    return tick2_create(t, io, nullptr, tick, "rg_tick2_create");
}

int rg_tick2_create_sparse(rg_table_t *t, const rg_tick2_io_t *io, const rg_tick2_rows_t *rows, rg_tick2_t **tick)
{
    if (t && !rows) return fail(t, -1, "rg_tick2_create_sparse: rows is NULL");
    return tick2_create(t, io, rows, tick, "rg_tick2_create_sparse");
}

int rg_tick2_create_sparse_rounds(rg_table_t *t, const rg_tick2_io_t *io, const rg_tick2_rounds_t *rows, rg_tick2_t **tick)
{
    if (t && !rows) return fail(t, -1, "rg_tick2_create_sparse_rounds: rows is NULL");
    if (!t) return -1;
    const rg_tick2_rows_t list{rows->gid, rows->count, rows->capacity};
    return tick2_create(t, io, &list, tick, "rg_tick2_create_sparse_rounds", true, rows->rounds);
}

int rg_tick2_launch(rg_tick2_t *k)
{
    if (int rc = recording_bind(k, "rg_tick2_launch", "rg_tick2_create")) return rc;
    rg_table *t = k->t;
    HIP_TRY(t, hipGraphLaunch(k->exec, t->stream));             // (a launch behind one in flight is ordered after it on the stream: include/raftgpu.h)
    k->in_flight = true;
    return 0;
}

int rg_tick2_wait(rg_tick2_t *k) { return recording_wait(k); }

/* ---- assembling a batch on the device (rg_assemble32; kernels: rg_assemble.hpp) ------------------------------------------------------ */
struct rg_assembler {
    rg_table *t = nullptr;
    uint32_t max_events = 0, max_expired = 0;
    rg::AsmParams sc{};                             // the scratch pointers and their capacities; the rest is filled per run
    enum { IN_WORDS, IN_GID, IN_HEAD, IN_ABCD, EX_GID, EX_EPOCH,                        // RG_MEM_HOST: the sources ...
           OUT_GID, OUT_WORDS, OUT_HEAD, OUT_ABCD, OUT_ORIGIN, OUT_DEFERRED,            // ... and the batch
           ROUTE_PC, ROUTE_AC, ROUTE_SC, AS_COLUMNS };                                  // RG_MEM_DEVICE routes: the scratch of the route's lists
    Staging as[AS_COLUMNS];
    bool ran = false;                               // rg_route32 routes the last run: its shape
    uint32_t last_C = 0, last_D = 0, last_in_cap = 0, last_ex_cap = 0;
    enum { RT_GID, RT_WORDS, RT_ORIGIN, RT_ROW, RT_PERSIST, RT_SEND, RT_CELL, RT_OROW, RT_OPERSIST, RT_XCELL, RT_XROW, RT_XPERSIST, RT_PLIST, RT_ALIST, RT_SLIST, RT_SOFF,
           RT_COUNTS, RT_PC, RT_AC, RT_SC, RT_COLUMNS };
    Staging rt[RT_COLUMNS];                         // RG_MEM_HOST: the columns of rg_decided_t and rg_routed_t, and the lists' count arrays
    // the carry (rg_assembler_carry_enable): two carries in device memory; a run reads carry[runs & 1] and leaves the other: the host's call counter, never device data
    struct Carry { uint32_t *count = nullptr, *gid = nullptr; rg::U32x2 *head = nullptr; rg::I32x4 *abcd = nullptr; };
    uint32_t carry_cap = 0;
    Carry carry[2];
    unsigned runs = 0;
    enum { RC_CELL, RC_ROW, RC_PERSIST, RC_COLUMNS };
    Staging rc[RC_COLUMNS];                         // RG_MEM_HOST: the columns of rg_routed_carry_t
};

// what an assembler holds per event (and per carried slot): freed, then allocated for max_events + max_expired + carry_capacity positions and two carries of
// carry_capacity rows (called with the table's device current and its stream idle; on failure the assembler holds none of them)
static void assembler_release_events(struct rg_assembler *a)
{
    rg::AsmParams &p = a->sc;
    void *cols[] = {p.rowcnt, p.segoff, p.seg, p.flag, p.dcounts, p.big, p.where, a->carry[0].count, a->carry[0].gid, a->carry[0].head, a->carry[0].abcd,
                    a->carry[1].count, a->carry[1].gid, a->carry[1].head, a->carry[1].abcd};
    for (void *c : cols) if (c) (void)hipFree(c);
    p.rowcnt = p.segoff = p.seg = p.dcounts = p.big = p.where = nullptr; p.flag = nullptr;
    a->carry[0] = a->carry[1] = rg_assembler::Carry{};
    a->carry_cap = 0; a->runs = 0; a->ran = false;
}

static int assembler_size_events(struct rg_assembler *a, uint32_t carry_capacity, const char *who)
{
    rg_table *t = a->t;
    assembler_release_events(a);
    rg::AsmParams &p = a->sc;
    const size_t G = t->G, events = (size_t)a->max_events + a->max_expired + carry_capacity, eb = events ? (events + 255) / 256 : 1, K = carry_capacity;
    p.seg_cap = (uint32_t)events;
    p.rows_cap = (uint32_t)(G < events ? G : events);                  // a listed row has an event: there are never more rows than events, or than groups
    p.big_cap = (uint32_t)(events / (rg::ASM_SMALL + 1) + 1);          // ... and a row queued for asm_big_rows_kernel has more than ASM_SMALL of them
    struct { void **ptr; size_t bytes; bool zero; } cols[] = {
        {(void **)&p.rowcnt, ((size_t)p.rows_cap + 1) * sizeof(uint32_t), false}, {(void **)&p.segoff, ((size_t)p.rows_cap + 1) * sizeof(uint32_t), false},
        {(void **)&p.seg, (events + 1) * sizeof(uint32_t), false}, {(void **)&p.flag, events + 1, false}, {(void **)&p.dcounts, (eb * 4 + 1) * sizeof(uint32_t), false},
        {(void **)&p.big, (size_t)p.big_cap * sizeof(uint32_t), false},
        {(void **)&p.where, K ? (events + 1) * sizeof(uint32_t) : 0, false},
        {(void **)&a->carry[0].count, K ? sizeof(uint32_t) : 0, true}, {(void **)&a->carry[1].count, K ? sizeof(uint32_t) : 0, true},
        {(void **)&a->carry[0].gid, K * sizeof(uint32_t), false}, {(void **)&a->carry[1].gid, K * sizeof(uint32_t), false},
        {(void **)&a->carry[0].head, K * sizeof(rg::U32x2), false}, {(void **)&a->carry[1].head, K * sizeof(rg::U32x2), false},
        {(void **)&a->carry[0].abcd, K * sizeof(rg::I32x4), false}, {(void **)&a->carry[1].abcd, K * sizeof(rg::I32x4), false}};
    for (auto &c : cols) {
        if (!c.bytes) continue;
        hipError_t e = hipMalloc(c.ptr, c.bytes);
        if (e == hipSuccess && c.zero) e = hipMemsetAsync(*c.ptr, 0, c.bytes, t->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(t->stream);
            assembler_release_events(a);
            return fail(t, -2, "%s: %zu bytes of scratch: %s", who, c.bytes, hipGetErrorString(e));
        }
    }
    if (hipStreamSynchronize(t->stream) != hipSuccess) { assembler_release_events(a); return fail(t, -2, "%s: hipStreamSynchronize failed", who); }
    a->carry_cap = carry_capacity;
    return 0;
}

static void assembler_release(struct rg_assembler *a)
{
    assembler_release_events(a);
    void *cols[] = {a->sc.cnt, a->sc.bitmap, a->sc.rowof, a->sc.wordoff, a->sc.scalars};
    for (void *c : cols) if (c) (void)hipFree(c);
    release(a->as, rg_assembler::AS_COLUMNS);
    release(a->rt, rg_assembler::RT_COLUMNS);
    release(a->rc, rg_assembler::RC_COLUMNS);
    *a = rg_assembler{};
}

int rg_assembler_destroy(rg_assembler_t *a)
{
    if (!a) return 0;
    if (rg_table *t = a->t) {
        (void)hipSetDevice(t->device);
        if (t->stream) (void)hipStreamSynchronize(t->stream);
        t->assemblers.erase(std::remove(t->assemblers.begin(), t->assemblers.end(), a), t->assemblers.end());
        assembler_release(a);
    }
    delete a;
    return 0;
}

int rg_assembler_create(rg_table_t *t, uint32_t max_events, uint32_t max_expired, rg_assembler_t **out)
{
    if (!t) return -1;
    if (!out) return fail(t, -1, "rg_assembler_create: a is NULL");
    *out = nullptr;
    if ((uint64_t)max_events + max_expired >= (1ull << 31))
        return fail(t, -1, "rg_assembler_create: %u + %u events: a run holds fewer than 2^31 (the ids of the expired source carry bit 31)", max_events, max_expired);
    if (bind(t)) return -2;
    rg_assembler *a = new rg_assembler();
    a->t = t; a->max_events = max_events; a->max_expired = max_expired;
    rg::AsmParams &p = a->sc;
    const size_t G = t->G, words = (G + 63) / 64;
    p.groups = t->G; p.words = (uint32_t)words;
    struct { void **ptr; size_t bytes; bool zero; } cols[] = {
        {(void **)&p.cnt, G * sizeof(uint32_t), true}, {(void **)&p.bitmap, words * sizeof(unsigned long long), true}, {(void **)&p.rowof, G * sizeof(uint32_t), true},
        {(void **)&p.wordoff, (words + 1) * sizeof(uint32_t), false}, {(void **)&p.scalars, (rg::ASM_SCALARS + 3) * sizeof(uint32_t), true}};
    for (auto &c : cols) {
        hipError_t e = hipMalloc(c.ptr, c.bytes);
        if (e == hipSuccess && c.zero) e = hipMemsetAsync(*c.ptr, 0, c.bytes, t->stream);
        if (e != hipSuccess) {
            assembler_release(a);
            delete a;
            return fail(t, -2, "rg_assembler_create: %zu bytes of scratch: %s", c.bytes, hipGetErrorString(e));
        }
    }
    if (int rc = assembler_size_events(a, 0, "rg_assembler_create")) { assembler_release(a); delete a; return rc; }
    t->assemblers.push_back(a);
    *out = a;
    return 0;
}

int rg_assemble32(rg_assembler_t *a, const rg_arrivals_t *in, const rg_assembled_t *out, int memspace)
{
    if (!a || !a->t) return -1;
    rg_table *t = a->t;
    const char *who = "rg_assemble32";
    if (!in || !out) return fail(t, -1, "%s: NULL arrivals or batch", who);
    if (!in->count || (in->capacity && (!in->gid || !in->head || !in->abcd))) return fail(t, -1, "%s: count, gid, head and abcd of the arrival log are required", who);
    if (!out->gid || !out->count || !out->rounds || !out->head || !out->abcd || !out->origin || !out->stats || (out->deferred_capacity && !out->deferred))
        return fail(t, -1, "%s: gid, count, rounds, head, abcd, origin and stats of the batch are required (and deferred, unless deferred_capacity is 0)", who);
    if (out->capacity == 0 || out->capacity > t->G) return fail(t, -1, "%s: capacity %u outside 1 .. %u groups", who, out->capacity, t->G);
    if (out->max_rounds < 1 || out->max_rounds > 64) return fail(t, -1, "%s: max_rounds %u outside 1 .. 64", who, out->max_rounds);
    if (in->capacity > a->max_events) return fail(t, -1, "%s: an arrival log of %u events, the assembler was created for %u", who, in->capacity, a->max_events);
    const int sources = (in->expired_gid != nullptr) + (in->expired_epoch != nullptr) + (in->expired_count != nullptr);
    if (sources != 0 && sources != 3) return fail(t, -1, "%s: the expired source comes as all three columns or none", who);
    const bool expired = sources == 3;
    if (expired && in->expired_capacity > a->max_expired)
        return fail(t, -1, "%s: an expired source of %u entries, the assembler was created for %u", who, in->expired_capacity, a->max_expired);
    if (memspace != RG_MEM_DEVICE && memspace != RG_MEM_HOST) return fail(t, -1, "%s: unknown memspace %d", who, memspace);
    if (!a->sc.seg) return fail(t, -1, "%s: the assembler holds no scratch (an rg_assembler_carry_enable ran out of memory): enable again, or destroy it", who);
    if (a->carry_cap && t->auto_window)
        return fail(t, -1, "%s: a carrying assembler on a table with RG_OPT_AUTO_INDEX_BASE: a base that a decided row moves would leave the group's carried rows relative to the old one", who);
    const uint32_t C = out->capacity, D = out->max_rounds, ex_cap = expired ? in->expired_capacity : 0u;
    const size_t cells = (size_t)C * D;
    rg::AsmParams p = a->sc;
    p.in_cap = in->capacity; p.ex_cap = ex_cap; p.C = C; p.D = D; p.deferred_cap = out->deferred_capacity;
    if (a->carry_cap) {                                                // the carry stays in the assembler's device memory in both memspaces
        const rg_assembler::Carry &rd = a->carry[a->runs & 1u], &wr = a->carry[(a->runs & 1u) ^ 1u];
        p.carry_cap = a->carry_cap;
        p.cr_count = rd.count; p.cr_gid = rd.gid; p.cr_head = rd.head; p.cr_abcd = rd.abcd;
        p.cw_count = wr.count; p.cw_gid = wr.gid; p.cw_head = wr.head; p.cw_abcd = wr.abcd;
    }
    if (memspace == RG_MEM_DEVICE) {
        void *v[16] = {};
        const struct { const void *ptr; const char *what; } cols[] = {
            {in->count, "count"}, {in->gid, "gid"}, {in->head, "head"}, {in->abcd, "abcd"}, {in->expired_gid, "expired_gid"}, {in->expired_epoch, "expired_epoch"},
            {in->expired_count, "expired_count"}, {out->gid, "the batch's gid"}, {out->count, "the batch's count"}, {out->rounds, "rounds"}, {out->head, "the batch's head"},
            {out->abcd, "the batch's abcd"}, {out->origin, "origin"}, {out->deferred, "deferred"}, {out->stats, "stats"}};
        int k = 0;
        for (const auto &c : cols) if (int rc = device_visible(t, "rg_assemble32", c.ptr, c.what, &v[k++])) return rc;
        p.in_count = (const uint32_t *)v[0]; p.in_gid = (const uint32_t *)v[1]; p.in_head = (const rg::U32x2 *)v[2]; p.in_abcd = (const rg::I32x4 *)v[3];
        p.ex_gid = (const uint32_t *)v[4]; p.ex_epoch = (const uint32_t *)v[5]; p.ex_count = (const uint32_t *)v[6];
        p.gid = (uint32_t *)v[7]; p.count = (uint32_t *)v[8]; p.rounds = (uint32_t *)v[9]; p.head = (rg::U32x2 *)v[10]; p.abcd = (rg::I32x4 *)v[11];
        p.origin = (uint32_t *)v[12]; p.deferred = (uint32_t *)v[13]; p.stats = (uint32_t *)v[14];
        if (bind(t)) return -2;
        HIP_TRY(t, rg::launch_assemble(p, t->stream));
        a->ran = true; a->last_C = C; a->last_D = D; a->last_in_cap = in->capacity; a->last_ex_cap = ex_cap; a->runs += 1;
        return 0;
    }
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    // host memory: stage the sources in (as much of them as this run reads), run, bring back what the run wrote — rows 0 .. n - 1 of rounds 0 .. R - 1 — and nothing else
    const uint32_t m = *in->count < in->capacity ? *in->count : in->capacity;
    const uint32_t e = !expired || *in->expired_count == 0xFFFFFFFFu ? 0u : (*in->expired_count < ex_cap ? *in->expired_count : ex_cap);
    typedef rg_assembler A;
    const uint32_t words_in[2] = {*in->count, expired ? *in->expired_count : 0u};
    uint32_t *ow = nullptr;                                            // {n, R, stats[4]}
    if (stage_in(t, a->as[A::IN_WORDS], words_in, 2, s, &p.in_count) || stage_in(t, a->as[A::IN_GID], in->gid, m, s, &p.in_gid) ||
        stage_in(t, a->as[A::IN_HEAD], in->head, m, s, &p.in_head) || stage_in(t, a->as[A::IN_ABCD], in->abcd, m, s, &p.in_abcd) ||
        stage_in(t, a->as[A::EX_GID], in->expired_gid, e, s, &p.ex_gid) || stage_in(t, a->as[A::EX_EPOCH], in->expired_epoch, e, s, &p.ex_epoch) ||
        stage_out(t, a->as[A::OUT_GID], C, &p.gid) || stage_out(t, a->as[A::OUT_WORDS], 6, &ow) || stage_out(t, a->as[A::OUT_HEAD], cells, &p.head) ||
        stage_out(t, a->as[A::OUT_ABCD], cells, &p.abcd) || stage_out(t, a->as[A::OUT_ORIGIN], cells, &p.origin) ||
        stage_out(t, a->as[A::OUT_DEFERRED], out->deferred_capacity, &p.deferred))
        return -2;
    p.ex_count = expired ? p.in_count + 1 : nullptr;
    p.count = ow; p.rounds = ow + 1; p.stats = ow + 2;
    HIP_TRY(t, rg::launch_assemble(p, s));
    a->ran = true; a->last_C = C; a->last_D = D; a->last_in_cap = in->capacity; a->last_ex_cap = ex_cap; a->runs += 1;
    uint32_t back[6] = {};
    HIP_TRY(t, hipMemcpyAsync(back, ow, sizeof back, hipMemcpyDeviceToHost, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    const uint32_t n = back[0], R = back[1];
    *out->count = n; *out->rounds = R;
    memcpy(out->stats, back + 2, 4 * sizeof(uint32_t));
    HIP_TRY(t, col_down(a->as[A::OUT_GID], out->gid, 0, n, s));
    for (uint32_t r = 0; r < R; r++) {
        const size_t at = (size_t)r * C;
        HIP_TRY(t, col_down(a->as[A::OUT_HEAD], out->head, at, n, s));
        HIP_TRY(t, col_down(a->as[A::OUT_ABCD], out->abcd, at, n, s));
        HIP_TRY(t, col_down(a->as[A::OUT_ORIGIN], out->origin, at, n, s));
    }
    const uint32_t kept = back[3] < out->deferred_capacity ? back[3] : out->deferred_capacity;
    HIP_TRY(t, col_down(a->as[A::OUT_DEFERRED], out->deferred, 0, kept, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

/* ---- routing a decided batch back to arrival order (rg_route32; kernels: rg_route.hpp) ----------------------------------------------- */
// rg_route32 (carried == nullptr) and rg_route32_carry: the same checks, staging and launch_route; the second adds the carried columns and their pass
static int route32(rg_assembler_t *a, const rg_decided_t *in, const rg_routed_t *out, const rg_routed_carry_t *carried, bool carry, int memspace, const char *who)
{
    if (!a || !a->t) return -1;
    rg_table *t = a->t;
    if (!in || !out) return fail(t, -1, "%s: NULL decided batch or routed columns", who);
    if (carry && !a->carry_cap) return fail(t, -1, "%s: the assembler has no carry (rg_assembler_carry_enable)", who);
    if (carry && (!carried || (carried->capacity && (!carried->cell || !carried->row || !carried->persist32))))
        return fail(t, -1, "%s: cell, row and persist32 of the carried columns are required", who);
    if (carry && carried->capacity != a->carry_cap)
        return fail(t, -1, "%s: a carried capacity of %u, the assembler's carry holds %u", who, carried->capacity, a->carry_cap);
    if (carry && (uint64_t)in->capacity * in->max_rounds > (1ull << 31))
        return fail(t, -1, "%s: %u x %u cells: a cell index beside RG_ROUTE_CARRIED holds at most 2^31", who, in->capacity, in->max_rounds);
    if (!in->gid || !in->count || !in->rounds || !in->origin || !in->row || !in->persist32)
        return fail(t, -1, "%s: gid, count, rounds, origin, row and persist32 of the decided batch are required", who);
    if (!out->counts || (out->arrival_capacity && (!out->cell || !out->row || !out->persist32)) || (out->persist_capacity && !out->persist_list) ||
        (out->attention_capacity && !out->attention))
        return fail(t, -1, "%s: cell, row, persist32 and counts of the routed columns are required (and persist_list and attention, unless their capacity is 0)", who);
    if ((in->send_head != nullptr) != (in->send != nullptr)) return fail(t, -1, "%s: the send table comes as send_head and send, or as neither", who);
    const bool sends = in->send != nullptr && t->F > 0;
    if (sends && (!out->send_offset || (out->send_capacity && !out->send_list)))
        return fail(t, -1, "%s: a send table needs send_offset (and send_list, unless send_capacity is 0)", who);
    const int triple = (out->expired_cell != nullptr) + (out->expired_row != nullptr) + (out->expired_persist32 != nullptr);
    if (triple != 0 && triple != 3) return fail(t, -1, "%s: the expired columns come as all three or none", who);
    const bool expired = triple == 3;
    if (in->capacity == 0 || in->capacity > t->G) return fail(t, -1, "%s: capacity %u outside 1 .. %u groups", who, in->capacity, t->G);
    if (in->max_rounds < 1 || in->max_rounds > 64) return fail(t, -1, "%s: max_rounds %u outside 1 .. 64", who, in->max_rounds);
    if ((uint64_t)in->capacity * in->max_rounds >= 0xFFFFFFFFull)
        return fail(t, -1, "%s: %u x %u cells: a cell index holds fewer than 2^32 - 1", who, in->capacity, in->max_rounds);
    if (memspace != RG_MEM_DEVICE && memspace != RG_MEM_HOST) return fail(t, -1, "%s: unknown memspace %d", who, memspace);
    if (!a->ran) return fail(t, -1, "%s: the assembler has not run yet: there is no run to route", who);
    if (in->capacity != a->last_C || in->max_rounds != a->last_D)
        return fail(t, -1, "%s: capacity %u and max_rounds %u, the assembler's last run had %u and %u", who, in->capacity, in->max_rounds, a->last_C, a->last_D);
    if (out->arrival_capacity != a->last_in_cap)
        return fail(t, -1, "%s: an arrival capacity of %u, the assembler's last run had %u", who, out->arrival_capacity, a->last_in_cap);
    if (expired && out->expired_capacity != a->last_ex_cap)
        return fail(t, -1, "%s: an expired capacity of %u, the assembler's last run had %u", who, out->expired_capacity, a->last_ex_cap);
    const uint32_t C = in->capacity, D = in->max_rounds, F = t->F, in_cap = out->arrival_capacity, ex_cap = expired ? out->expired_capacity : 0u;
    rg::RouteParams p{};
    p.C = C; p.D = D; p.F = F; p.in_cap = in_cap; p.ex_cap = ex_cap; p.last = a->sc.scalars + rg::ASM_LAST; p.span = rg::route_span(C, D, F); p.bpr = (uint32_t)((C + 4ull * p.span - 1) / (4ull * p.span));
    p.persist_cap = out->persist_capacity; p.attention_cap = out->attention_capacity; p.send_cap = sends ? out->send_capacity : 0u;
    const size_t W = (size_t)D * p.bpr * 4, Ws = (size_t)F * p.bpr * 4;
    typedef rg_assembler A;
    rg::RouteCarryParams cp{};
    cp.last = p.last; cp.where = a->sc.where; cp.in_cap = in_cap; cp.ex_cap = a->last_ex_cap; cp.carry_cap = a->carry_cap; cp.cells = C * D;
    if (memspace == RG_MEM_DEVICE) {
        void *v[24] = {};
        const struct { const void *ptr; const char *what; } cols[] = {
            {in->gid, "gid"}, {in->count, "count"}, {in->rounds, "rounds"}, {in->origin, "origin"}, {in->row, "the decided row"}, {in->persist32, "the decided persist32"},
            {in->send_head, "send_head"}, {in->send, "send"}, {out->cell, "cell"}, {out->row, "the routed row"}, {out->persist32, "the routed persist32"},
            {out->expired_cell, "expired_cell"}, {out->expired_row, "expired_row"}, {out->expired_persist32, "expired_persist32"}, {out->persist_list, "persist_list"},
            {out->attention, "attention"}, {out->send_list, "send_list"}, {out->send_offset, "send_offset"}, {out->counts, "counts"},
            {carry ? carried->cell : nullptr, "the carried cell"}, {carry ? carried->row : nullptr, "the carried row"},
            {carry ? carried->persist32 : nullptr, "the carried persist32"}};
        int k = 0;
        for (const auto &c : cols) if (int rc = device_visible(t, who, c.ptr, c.what, &v[k++])) return rc;
        if (bind(t)) return -2;
        if (stage_out(t, a->as[A::ROUTE_PC], W + 1, &p.pc) || stage_out(t, a->as[A::ROUTE_AC], W + 1, &p.ac) || (sends && stage_out(t, a->as[A::ROUTE_SC], Ws + 1, &p.sc))) return -2;
        p.gid = (const uint32_t *)v[0]; p.count = (const uint32_t *)v[1]; p.rounds = (const uint32_t *)v[2]; p.origin = (const uint32_t *)v[3];
        p.row = (const rg::I32x4 *)v[4]; p.persist32 = (const rg::I32x4 *)v[5]; p.send = sends ? (const rg_send_t *)v[7] : nullptr;
        p.cell = (uint32_t *)v[8]; p.out_row = (rg::I32x4 *)v[9]; p.out_persist = (rg::I32x4 *)v[10];
        p.ex_cell = (uint32_t *)v[11]; p.ex_row = (rg::I32x4 *)v[12]; p.ex_persist = (rg::I32x4 *)v[13];
        p.persist_list = (rg::U32x2 *)v[14]; p.attention = (rg::U32x2 *)v[15]; p.send_list = (rg::U32x2 *)v[16]; p.send_offset = (uint32_t *)v[17]; p.counts = (uint32_t *)v[18];
        HIP_TRY(t, rg::launch_route(p, t->stream));
        if (carry) {
            cp.row = p.row; cp.persist32 = p.persist32; cp.cell = p.cell; cp.ex_cell = p.ex_cell;
            cp.cr_cell = (uint32_t *)v[19]; cp.cr_row = (rg::I32x4 *)v[20]; cp.cr_persist = (rg::I32x4 *)v[21];
            HIP_TRY(t, rg::launch_route_carry(cp, t->stream));
        }
        return 0;
    }
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    // host memory: the e and m of the run come back first; then rows 0 .. n - 1 of rounds 0 .. R - 1 go in, and with them what the routed columns hold below m / e — a
    // placed entry is overwritten, any other travels back as it came —; out come the entries below m / e and what the lists hold
    uint32_t last[3] = {};
    HIP_TRY(t, hipMemcpyAsync(last, a->sc.scalars + rg::ASM_LAST, sizeof last, hipMemcpyDeviceToHost, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    const uint32_t e = expired ? (last[0] < ex_cap ? last[0] : ex_cap) : 0u, m = last[1] < in_cap ? last[1] : in_cap;
    const uint32_t n = *in->count < C ? *in->count : C, R = *in->rounds < 1 ? 1u : (*in->rounds < D ? *in->rounds : D);
    const size_t cells = (size_t)C * D;
    Staging *rt = a->rt;
    const uint32_t words[2] = {n, R};
    // every column gets a buffer, an absent or empty one 16 bytes
    auto col = [&](int k, size_t len, auto **dev) { return stage_out(t, rt[k], len ? len : 16 / sizeof(**dev), dev); };
    if (stage_in(t, rt[A::RT_WORDS], words, 2, s, &p.count) || col(A::RT_GID, C, &p.gid) || col(A::RT_ORIGIN, cells, &p.origin) || col(A::RT_ROW, cells, &p.row) ||
        col(A::RT_PERSIST, cells, &p.persist32) || col(A::RT_SEND, sends ? (size_t)F * C : 0, &p.send) || col(A::RT_CELL, m, &p.cell) || col(A::RT_OROW, m, &p.out_row) ||
        col(A::RT_OPERSIST, m, &p.out_persist) || col(A::RT_XCELL, e, &p.ex_cell) || col(A::RT_XROW, e, &p.ex_row) || col(A::RT_XPERSIST, e, &p.ex_persist) ||
        col(A::RT_PLIST, p.persist_cap, &p.persist_list) || col(A::RT_ALIST, p.attention_cap, &p.attention) || col(A::RT_SLIST, p.send_cap, &p.send_list) ||
        col(A::RT_SOFF, (size_t)F + 1, &p.send_offset) || col(A::RT_COUNTS, 4, &p.counts) || col(A::RT_PC, W + 1, &p.pc) || col(A::RT_AC, W + 1, &p.ac) ||
        col(A::RT_SC, Ws + 1, &p.sc))
        return -2;
    p.rounds = p.count + 1;
    if (!sends) p.send = nullptr;
    if (!expired) p.ex_cell = nullptr, p.ex_row = p.ex_persist = nullptr;
    HIP_TRY(t, col_up(rt[A::RT_GID], in->gid, 0, n, s));
    for (uint32_t r = 0; r < R; r++) {
        const size_t at = (size_t)r * C;
        HIP_TRY(t, col_up(rt[A::RT_ORIGIN], in->origin, at, n, s));
        HIP_TRY(t, col_up(rt[A::RT_ROW], in->row, at, n, s));
        HIP_TRY(t, col_up(rt[A::RT_PERSIST], in->persist32, at, n, s));
    }
    for (uint32_t j = 0; sends && j < F; j++) HIP_TRY(t, col_up(rt[A::RT_SEND], in->send, (size_t)j * C, n, s));
    HIP_TRY(t, col_up(rt[A::RT_OROW], out->row, 0, m, s));
    HIP_TRY(t, col_up(rt[A::RT_OPERSIST], out->persist32, 0, m, s));
    if (expired) {
        HIP_TRY(t, col_up(rt[A::RT_XROW], out->expired_row, 0, e, s));
        HIP_TRY(t, col_up(rt[A::RT_XPERSIST], out->expired_persist32, 0, e, s));
    }
    HIP_TRY(t, rg::launch_route(p, s));
    const uint32_t q = carry ? (last[2] < a->carry_cap ? last[2] : a->carry_cap) : 0u;
    if (carry) {                                                       // the carried columns: as the arrival columns, entries below q
        if (stage_out(t, a->rc[A::RC_CELL], (size_t)q + 1, &cp.cr_cell) || stage_out(t, a->rc[A::RC_ROW], (size_t)q + 1, &cp.cr_row) ||
            stage_out(t, a->rc[A::RC_PERSIST], (size_t)q + 1, &cp.cr_persist))
            return -2;
        cp.row = p.row; cp.persist32 = p.persist32; cp.cell = p.cell; cp.ex_cell = p.ex_cell;
        HIP_TRY(t, col_up(a->rc[A::RC_ROW], carried->row, 0, q, s));
        HIP_TRY(t, col_up(a->rc[A::RC_PERSIST], carried->persist32, 0, q, s));
        HIP_TRY(t, rg::launch_route_carry(cp, s));
    }
    uint32_t counts[4] = {};
    HIP_TRY(t, col_down(rt[A::RT_COUNTS], counts, 0, 4, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    memcpy(out->counts, counts, sizeof counts);
    HIP_TRY(t, col_down(rt[A::RT_CELL], out->cell, 0, m, s));
    HIP_TRY(t, col_down(rt[A::RT_OROW], out->row, 0, m, s));
    HIP_TRY(t, col_down(rt[A::RT_OPERSIST], out->persist32, 0, m, s));
    if (expired) {
        HIP_TRY(t, col_down(rt[A::RT_XCELL], out->expired_cell, 0, e, s));
        HIP_TRY(t, col_down(rt[A::RT_XROW], out->expired_row, 0, e, s));
        HIP_TRY(t, col_down(rt[A::RT_XPERSIST], out->expired_persist32, 0, e, s));
    }
    HIP_TRY(t, col_down(rt[A::RT_PLIST], out->persist_list, 0, counts[0] < p.persist_cap ? counts[0] : p.persist_cap, s));
    HIP_TRY(t, col_down(rt[A::RT_ALIST], out->attention, 0, counts[1] < p.attention_cap ? counts[1] : p.attention_cap, s));
    if (sends) {
        HIP_TRY(t, col_down(rt[A::RT_SLIST], out->send_list, 0, counts[2] < p.send_cap ? counts[2] : p.send_cap, s));
        HIP_TRY(t, col_down(rt[A::RT_SOFF], out->send_offset, 0, (size_t)F + 1, s));
    }
    if (carry) {
        HIP_TRY(t, col_down(a->rc[A::RC_CELL], carried->cell, 0, q, s));
        HIP_TRY(t, col_down(a->rc[A::RC_ROW], carried->row, 0, q, s));
        HIP_TRY(t, col_down(a->rc[A::RC_PERSIST], carried->persist32, 0, q, s));
    }
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

int rg_route32(rg_assembler_t *a, const rg_decided_t *in, const rg_routed_t *out, int memspace) { return route32(a, in, out, nullptr, false, memspace, "rg_route32"); }

int rg_route32_carry(rg_assembler_t *a, const rg_decided_t *in, const rg_routed_t *out, const rg_routed_carry_t *carried, int memspace)
{
    return route32(a, in, out, carried, true, memspace, "rg_route32_carry");
}

/* ---- the carry of an assembler (include/raftgpu.h, "carrying deferred events") -------------------------------------------------------- */
int rg_assembler_carry_enable(rg_assembler_t *a, uint32_t carry_capacity)
{
    if (!a || !a->t) return -1;
    rg_table *t = a->t;
    const char *who = "rg_assembler_carry_enable";
    if (carry_capacity && (a->max_events >= (1u << 30) || a->max_expired >= (1u << 30) || carry_capacity >= (1u << 30)))
        return fail(t, -1, "%s: max_events %u, max_expired %u, carry_capacity %u: each stays below 2^30 (the ids of carried slots carry bit 30)", who, a->max_events,
                    a->max_expired, carry_capacity);
    if (bind(t)) return -2;
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return assembler_size_events(a, carry_capacity, who);
}

int rg_assembler_carry_reset(rg_assembler_t *a)
{
    if (!a || !a->t) return -1;
    rg_table *t = a->t;
    if (!a->carry_cap) return fail(t, -1, "rg_assembler_carry_reset: the assembler has no carry (rg_assembler_carry_enable)");
    if (bind(t)) return -2;
    HIP_TRY(t, hipMemsetAsync(a->carry[a->runs & 1u].count, 0, sizeof(uint32_t), t->stream));
    return 0;
}

int rg_assembler_carry_read(rg_assembler_t *a, int which, uint32_t capacity, uint32_t *count, uint32_t *gid, rg_ev_head_t *head, rg_ev_quad32_t *abcd)
{
    if (!a || !a->t) return -1;
    rg_table *t = a->t;
    const char *who = "rg_assembler_carry_read";
    if (!a->carry_cap) return fail(t, -1, "%s: the assembler has no carry (rg_assembler_carry_enable)", who);
    if (which != RG_CARRY_NEXT && which != RG_CARRY_LAST) return fail(t, -1, "%s: unknown carry %d", who, which);
    if (!count || (capacity && (!gid || !head || !abcd))) return fail(t, -1, "%s: count is required (and gid, head and abcd, unless capacity is 0)", who);
    if (bind(t)) return -2;
    const rg_assembler::Carry &c = a->carry[(a->runs & 1u) ^ (which == RG_CARRY_LAST ? 1u : 0u)];
    hipStream_t s = t->stream;
    uint32_t q = 0;
    HIP_TRY(t, hipMemcpyAsync(&q, c.count, sizeof q, hipMemcpyDeviceToHost, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    q = q < a->carry_cap ? q : a->carry_cap;
    *count = q;
    const size_t k = q < capacity ? q : capacity;
    if (k) {
        HIP_TRY(t, hipMemcpyAsync(gid, c.gid, k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(t, hipMemcpyAsync(head, c.head, k * sizeof(rg_ev_head_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(t, hipMemcpyAsync(abcd, c.abcd, k * sizeof(rg_ev_quad32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(t, hipStreamSynchronize(s));
    }
    return 0;
}

/* ---- the table's groups by class, and state by a list of groups (include/raftgpu.h, rg_scan.hpp) --------------------------------------------- */

int rg_scan(rg_table_t *t, const rg_scan_query_t *q, const rg_scan_result_t *out, int memspace)
{
    if (!t) return -1;
    const char *who = "rg_scan";
    if (!q || !out) return fail(t, -1, "%s: NULL query or result", who);
    if (!out->summary) return fail(t, -1, "%s: summary is required", who);
    if (!out->list && out->list_capacity) return fail(t, -1, "%s: a NULL list with a capacity of %u", who, out->list_capacity);
    if (q->reserved != 0) return fail(t, -1, "%s: reserved is %u, not 0", who, q->reserved);
    if ((q->any | q->all | q->none) > 0xFFFFu) return fail(t, -1, "%s: a mask names a bit above 15 (any 0x%x, all 0x%x, none 0x%x)", who, q->any, q->all, q->none);
    const int64_t most = (int64_t)1 << 62;
    if (q->backlog < 0 || q->backlog > most) return fail(t, -1, "%s: backlog %lld outside [0, 2^62]", who, (long long)q->backlog);
    if (q->lag < 0 || q->lag > most) return fail(t, -1, "%s: lag %lld outside [0, 2^62]", who, (long long)q->lag);
    if (memspace != RG_MEM_DEVICE && memspace != RG_MEM_HOST) return fail(t, -1, "%s: unknown memspace %d", who, memspace);
    const size_t G = t->G, blocks = (G + 255) / 256, waves = blocks * 4;
    rg::ScanParams p{};
    p.t = t->dt; p.deadline = t->timer_deadline; p.has_bases = t->has_bases; p.followers = t->F;
    p.any = q->any; p.all = q->all; p.none = q->none; p.backlog = q->backlog; p.lag = q->lag; p.now = q->now;
    p.list_cap = out->list_capacity;
    void *v[3] = {};
    if (memspace == RG_MEM_DEVICE) {
        const struct { const void *ptr; const char *what; } cols[] = {{out->bits, "bits"}, {out->list, "list"}, {out->summary, "summary"}};
        int k = 0;
        for (const auto &c : cols) if (int rc = device_visible(t, who, c.ptr, c.what, &v[k++])) return rc;
    }
    if (bind(t)) return -2;
    if (stage_out(t, t->scan[S_WC], waves + 1, &p.wc) || stage_out(t, t->scan[S_SEL], waves, &p.sel) || stage_out(t, t->scan[S_PART], blocks * rg::SCAN_WORDS, &p.part)) return -2;
    hipStream_t s = t->stream;
    if (memspace == RG_MEM_DEVICE) {
        p.bits = (uint32_t *)v[0]; p.list = (uint32_t *)v[1]; p.summary = (unsigned long long *)v[2];
        HIP_TRY(t, rg::launch_scan(p, s));
        return 0;
    }
    if ((out->bits && stage_out(t, t->scan[S_BITS], G, &p.bits)) || (p.list_cap && stage_out(t, t->scan[S_LIST], (size_t)p.list_cap, &p.list)) ||
        stage_out(t, t->scan[S_SUMMARY], (size_t)RG_SCAN_SUMMARY, &p.summary))
        return -2;
    HIP_TRY(t, rg::launch_scan(p, s));
    uint64_t summary[RG_SCAN_SUMMARY] = {};
    HIP_TRY(t, col_down(t->scan[S_SUMMARY], summary, 0, (size_t)RG_SCAN_SUMMARY, s));
    if (out->bits) HIP_TRY(t, col_down(t->scan[S_BITS], out->bits, 0, G, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    memcpy(out->summary, summary, sizeof summary);
    const size_t listed = summary[16] < p.list_cap ? (size_t)summary[16] : p.list_cap;      // entries beyond what was written are not touched
    if (listed) {
        HIP_TRY(t, col_down(t->scan[S_LIST], out->list, 0, listed, s));
        HIP_TRY(t, hipStreamSynchronize(s));
    }
    return 0;
}

// the gids of a state list on the device, and room for the image of their columns
static int state_list_stage(rg_table *t, uint32_t n, const uint32_t *gid, rg::StateListParams &p)
{
    p.t = t->dt; p.n = n; p.followers = t->F;
    p.deadline = t->timer_deadline; p.timer_epoch = t->timer_epoch; p.ok = t->health_ok; p.fail = t->health_fail; p.recent = t->health_recent; p.in_flight = t->in_flight;
    if (int rc = stage_in(t, t->scan[L_GID], gid, (size_t)n, t->stream, &p.gid)) return rc;
    return stage_out(t, t->scan[L_IMAGE], (size_t)rg::state_list_columns(t->F) * n, &p.image);
}

int rg_read_state_list(rg_table_t *t, uint32_t n, const uint32_t *gid, rg_group_state_t *d)
{
    if (!t) return -1;
    const char *who = "rg_read_state_list";
    if (n > t->G) return fail(t, -1, "%s: %u groups listed, the table has %u", who, n, t->G);
    if (n == 0) return 0;
    if (!gid) return fail(t, -1, "%s: gid is NULL", who);
    if (!d || !state_complete(d)) return fail(t, -1, "%s: dst or one of its columns is NULL", who);
    for (uint32_t i = 0; i < n; i++)
        if (gid[i] >= t->G) return fail(t, -1, "%s: gid[%u] = %u, the table has %u groups", who, i, gid[i], t->G);
    if (bind(t)) return -2;
    rg::StateListParams p{};
    if (int rc = state_list_stage(t, n, gid, p)) return rc;
    StateImage im(n, t->F);
    hipStream_t s = t->stream;
    HIP_TRY(t, rg::launch_state_gather(p, s));
    HIP_TRY(t, hipMemcpyAsync(im.cells.data(), p.image, im.bytes(), hipMemcpyDeviceToHost, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    unpack_state(im, n, t->F, d);
    return 0;
}

int rg_load_state_list(rg_table_t *t, uint32_t n, const uint32_t *gid, const rg_group_state_t *src)
{
    if (!t) return -1;
    const char *who = "rg_load_state_list";
    if (n > t->G) return fail(t, -1, "%s: %u groups listed, the table has %u", who, n, t->G);
    if (n == 0) return 0;
    if (!gid) return fail(t, -1, "%s: gid is NULL", who);
    if (!src || !state_complete(src)) return fail(t, -1, "%s: src or one of its columns is NULL", who);
    for (uint32_t i = 0; i < n; i++)
        if (gid[i] >= t->G) return fail(t, -1, "%s: gid[%u] = %u, the table has %u groups", who, i, gid[i], t->G);
    {   // distinct gids make every destination the store of one lane
        std::vector<std::pair<uint32_t, uint32_t>> order(n);
        for (uint32_t i = 0; i < n; i++) order[i] = {gid[i], i};
        std::sort(order.begin(), order.end());
        for (uint32_t i = 1; i < n; i++)
            if (order[i].first == order[i - 1].first)
                return fail(t, -1, "%s: gid[%u] and gid[%u] both name group %u", who, order[i - 1].second, order[i].second, order[i].first);
    }
    StateImage im(n, t->F);
    if (int rc = pack_state(t, who, src, n, 0, gid, im)) return rc;        // every row, before anything reaches the device
    if (bind(t)) return -2;
    rg::StateListParams p{};
    if (int rc = state_list_stage(t, n, gid, p)) return rc;
    hipStream_t s = t->stream;
    HIP_TRY(t, hipMemcpyAsync(p.image, im.cells.data(), im.bytes(), hipMemcpyHostToDevice, s));
    HIP_TRY(t, rg::launch_state_scatter(p, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

/* ---- what a launch asks a host to do, as lists (rg_effects32, include/raftgpu.h; kernels: rg_effects.hpp) ------------------------------------ */
int rg_effects32(rg_table_t *t, const rg_effects_in_t *in, const rg_effects_t *out, int memspace)
{
    if (!t) return -1;
    const char *who = "rg_effects32";
    if (!in || !out) return fail(t, -1, "%s: NULL rows or lists", who);
    if (!in->row) return fail(t, -1, "%s: row is required", who);
    if (!out->counts) return fail(t, -1, "%s: counts is required", who);
    if (!out->log_list && out->log_capacity) return fail(t, -1, "%s: a NULL log_list with a capacity of %u", who, out->log_capacity);
    if (!out->commit_list && out->commit_capacity) return fail(t, -1, "%s: a NULL commit_list with a capacity of %u", who, out->commit_capacity);
    if (!out->attention && out->attention_capacity) return fail(t, -1, "%s: a NULL attention list with a capacity of %u", who, out->attention_capacity);
    if (in->capacity == 0 || in->capacity > t->G) return fail(t, -1, "%s: capacity %u outside 1 .. %u groups", who, in->capacity, t->G);
    if (in->max_rounds < 1 || in->max_rounds >= (1u << 24))
        return fail(t, -1, "%s: max_rounds %u outside 1 .. 2^24 - 1 (the rounds of one compact launch)", who, in->max_rounds);
    if ((uint64_t)in->capacity * in->max_rounds >= (1ull << 32))
        return fail(t, -1, "%s: %u x %u cells: a cell index holds fewer than 2^32", who, in->capacity, in->max_rounds);
    if (memspace != RG_MEM_DEVICE && memspace != RG_MEM_HOST) return fail(t, -1, "%s: unknown memspace %d", who, memspace);
    const uint32_t C = in->capacity, D = in->max_rounds;
    const size_t cells = (size_t)C * D;
    rg::EffectsParams p{};
    p.C = C; p.D = D; p.log_cap = out->log_capacity; p.commit_cap = out->commit_capacity; p.attention_cap = out->attention_capacity;
    p.cspan = rg::effects_span(cells); p.rspan = rg::effects_span(C);
    p.Wc = (uint32_t)((cells + p.cspan - 1) / p.cspan); p.Wr = (C + p.rspan - 1) / p.rspan;
    if (memspace == RG_MEM_DEVICE) {
        void *v[8] = {};
        const struct { const void *ptr; const char *what; } cols[] = {{in->gid, "gid"}, {in->count, "count"}, {in->rounds, "rounds"}, {in->row, "row"},
            {out->log_list, "log_list"}, {out->commit_list, "commit_list"}, {out->attention, "attention"}, {out->counts, "counts"}};
        int k = 0;
        for (const auto &c : cols) if (int rc = device_visible(t, who, c.ptr, c.what, &v[k++])) return rc;
        if (bind(t)) return -2;
        if (stage_out(t, t->fx[E_LC], (size_t)p.Wc + 1, &p.lc) || stage_out(t, t->fx[E_AC], (size_t)p.Wc + 1, &p.ac) || stage_out(t, t->fx[E_CC], (size_t)p.Wr + 1, &p.cc)) return -2;
        p.gid = (const uint32_t *)v[0]; p.count = (const uint32_t *)v[1]; p.rounds = (const uint32_t *)v[2]; p.row = (const rg::I32x4 *)v[3];
        p.log_list = (rg::U32x2 *)v[4]; p.commit_list = (rg::I32x4 *)v[5]; p.attention = (rg::U32x2 *)v[6]; p.counts = (uint32_t *)v[7];
        HIP_TRY(t, rg::launch_effects(p, t->stream));
        return 0;
    }
    // host memory: rows 0 .. n - 1 of rounds 0 .. R - 1 (and as much of the gid list) go in, n and R as two words; out come the counts and what the lists hold
    const uint32_t n = !in->count ? C : (*in->count < C ? *in->count : C), R = !in->rounds ? D : (*in->rounds < 1 ? 1u : (*in->rounds < D ? *in->rounds : D));
    for (uint32_t i = 0; in->gid && i < n; i++)
        if (in->gid[i] >= t->G) return fail(t, -1, "%s: gid[%u] = %u, the table has %u groups", who, i, in->gid[i], t->G);
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    Staging *fx = t->fx;
    const uint32_t words[2] = {n, R};
    if (stage_out(t, fx[E_LC], (size_t)p.Wc + 1, &p.lc) || stage_out(t, fx[E_AC], (size_t)p.Wc + 1, &p.ac) || stage_out(t, fx[E_CC], (size_t)p.Wr + 1, &p.cc) ||
        stage_in(t, fx[E_WORDS], words, 2, s, &p.count) || (in->gid && stage_in(t, fx[E_GID], in->gid, (size_t)n, s, &p.gid)) || stage_out(t, fx[E_ROW], cells, &p.row) ||
        (p.log_cap && stage_out(t, fx[E_LOG], (size_t)p.log_cap, &p.log_list)) || (p.commit_cap && stage_out(t, fx[E_COMMIT], (size_t)p.commit_cap, &p.commit_list)) ||
        (p.attention_cap && stage_out(t, fx[E_ATTENTION], (size_t)p.attention_cap, &p.attention)) || stage_out(t, fx[E_COUNTS], 4, &p.counts))
        return -2;
    p.rounds = p.count + 1;
    for (uint32_t r = 0; r < R; r++) HIP_TRY(t, col_up(fx[E_ROW], in->row, (size_t)r * C, n, s));
    HIP_TRY(t, rg::launch_effects(p, s));
    uint32_t counts[4] = {};
    HIP_TRY(t, col_down(fx[E_COUNTS], counts, 0, 4, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    memcpy(out->counts, counts, sizeof counts);
    HIP_TRY(t, col_down(fx[E_LOG], out->log_list, 0, counts[0] < p.log_cap ? counts[0] : p.log_cap, s));          // entries beyond what was written are not touched
    HIP_TRY(t, col_down(fx[E_COMMIT], out->commit_list, 0, counts[1] < p.commit_cap ? counts[1] : p.commit_cap, s));
    HIP_TRY(t, col_down(fx[E_ATTENTION], out->attention, 0, counts[2] < p.attention_cap ? counts[2] : p.attention_cap, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

int rg_submit_wait(rg_table_t *t)
{
    if (!t) return -1;
    if (bind(t, false)) return -2;
    return wait_oldest(t);
}

int rg_submit(rg_table_t *t, const rg_batch_t *in, const rg_outcome_t *out, int memspace)
{
    if (!t) return -1;
    if (int rc = check_batch(t, in, out, memspace == RG_MEM_HOST)) return rc;
    if (in->count == 0) return 0;
    if (bind(t)) return -2;
    const bool sparse = in->gid != nullptr;

    const size_t rows = (size_t)in->rounds * in->count;
    rg::StepParams p = step_params(t, shape_of(in));

    if (memspace == RG_MEM_DEVICE) {
        p.gid = in->gid; p.head = in->head;
        p.ab = (const I64x2 *)in->ab; p.cd = (const I64x2 *)in->cd; p.hint = (const I64x2 *)in->hint;
        p.entry_terms = in->entry_terms;
        p.reply = out->reply; p.logfx = (I64x2 *)out->logfx; p.persist = out->persist;
        return launch(t, p, sparse);
    }
    if (memspace != RG_MEM_HOST) return fail(t, -1, "rg_submit: unknown memspace %d", memspace);

    hipStream_t s = t->stream;
    if (int rc = outcome_wide(t, t->st, rows, p)) return rc;
    if (int rc = upload_wide(t, t->st, in, s, p)) return rc;
    // conditional outputs: rows the kernel does not write come back zeroed (they are only valid when flagged)
    HIP_TRY(t, hipMemsetAsync(p.logfx, 0, rows * sizeof(I64x2), s));
    HIP_TRY(t, hipMemsetAsync(p.persist, 0, rows * sizeof(rg_persist_t), s));
    if (int rc = launch(t, p, sparse)) return rc;
    if (int rc = download_wide(t, t->st, *out, rows, s)) return rc;
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

/* Compact rows decided into the wide outcome columns w (rg_submit32), into the compact outcome rows c32 (rg_submit32c*), or into c32 with w as its overflow
 * columns; either may be nullptr. The callers have checked their arguments and the shape. */
static int submit_compact(rg_table *t, const rg_batch32_t *in, const rg_outcome_t *w, const rg_outcome32_t *c32, int memspace, const char *who)
{
    if (in->count == 0) return 0;
    if (bind(t)) return -2;
    const bool sparse = in->gid != nullptr;
    const size_t rows = (size_t)in->rounds * in->count;
    rg::StepParams p = step_params(t, shape_of(in));
    if (memspace == RG_MEM_DEVICE) {
        p.gid = in->gid; p.head = in->head; p.abcd32 = (const rg::I32x4 *)in->abcd;
        p.entry_terms32 = in->entry_count ? in->entry_terms : nullptr;
        if (c32) { p.out32 = (rg::I32x4 *)c32->row; p.persist32 = (rg::I32x4 *)c32->persist; }
        if (w) { p.reply = w->reply; p.logfx = (I64x2 *)w->logfx; p.persist = w->persist; }
        return launch(t, p, sparse);
    }
    if (memspace != RG_MEM_HOST) return fail(t, -1, "%s: unknown memspace %d", who, memspace);
    hipStream_t s = t->stream;
    BatchCols &c = t->st;
    if (c32 && (stage_out(t, c[C_OUT32], rows, &p.out32) || stage_out(t, c[C_PERSIST32], rows, &p.persist32))) return -2;
    if (w)
        if (int rc = outcome_wide(t, c, rows, p)) return rc;
    if (int rc = upload_compact(t, c, in, s, p)) return rc;
    // conditional rows come back zeroed, as rg_submit's; as overflow columns the reply rows are conditional too
    if (c32) HIP_TRY(t, hipMemsetAsync(p.persist32, 0, rows * sizeof(rg_persist32_t), s));
    if (c32 && w) HIP_TRY(t, hipMemsetAsync(p.reply, 0, rows * sizeof(rg_reply_t), s));
    if (w) {
        HIP_TRY(t, hipMemsetAsync(p.logfx, 0, rows * sizeof(I64x2), s));
        HIP_TRY(t, hipMemsetAsync(p.persist, 0, rows * sizeof(rg_persist_t), s));
    }
    if (int rc = launch(t, p, sparse)) return rc;
    if (c32 && (stage_back(t, c[C_OUT32], c32->row, rows, s) || stage_back(t, c[C_PERSIST32], c32->persist, rows, s))) return -2;
    if (w)
        if (int rc = download_wide(t, c, *w, rows, s)) return rc;
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

/* compact rows, HBM-resident or host: see include/raftgpu.h */
int rg_submit32(rg_table_t *t, const rg_batch32_t *in, const rg_outcome_t *out, int memspace)
{
    if (!t) return -1;
    if (int rc = compact_ok(t, "rg_submit32")) return rc;
    if (!in || !out) return fail(t, -1, "rg_submit32: NULL batch or outcome");
    if (!in->head || !in->abcd) return fail(t, -1, "rg_submit32: head and abcd are required");
    if (!out->reply || !out->logfx || !out->persist) return fail(t, -1, "rg_submit: head/ab/cd/reply/logfx/persist are required");
    if (int rc = check_shape(t, shape_of(in), memspace == RG_MEM_HOST)) return rc;
    return submit_compact(t, in, out, nullptr, memspace, "rg_submit32");
}

int rg_wide_body_workgroups(rg_table_t *t, uint64_t *count, int reset)
{
    if (!t || !count) return -1;
    if (bind(t)) return -2;
    unsigned long long v = 0;
    HIP_TRY(t, hipMemcpyAsync(&v, t->wide_bodies, sizeof v, hipMemcpyDeviceToHost, t->stream));
    if (reset) HIP_TRY(t, hipMemsetAsync(t->wide_bodies, 0, sizeof v, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    *count = v;
    return 0;
}

/* the index base of the compact formats: see include/raftgpu.h */
int rg_index_base_set(rg_table_t *t, uint32_t first, uint32_t count, const int64_t *base)
{
    if (!t) return -1;
    if (!base) return fail(t, -1, "rg_index_base_set: NULL base");
    if ((uint64_t)first + count > t->G) return fail(t, -1, "rg_index_base_set: groups [%u, %u) of %u", first, first + count, t->G);
    for (uint32_t i = 0; i < count; i++)
        if (base[i] < 0) return fail(t, -1, "rg_index_base_set: base[%u] = %lld is negative", i, (long long)base[i]);
    for (uint32_t i = 0; i < count; i++)
        if (base[i] != 0 && !t->has_bases) { t->has_bases = 1; t->config_gen += 1; }       // (sticky: the kernels read the column from now on; recorded ticks are stale)
    if (count == 0) return 0;
    if (bind(t)) return -2;
    HIP_TRY(t, hipMemcpyAsync(t->dt.ibase + first, base, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return 0;
}

int rg_index_base_get(rg_table_t *t, uint32_t first, uint32_t count, int64_t *base)
{
    if (!t) return -1;
    if (!base) return fail(t, -1, "rg_index_base_get: NULL base");
    if ((uint64_t)first + count > t->G) return fail(t, -1, "rg_index_base_get: groups [%u, %u) of %u", first, first + count, t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    HIP_TRY(t, hipMemcpyAsync(base, t->dt.ibase + first, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return 0;
}

/* RG_OPT_AUTO_INDEX_BASE's rule on a caller's mirror (no device involved): see include/raftgpu.h. flush(row) -> the row's flush index in absolute terms. */
extern "C++" template <class Flush>
int advance_bases(uint32_t rounds, uint32_t count, const uint32_t *gid, const rg_ev_head_t *head, int32_t window, uint32_t groups, int64_t *index_base,
                         Flush flush)
{
    if (!head || !index_base || window < 1 || window >= (1 << 30)) return -1;
    if (gid ? count > groups : count != groups) return -2;
    if (gid)
        for (uint32_t i = 0; i < count; i++)
            if (gid[i] >= groups) return -2;
    // every a of the batch is taken against the array as it is on entry: the per-group maxima first, then the moves
    std::vector<int64_t> top(gid ? count : groups, 0);
    for (uint32_t r = 0; r < rounds; r++)
        for (uint32_t i = 0; i < count; i++) {
            const size_t row = (size_t)r * count + i;
            if (RG_HDR_KIND(head[row].hdr) != RG_EV_LOG_FLUSH) continue;
            const int64_t a = flush(row, gid ? gid[i] : i);
            if (a > top[i]) top[i] = a;
        }
    for (uint32_t i = 0; i < (uint32_t)top.size(); i++) {
        int64_t &base = index_base[gid ? gid[i] : i];
        if (top[i] - window > base) base = top[i] - window;
    }
    return 0;
}

int rg_index_base_advance(const rg_batch_t *in, int32_t window, uint32_t groups, int64_t *index_base)
{
    if (!in || !in->ab) return -1;
    return advance_bases(in->rounds, in->count, in->gid, in->head, window, groups, index_base, [&](size_t row, uint32_t) { return (int64_t)in->ab[row].x; });
}

int rg_index_base_advance32(const rg_batch32_t *in, int32_t window, uint32_t groups, int64_t *index_base)
{
    if (!in || !in->abcd) return -1;
    return advance_bases(in->rounds, in->count, in->gid, in->head, window, groups, index_base, [&](size_t row, uint32_t g) {
        const int32_t a = in->abcd[row].a;
        return a <= 0 ? (int64_t)0 : (int64_t)a + index_base[g];      // (read before any move: the moves come after the whole batch; a < 0 is no index)
    });
}

/* which of a row's fields a, b, c, d (bits 0..3) are log indices (rg_device.hpp: index_fields) */
static uint32_t host_index_fields(uint32_t kind)
{
    switch (kind) {
    case RG_EV_AE_REQ: return 0xAu;
    case RG_EV_AE_ACK: return 0x6u;
    case RG_EV_IS_ACK: case RG_EV_RV_REQ: case RG_EV_PV_REQ: case RG_EV_IS_REQ: return 0x2u;
    case RG_EV_LOG_FLUSH: return 0x1u;
    default: return 0u;
    }
}

/* compact rows in, compact outcome rows out (ABI 4), dense (rg_submit32c) or for a list of groups (rg_submit32c_sparse): see include/raftgpu.h */
static int submit32c(rg_table_t *t, const rg_batch32_t *in, const rg_outcome32_t *out, int memspace, bool sparse, const char *who, bool list_rounds = false)
{
    if (!t) return -1;
    if (int rc = compact_ok(t, who)) return rc;
    if (!in || !out) return fail(t, -1, "%s: NULL batch or outcome", who);
    if (!in->head || !in->abcd || !out->row || !out->persist) return fail(t, -1, "%s: head, abcd, row and persist are required", who);
    if (!sparse && in->gid) return fail(t, -1, "rg_submit32c: dense batches only (gid must be NULL); a list of groups goes through rg_submit32c_sparse");
    if (sparse && !in->gid) return fail(t, -1, "%s: gid is required (dense batches go through rg_submit32c)", who);
    const int wides = (out->wide.reply != nullptr) + (out->wide.logfx != nullptr) + (out->wide.persist != nullptr);
    if (wides != 0 && wides != 3) return fail(t, -1, "%s: the overflow columns come as all three or none", who);
    if (int rc = check_shape(t, shape_of(in), memspace == RG_MEM_HOST, list_rounds)) return rc;
    return submit_compact(t, in, wides ? &out->wide : nullptr, out, memspace, who);
}

int rg_submit32c(rg_table_t *t, const rg_batch32_t *in, const rg_outcome32_t *out, int memspace)
{
    return submit32c(t, in, out, memspace, false, "rg_submit32c");
}

int rg_submit32c_sparse(rg_table_t *t, const rg_batch32_t *in, const rg_outcome32_t *out, int memspace)
{
    return submit32c(t, in, out, memspace, true, "rg_submit32c_sparse");
}

int rg_submit32c_sparse_rounds(rg_table_t *t, const rg_batch32_t *in, const rg_outcome32_t *out, int memspace)
{
    return submit32c(t, in, out, memspace, true, "rg_submit32c_sparse_rounds", true);
}

/* host-side: rg_out32_t / rg_persist32_t rows -> the wide columns (no device involved) */
int rg_outcome32_unpack(const rg_outcome32_t *in, uint32_t rounds, uint32_t count, uint32_t *role_epoch, const rg_outcome_t *out)
{
    return rg_outcome32_unpack_rel(in, rounds, count, role_epoch, nullptr, out);
}

int rg_outcome32_unpack_rel(const rg_outcome32_t *in, uint32_t rounds, uint32_t count, uint32_t *role_epoch, const int64_t *index_base, const rg_outcome_t *out)
{
    if (!in || !in->row || !in->persist || !role_epoch || !out || !out->reply || !out->logfx || !out->persist) return -1;
    auto absolute = [&](int32_t v, uint32_t i) { return v == 0 ? (int64_t)0 : (int64_t)v + (index_base ? index_base[i] : 0); };
    for (uint32_t r = 0; r < rounds; r++) {
        for (uint32_t i = 0; i < count; i++) {
            const size_t row = (size_t)r * count + i;
            const rg_out32_t c = in->row[row];
            const uint32_t flags = c.flags & ~RG_F_WIDE_VALUES;
            const bool has_lfx = (flags & (RG_F_COMMIT | RG_F_LOG_APPEND | RG_F_LOG_TRUNC)) != 0 || RG_F_STATUS(flags) == RG_NEED_HOST;
            const bool has_from = (flags & (RG_F_LOG_APPEND | RG_F_LOG_TRUNC)) != 0 || RG_F_STATUS(flags) == RG_NEED_HOST;
            const bool has_per = (flags & RG_F_PERSIST) != 0;
            if (c.flags & RG_F_WIDE_VALUES) {
                if (!in->wide.reply || !in->wide.logfx || !in->wide.persist) return -3;
                out->reply[row] = in->wide.reply[row];
                out->logfx[row] = has_lfx ? in->wide.logfx[row] : rg_logfx_t{0, 0};
                out->persist[row] = has_per ? in->wide.persist[row] : rg_persist_t{0, 0, 0};
                if (out->reply[row].flags != flags) return -4;          // the two copies of a row disagree
                role_epoch[i] = out->reply[row].role_epoch;
                continue;
            }
            if (has_per) role_epoch[i] = in->persist[row].role_epoch;
            out->reply[row] = rg_reply_t{(flags & RG_F_REPLIED) ? (int64_t)c.resp_term : 0, flags, role_epoch[i]};
            out->logfx[row] = has_lfx ? rg_logfx_t{absolute(c.commit_index, i), has_from ? absolute(c.log_from, i) : 0} : rg_logfx_t{0, 0};
            out->persist[row] = has_per ? rg_persist_t{(int64_t)in->persist[row].term, in->persist[row].voted_for, in->persist[row].role}
                                        : rg_persist_t{0, 0, 0};
        }
    }
    return 0;
}

/* host-side packer: rg_batch_t -> rg_batch32_t (no device involved) */
int64_t rg_batch32_pack(const rg_batch_t *in, rg_ev_head_t *head, rg_ev_quad32_t *abcd, int32_t *entry_terms)
{
    return rg_batch32_pack_rel(in, nullptr, head, abcd, entry_terms);
}

int64_t rg_batch32_pack_rel(const rg_batch_t *in, const int64_t *index_base, rg_ev_head_t *head, rg_ev_quad32_t *abcd, int32_t *entry_terms)
{
    if (!in || !in->head || !in->ab || !in->cd || !head || !abcd) return -1;
    if (in->hint) return -2;                                    // hints answer RG_NEED_HOST rows: those batches stay wide
    const size_t rows = (size_t)in->rounds * in->count;
    auto fits = [](int64_t v) { return v >= 0 && v < (int64_t)1 << 31; };
    uint64_t out_terms = 0;
    for (size_t r = 0; r < rows; r++) {
        const uint32_t hdr = in->head[r].hdr & ~(RG_HDR_HINT_BIT | RG_HDR_SAME_TERM | (1u << 11)), aux = in->head[r].aux;
        int64_t a = in->ab[r].x, b = in->ab[r].y, c = in->cd[r].x, d = in->cd[r].y;
        if (RG_HDR_KIND(hdr) == RG_EV_NONE) a = b = c = d = 0;      // a row that is not addressed carries nothing: whatever its fields hold does not travel
        if (index_base) {                                       // a log index x of group g travels as x - base[g]; 0 ("none") as 0; anything at or below the base has no image
            const size_t i = r % in->count;
            const int64_t base = index_base[in->gid ? in->gid[i] : i];
            const uint32_t ix = host_index_fields(RG_HDR_KIND(hdr));
            int64_t *f[4] = {&a, &b, &c, &d};
            for (int k = 0; k < 4; k++)
                if (((ix >> k) & 1u) && *f[k] != 0) { if (*f[k] <= base) return -3; *f[k] -= base; }
        }
        if (!fits(a) || !fits(b) || !fits(c) || !fits(d)) return -3;
        abcd[r] = rg_ev_quad32_t{(int32_t)a, (int32_t)b, (int32_t)c, (int32_t)d};
        head[r].hdr = hdr; head[r].aux = aux;
        const uint32_t n = RG_HDR_N(hdr);
        if (RG_HDR_KIND(hdr) != RG_EV_AE_REQ || n == 0) continue;
        if (!in->entry_terms || (uint64_t)aux + n > in->entry_count) { head[r].aux = 0xFFFFFFFFu; continue; }   // unreadable stays unreadable (RG_BAD_EVENT): aux + n exceeds any entry_count
        const int64_t *e = in->entry_terms + aux;
        bool same = true;
        for (uint32_t k = 0; k < n; k++) { if (!fits(e[k])) return -3; same = same && e[k] == e[0]; }
        if (same) {
            head[r].hdr = hdr | RG_HDR_SAME_TERM; head[r].aux = (uint32_t)e[0];
        } else {
            if (!entry_terms) return -4;
            head[r].aux = (uint32_t)out_terms;
            for (uint32_t k = 0; k < n; k++) entry_terms[out_terms + k] = (int32_t)e[k];
            out_terms += n;
        }
    }
    return (int64_t)out_terms;
}

int rg_replicate(rg_table_t *t, uint32_t count, const uint32_t *gid, const uint8_t *heartbeat, const uint16_t *in_flight,
                 rg_send_head_t *head, rg_send_t *send, int memspace)
{
    if (!t) return -1;
    if (!head || !send) return fail(t, -1, "rg_replicate: head and send are required");
    if (gid ? count > t->G : count != t->G) return fail(t, -1, "rg_replicate: %u rows for %u groups", count, t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    rg::ReplicateParams p{};
    p.t = t->dt; p.count = count;
    if (memspace == RG_MEM_DEVICE) {
        p.gid = gid; p.heartbeat = heartbeat; p.in_flight = in_flight; p.head = head; p.send = send;
        HIP_TRY(t, rg::launch_replicate(p, (int)t->F, t->stream));
        return 0;
    }
    if (memspace != RG_MEM_HOST) return fail(t, -1, "rg_replicate: unknown memspace %d", memspace);
    uint32_t i = 0;
    if (gid)
        if (const int why = bad_gid_list(gid, count, t->G, &i))
            return why == 1 ? fail(t, -1, "rg_replicate: gid[%u]=%u out of range", i, gid[i]) : fail(t, -1, "rg_replicate: gid must be strictly ascending (row %u)", i);
    hipStream_t s = t->stream;
    const size_t F = t->F;
    if (stage_out(t, t->aux[X_SH], count, &p.head) || stage_out(t, t->aux[X_SS], count * F, &p.send)) return -2;
    if (gid && stage_in(t, t->st[C_GID], gid, count, s, &p.gid)) return -2;
    if (heartbeat && stage_in(t, t->aux[X_HB], heartbeat, count, s, &p.heartbeat)) return -2;
    if (in_flight && stage_in(t, t->aux[X_FL], in_flight, count * F, s, &p.in_flight)) return -2;
    HIP_TRY(t, rg::launch_replicate(p, (int)t->F, s));
    if (stage_back(t, t->aux[X_SH], head, count, s) || stage_back(t, t->aux[X_SS], send, count * F, s)) return -2;
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

/* ---- N4: timers --------------------------------------------------------------------------------------- */

int rg_timers_configure(rg_table_t *t, int64_t election_ms, int64_t heartbeat_ms, uint64_t seed)
{
    if (!t) return -1;
    if (election_ms <= 0 || heartbeat_ms <= 0 || election_ms > (INT64_MAX >> 2)) return fail(t, -1, "rg_timers_configure: bad intervals");
    t->election_ms = election_ms; t->heartbeat_ms = heartbeat_ms; t->timer_seed = seed;
    return 0;
}

static rg::TimerParams timer_params(rg_table *t)
{
    rg::TimerParams p{};
    p.deadline = t->timer_deadline; p.epoch = t->timer_epoch; p.ident = t->dt.ident; p.groups = t->G;
    p.election_ms = t->election_ms; p.heartbeat_ms = t->heartbeat_ms; p.seed = t->timer_seed;
    return p;
}

int rg_timers_update(rg_table_t *t, uint32_t rounds, uint32_t count, const uint32_t *gid, const rg_reply_t *reply,
                     const int64_t *now, int memspace)
{
    if (!t) return -1;
    if (!reply || !now || rounds == 0) return fail(t, -1, "rg_timers_update: reply, now and rounds are required");
    if (gid ? (rounds != 1 || count > t->G) : count != t->G) return fail(t, -1, "rg_timers_update: %u rows for %u groups", count, t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    const size_t rows = (size_t)rounds * count;
    rg::TimerParams base = timer_params(t);
    base.count = count; base.gid = gid; base.reply = reply;
    if (memspace == RG_MEM_HOST) {
        if (stage_in(t, t->st[C_REPLY], reply, rows, s, &base.reply)) return -2;
        uint32_t i = 0;
        if (gid && bad_gid_list(gid, count, t->G, &i)) return fail(t, -1, "rg_timers_update: bad gid list at row %u", i);
        if (gid && stage_in(t, t->st[C_GID], gid, count, s, &base.gid)) return -2;
    } else if (memspace != RG_MEM_DEVICE) {
        return fail(t, -1, "rg_timers_update: unknown memspace %d", memspace);
    }
    if (int rc = clock_chunks(t, rounds, now, base, [&](rg::TimerParams &p, uint32_t r0) {
            p.reply = base.reply + (size_t)r0 * count;
            return rg::launch_timers_update(p, s);
        })) return rc;
    if (memspace == RG_MEM_HOST) HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

int rg_timers_update32(rg_table_t *t, uint32_t rounds, const rg_out32_t *row, const rg_persist32_t *persist32, const int64_t *now, int memspace)
{
    if (!t) return -1;
    if (!row || !persist32 || !now || rounds == 0) return fail(t, -1, "rg_timers_update32: row, persist32, now and rounds are required");
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    const uint32_t count = t->G;
    const size_t rows = (size_t)rounds * count;
    rg::TimerParams base = timer_params(t);
    base.count = count; base.out32 = (const rg::I32x4 *)row; base.persist32 = (const rg::I32x4 *)persist32;
    if (memspace == RG_MEM_HOST) {
        if (stage_in(t, t->st[C_OUT32], row, rows, s, &base.out32) || stage_in(t, t->st[C_PERSIST32], persist32, rows, s, &base.persist32)) return -2;
    } else if (memspace != RG_MEM_DEVICE) {
        return fail(t, -1, "rg_timers_update32: unknown memspace %d", memspace);
    }
    if (int rc = clock_chunks(t, rounds, now, base, [&](rg::TimerParams &p, uint32_t r0) {
            p.out32 = base.out32 + (size_t)r0 * count; p.persist32 = base.persist32 + (size_t)r0 * count;
            return rg::launch_timers_update(p, s);
        })) return rc;
    if (memspace == RG_MEM_HOST) HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

int rg_timers_arm(rg_table_t *t, int64_t now)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    rg::TimerParams p = timer_params(t);
    p.now[0] = now;
    HIP_TRY(t, rg::launch_timers_arm(p, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return 0;
}

int rg_timers_expired_epochs(rg_table_t *t, int64_t now, uint32_t *out_gid, uint32_t *out_epoch, uint32_t capacity, uint32_t *out_count, int memspace)
{
    if (!t) return -1;
    if (!out_count || (capacity && !out_gid)) return fail(t, -1, "rg_timers_expired: out_gid/out_count are required");
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    uint32_t *d_out = out_gid, *d_ep = out_epoch;
    const size_t cap = capacity ? capacity : 1;
    if (memspace == RG_MEM_HOST) {
        if (stage_out(t, t->aux[X_TGID], 2 * cap, &d_out)) return -2;          // gids, then epochs
        d_ep = out_epoch ? d_out + cap : nullptr;
    } else if (memspace != RG_MEM_DEVICE) {
        return fail(t, -1, "rg_timers_expired: unknown memspace %d", memspace);
    }
    const uint32_t waves = (t->G + 63) / 64;
    HIP_TRY(t, rg::launch_timers_expired(t->timer_deadline, t->dt.ident, t->G, now, nullptr, t->timer_counts, t->timer_counts + waves, d_out, d_ep, capacity, s));
    uint32_t total = 0;
    HIP_TRY(t, hipMemcpyAsync(&total, t->timer_counts + waves, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    *out_count = total;
    const uint32_t n = total < capacity ? total : capacity;
    if (memspace == RG_MEM_HOST && n) {
        HIP_TRY(t, hipMemcpyAsync(out_gid, d_out, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (out_epoch) HIP_TRY(t, hipMemcpyAsync(out_epoch, d_ep, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(t, hipStreamSynchronize(s));
    }
    return 0;
}

int rg_timers_expired(rg_table_t *t, int64_t now, uint32_t *out_gid, uint32_t capacity, uint32_t *out_count, int memspace)
{
    return rg_timers_expired_epochs(t, now, out_gid, nullptr, capacity, out_count, memspace);
}

int rg_timers_read(rg_table_t *t, uint32_t first, uint32_t count, int64_t *deadline)
{
    if (!t || !deadline) return -1;
    if ((uint64_t)first + count > t->G) return fail(t, -1, "rg_timers_read: range exceeds %u groups", t->G);
    if (bind(t)) return -2;
    HIP_TRY(t, hipMemcpyAsync(deadline, t->timer_deadline + first, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return 0;
}

/* ---- N4b: health ------------------------------------------------------------------------------------- */

static rg::HealthParams health_params(rg_table *t)
{
    rg::HealthParams p{};
    p.ok = t->health_ok; p.fail = t->health_fail; p.recent = t->health_recent; p.t = t->dt;
    p.followers = t->F; p.self = t->self;
    p.counts = t->in_flight;
    return p;
}

int rg_health_update(rg_table_t *t, uint32_t rounds, uint32_t count, const uint32_t *gid, const rg_ev_head_t *head,
                     const rg_reply_t *reply, const int64_t *now, int memspace)
{
    if (!t) return -1;
    if (!head || !reply || !now || rounds == 0) return fail(t, -1, "rg_health_update: head, reply, now and rounds are required");
    if (gid ? (rounds != 1 || count > t->G) : count != t->G) return fail(t, -1, "rg_health_update: %u rows for %u groups", count, t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    const size_t rows = (size_t)rounds * count;
    rg::HealthParams base = health_params(t);
    base.count = count; base.gid = gid; base.head = head; base.reply = reply;
    if (memspace == RG_MEM_HOST) {
        if (stage_in(t, t->st[C_HEAD], head, rows, s, &base.head) || stage_in(t, t->st[C_REPLY], reply, rows, s, &base.reply)) return -2;
        uint32_t i = 0;
        if (gid && bad_gid_list(gid, count, t->G, &i)) return fail(t, -1, "rg_health_update: bad gid list at row %u", i);
        if (gid && stage_in(t, t->st[C_GID], gid, count, s, &base.gid)) return -2;
    } else if (memspace != RG_MEM_DEVICE) {
        return fail(t, -1, "rg_health_update: unknown memspace %d", memspace);
    }
    if (int rc = clock_chunks(t, rounds, now, base, [&](rg::HealthParams &p, uint32_t r0) {
            p.head = base.head + (size_t)r0 * count; p.reply = base.reply + (size_t)r0 * count;
            return rg::launch_health_update(p, s);
        })) return rc;
    if (memspace == RG_MEM_HOST) HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

int rg_health_update32(rg_table_t *t, uint32_t rounds, const rg_ev_head_t *head, const rg_out32_t *row, const int64_t *now, int memspace)
{
    if (!t) return -1;
    if (!head || !row || !now || rounds == 0) return fail(t, -1, "rg_health_update32: head, row, now and rounds are required");
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    const uint32_t count = t->G;
    const size_t rows = (size_t)rounds * count;
    rg::HealthParams base = health_params(t);
    base.count = count; base.head = head; base.out32 = (const rg::I32x4 *)row;
    if (memspace == RG_MEM_HOST) {
        if (stage_in(t, t->st[C_HEAD], head, rows, s, &base.head) || stage_in(t, t->st[C_OUT32], row, rows, s, &base.out32)) return -2;
    } else if (memspace != RG_MEM_DEVICE) {
        return fail(t, -1, "rg_health_update32: unknown memspace %d", memspace);
    }
    if (int rc = clock_chunks(t, rounds, now, base, [&](rg::HealthParams &p, uint32_t r0) {
            p.head = base.head + (size_t)r0 * count; p.out32 = base.out32 + (size_t)r0 * count;
            return rg::launch_health_update(p, s);
        })) return rc;
    if (memspace == RG_MEM_HOST) HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

int rg_health_failure(rg_table_t *t, uint32_t n, const uint32_t *gid, const uint8_t *slot, const uint8_t *flags, int64_t now)
{
    if (!t) return -1;
    if (n && (!gid || !slot || !flags)) return fail(t, -1, "rg_health_failure: gid, slot and flags are required");
    if (n == 0) return 0;
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    const uint32_t *d_gid = nullptr;
    const uint8_t *d_slot = nullptr, *d_flags = nullptr;
    const uint16_t *d_done = nullptr;
    if (stage_in(t, t->aux[X_HGID], gid, n, s, &d_gid) || stage_in(t, t->aux[X_HSLOT], slot, n, s, &d_slot) || stage_in(t, t->aux[X_HFLAG], flags, n, s, &d_flags)) return -2;
    rg::HealthParams p = health_params(t);
    p.now[0] = now;
    std::vector<uint16_t> done;
    if (t->in_flight) {
        // requestInFlight-- per failed request (RG_HEALTH_NO_REQUEST: none was sent). Entries may repeat a (group, follower): their sum goes onto the first of
        // them, so that one lane of the kernel owns a counter
        done.assign(n, 0);
        std::unordered_map<uint64_t, uint32_t> first_of;
        for (uint32_t i = 0; i < n; i++) {
            if (flags[i] & RG_HEALTH_NO_REQUEST) continue;
            const uint32_t at = first_of.emplace(((uint64_t)gid[i] << 8) | slot[i], i).first->second;
            if (done[at] != 0xFFFFu) done[at] += 1;
        }
        if (stage_in(t, t->aux[X_HDONE], done.data(), n, s, &d_done)) return -2;
    }
    HIP_TRY(t, rg::launch_health_failure(p, n, d_gid, d_slot, d_flags, d_done, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    return 0;
}

int rg_ready(rg_table_t *t, int64_t now, int32_t critical_point, int64_t cool_down_ms, uint8_t *ready, int memspace)
{
    if (!t || !ready) return -1;
    if (bind(t)) return -2;
    hipStream_t s = t->stream;
    uint8_t *d_ready = ready;
    if (memspace == RG_MEM_HOST) {
        if (stage_out(t, t->aux[X_READY], t->G, &d_ready)) return -2;
    } else if (memspace != RG_MEM_DEVICE) {
        return fail(t, -1, "rg_ready: unknown memspace %d", memspace);
    }
    HIP_TRY(t, rg::launch_ready(health_params(t), now, critical_point, cool_down_ms, d_ready, s));
    if (memspace == RG_MEM_HOST) {
        if (int rc = stage_back(t, t->aux[X_READY], ready, t->G, s)) return rc;
        HIP_TRY(t, hipStreamSynchronize(s));
    }
    return 0;
}

int rg_health_read(rg_table_t *t, uint32_t first, uint32_t count, int64_t *request_success, int64_t *request_failure,
                   int32_t *recent_failure)
{
    if (!t || !request_success || !request_failure || !recent_failure) return -1;
    if ((uint64_t)first + count > t->G) return fail(t, -1, "rg_health_read: range exceeds %u groups", t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    const size_t n = count, F = t->F, G = t->G;
    std::vector<int64_t> ok(n * F), fl(n * F);
    std::vector<int32_t> rc(n * F);
    for (size_t j = 0; j < F; j++) {
        HIP_TRY(t, hipMemcpyAsync(ok.data() + j * n, t->health_ok + j * G + first, n * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(t, hipMemcpyAsync(fl.data() + j * n, t->health_fail + j * G + first, n * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(t, hipMemcpyAsync(rc.data() + j * n, t->health_recent + j * G + first, n * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    }
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < F; j++) {
            request_success[i * F + j] = ok[j * n + i]; request_failure[i * F + j] = fl[j * n + i]; recent_failure[i * F + j] = rc[j * n + i];
        }
    return 0;
}

static int in_flight_copy(rg_table_t *t, uint32_t first, uint32_t count, uint16_t *out, const uint16_t *in, const char *who)
{
    if (!t) return -1;
    if (!t->in_flight) return fail(t, -1, "%s: the table does not keep in-flight counts (rg_table_option RG_OPT_DEVICE_IN_FLIGHT is 0)", who);
    if (!out && !in) return fail(t, -1, "%s: in_flight is NULL", who);
    if ((uint64_t)first + count > t->G) return fail(t, -1, "%s: range exceeds %u groups", who, t->G);
    if (count == 0) return 0;
    if (bind(t)) return -2;
    const size_t n = count, F = t->F, G = t->G;
    std::vector<uint16_t> col(n * F);                       // follower-major, like the table
    if (in)
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < F; j++) col[j * n + i] = in[i * F + j];
    for (size_t j = 0; j < F; j++) {
        if (in) HIP_TRY(t, hipMemcpyAsync(t->in_flight + j * G + first, col.data() + j * n, n * sizeof(uint16_t), hipMemcpyHostToDevice, t->stream));
        else    HIP_TRY(t, hipMemcpyAsync(col.data() + j * n, t->in_flight + j * G + first, n * sizeof(uint16_t), hipMemcpyDeviceToHost, t->stream));
    }
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    if (out)
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < F; j++) out[i * F + j] = col[j * n + i];
    return 0;
}

int rg_in_flight_read(rg_table_t *t, uint32_t first, uint32_t count, uint16_t *in_flight)
{
    return in_flight_copy(t, first, count, in_flight, nullptr, "rg_in_flight_read");
}

int rg_in_flight_set(rg_table_t *t, uint32_t first, uint32_t count, const uint16_t *in_flight)
{
    return in_flight_copy(t, first, count, nullptr, in_flight, "rg_in_flight_set");
}

const char *rg_step_kernel(rg_table_t *t, uint32_t count)
{
    if (!t) return "";
    return step_lanes(t, count) == 0 ? "rg::step_split_kernel" : "rg::step_kernel";
}

int rg_sync(rg_table_t *t)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return 0;
}

/* ---- device memory helpers --------------------------------------------------------------------- */

int rg_host_alloc(rg_table_t *t, size_t bytes, void **hptr)
{
    if (!t || !hptr) return -1;
    if (bind(t)) return -2;
    HIP_TRY(t, hipHostMalloc(hptr, bytes ? bytes : 16, hipHostMallocDefault));
    return 0;
}

int rg_host_free(rg_table_t *t, void *hptr)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    HIP_TRY(t, hipHostFree(hptr));
    return 0;
}

int rg_dev_alloc(rg_table_t *t, size_t bytes, void **dptr)
{
    if (!t || !dptr) return -1;
    if (bind(t)) return -2;
    HIP_TRY(t, hipMalloc(dptr, bytes ? bytes : 16));
    return 0;
}

int rg_dev_free(rg_table_t *t, void *dptr)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    HIP_TRY(t, hipFree(dptr));
    return 0;
}

int rg_copy_to_device(rg_table_t *t, void *dst, const void *src, size_t bytes)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    HIP_TRY(t, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return 0;
}

int rg_copy_to_host(rg_table_t *t, void *dst, const void *src, size_t bytes)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    HIP_TRY(t, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    return 0;
}

void *rg_stream(rg_table_t *t) { return t ? (void *)t->stream : nullptr; }

/* ---- measurement -------------------------------------------------------------------------------- */

int rg_timing_enable(rg_table_t *t, int on)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    if (drain_timing(t)) return -2;
    t->timing = on != 0;
    return 0;
}

int rg_timing_read(rg_table_t *t, uint64_t *launches, double *total_ms, int reset)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    if (drain_timing(t)) return -2;
    if (launches) *launches = t->t_launches;
    if (total_ms) *total_ms = t->t_total_ms;
    if (reset) { t->t_launches = 0; t->t_total_ms = 0.0; }
    return 0;
}

int rg_timing_begin(rg_table_t *t)
{
    if (!t) return -1;
    if (bind(t)) return -2;
    if (!t->region0) { HIP_TRY(t, hipEventCreate(&t->region0)); HIP_TRY(t, hipEventCreate(&t->region1)); }
    HIP_TRY(t, hipEventRecord(t->region0, t->stream));
    return 0;
}

int rg_timing_end(rg_table_t *t, double *elapsed_ms)
{
    if (!t || !elapsed_ms) return -1;
    if (bind(t)) return -2;
    if (!t->region0) return fail(t, -1, "rg_timing_end without rg_timing_begin");
    HIP_TRY(t, hipEventRecord(t->region1, t->stream));
    HIP_TRY(t, hipEventSynchronize(t->region1));
    float ms = 0.f;
    HIP_TRY(t, hipEventElapsedTime(&ms, t->region0, t->region1));
    *elapsed_ms = ms;
    return 0;
}

int rg_counters_read(rg_table_t *t, uint64_t counters[RG_NUM_COUNTERS], int reset)
{
    if (!t || !counters) return -1;
    if (bind(t)) return -2;
    const size_t n = t->counter_slots * RG_NUM_COUNTERS;
    std::vector<unsigned long long> host(n);
    HIP_TRY(t, hipMemcpyAsync(host.data(), t->counters, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream));
    if (reset) HIP_TRY(t, hipMemsetAsync(t->counters, 0, n * sizeof(unsigned long long), t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
#ifdef RG_PROBE_HWID            // experiment build: the raw slots (wavefront placement and times) go to a file, tools/placement.py reads it
    if (const char *path = getenv("RG_DUMP_COUNTERS")) {
        if (FILE *f = fopen(path, "wb")) { fwrite(host.data(), sizeof(unsigned long long), n, f); fclose(f); }
    }
#endif
    for (int i = 0; i < RG_NUM_COUNTERS; i++) counters[i] = 0;
    for (size_t s = 0; s < t->counter_slots; s++)
        for (int i = 0; i < RG_NUM_COUNTERS; i++) counters[i] += host[s * RG_NUM_COUNTERS + i];
    return 0;
}

int rg_copy_bandwidth(rg_table_t *t, size_t bytes, int iters, double *gbps)
{
    if (!t || !gbps || iters < 1) return -1;
    if (bind(t)) return -2;
    bytes &= ~(size_t)15;
    if (bytes == 0) return fail(t, -1, "rg_copy_bandwidth: bytes must be >= 16");
    void *src = nullptr, *dst = nullptr;
    HIP_TRY(t, hipMalloc(&src, bytes));
    HIP_TRY(t, hipMalloc(&dst, bytes));
    HIP_TRY(t, hipMemsetAsync(src, 1, bytes, t->stream));
    hipEvent_t a, b;
    HIP_TRY(t, hipEventCreate(&a));
    HIP_TRY(t, hipEventCreate(&b));
    HIP_TRY(t, rg::launch_copy(src, dst, bytes, t->stream));      /* warm-up */
    HIP_TRY(t, hipEventRecord(a, t->stream));
    for (int i = 0; i < iters; i++) HIP_TRY(t, rg::launch_copy(src, dst, bytes, t->stream));
    HIP_TRY(t, hipEventRecord(b, t->stream));
    HIP_TRY(t, hipStreamSynchronize(t->stream));
    float ms = 0.f;
    HIP_TRY(t, hipEventElapsedTime(&ms, a, b));
    *gbps = 2.0 * (double)bytes * iters / ((double)ms * 1e-3) / 1e9;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipFree(src); (void)hipFree(dst);
    return 0;
}

}  // extern "C"
