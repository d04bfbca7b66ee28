// rg_scan.hpp — questions about the whole table answered on the device (rg_scan, include/raftgpu.h), and a group's columns gathered into / scattered from a
// contiguous image by a list of gids (rg_read_state_list / rg_load_state_list).
//
// rg_scan: one lane per group, every grid one-dimensional and sized from the group count. Wavefront w = g >> 6 covers ascending groups, so one count per
// wavefront, one prefix sum over the wavefronts (timers_scan_kernel) and popcount(ballot below the lane) give the list in ascending gid order — the scheme of
// timers_count / _scan / _emit and of the route — with no atomic anywhere. Four launches, three without a list, none of which waits for another workgroup:
//   1. scan_class_kernel     per group: the class word (written to `bits` when given), the selection; per wavefront the ballot of the selected lanes (sel[w]) and
//                            its popcount (wc[w]); per workgroup the 16 bit counts, the largest term, the largest / summed backlog and the largest lag (part[b][..]):
//                            ballots for the counts, a shuffle butterfly for the four 64-bit values, the four wavefronts folded through LDS
//   2. timers_scan_kernel    wc into offsets, the number of selected groups behind them
//   3. scan_summary_kernel   ONE workgroup folds part[0 .. workgroups) into summary[0 .. RG_SCAN_SUMMARY): 32 slices of workgroups x one lane per word, then the
//                            slices through LDS; integer sums and maxima, so the order of the fold does not show
//   4. scan_emit_kernel      per group: a selected lane writes its gid at wc[w] + popcount(sel[w] below the lane) when that lies below the capacity
// By layout the class kernel reads 9 x 16 B of a group's columns, 8 B of timer, 8 B of base (a table that had one) and 32 B per follower of a group whose
// `prepared` mark is set; it keeps no state between groups and uses no scratch memory.
//
// RG_SCAN_OFF_IMAGE is the entry check of narrow_body (rg_step.hpp) without what belongs to a launch (force_wide, rounds): load_group, the run-slot clean-up,
// group_to_rel, fits32(.., EV_LIMIT), small_fields_fit, the two base rules and peers_in_image, the read-only twin of stage_peers. The words the step kernel
// loads are the words looked at: for a group whose log is empty that includes the window and run 0 the log's last flush left in the table, which rg_read_state
// reports as zeros. An UNPREPARED group's peer columns are not read, as stage_peers does not stage them: whatever they hold, they do not set the bit.
//
// The state lists: the image of n groups is the layout rg_read_state / rg_load_state stage for a range of n — (5 + K + 2F) columns of n 16-byte elements, column c
// at c * n: term_commit, epoch, window, ident, elect, runs[K], peer_en[F], peer_m[F]. A workgroup of state_gather_kernel / state_scatter_kernel moves 256 elements
// of ONE column (column = blockIdx / ceil(n / 256), workgroup-uniform); the scatter has one more column's worth of workgroups, which reset what rg_load_state
// resets for a loaded group: no timer ticket, the timers' role epoch, fresh health statistics, nothing in flight. Distinct gids (the host checks) make every
// destination the store of exactly one lane.
#pragma once

#include "rg_device.hpp"

namespace rg {

constexpr uint32_t SCAN_WORDS = RG_SCAN_SUMMARY;    // words of a workgroup's partial summary, laid out as the summary itself ([16]: unused, the scan's total goes there)
constexpr uint32_t SCAN_SLICES = 32;                // scan_summary_kernel: 32 slices x 32 lanes, one lane per word

struct ScanParams {
    DevTable t;
    const int64_t *deadline;                        // [G] the timers' tickets
    int32_t has_bases;                              // 0: the ibase column is all zero and is not read (StepParams::has_bases)
    uint32_t followers;
    uint32_t any, all, none;
    int64_t backlog, lag, now;
    uint32_t *bits, *list;                          // nullptr: not wanted
    uint32_t list_cap;
    unsigned long long *summary;                    // [RG_SCAN_SUMMARY]
    // scratch (the table's)
    uint32_t *wc;                                   // [ceil(G / 256) * 4 + 1] selected groups per wavefront -> offsets, last = their sum
    unsigned long long *sel;                        // [ceil(G / 256) * 4] the selected lanes of a wavefront
    unsigned long long *part;                       // [ceil(G / 256)][SCAN_WORDS]
};

hipError_t launch_scan(const ScanParams &p, hipStream_t s);

struct StateListParams {
    DevTable t;
    uint32_t n, followers;
    const uint32_t *gid;                            // [n], every one below t.groups
    I32x4 *image;                                   // [(5 + K + 2 * followers) * n]
    // the scatter's resets
    int64_t *deadline;
    uint32_t *timer_epoch;
    int64_t *ok, *fail;                             // [F][G]
    int32_t *recent;
    uint16_t *in_flight;                            // nullptr: the option is off
};

inline uint32_t state_list_columns(uint32_t followers) { return 5u + (uint32_t)K + 2u * followers; }
hipError_t launch_state_gather(const StateListParams &p, hipStream_t s);
hipError_t launch_state_scatter(const StateListParams &p, hipStream_t s);

#ifdef RG_SCAN_KERNELS

// stage_peers(.., PeersNarrow) without its stores: do the followers' records of a prepared group have an image in [0, EV_LIMIT) relative to `base`. `lag` gets the
// largest last - matchIndex over the followers (what RG_SCAN_LAGGING and summary[20] are made of), INT64_MIN when the group is not prepared.
__device__ __forceinline__ bool peers_in_image(const DevTable &t, uint32_t gi, bool prepared, uint32_t followers, int64_t base, int64_t last, int64_t &lag)
{
    lag = INT64_MIN;
    if (!prepared) return true;
    const uint32_t G = t.groups;
    uint64_t w = 0;
    for (uint32_t j = 0; j < followers; j++) {
        const I64x2 en = t.peer_en[(size_t)j * G + gi];
        const Match m = t.peer_m[(size_t)j * G + gi];
        w |= (uint64_t)to_rel(en.x, base) | (uint64_t)to_rel(en.y, base) | (uint64_t)to_rel(m.match_index, base);
        lag = max64(lag, wsub(last, m.match_index));
    }
    return w < (uint64_t)EV_LIMIT;
}

__device__ __forceinline__ unsigned long long scan_wave_max(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long scan_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void scan_class_kernel(const ScanParams p)
{
    __shared__ unsigned long long fold[4][SCAN_WORDS];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool active = g < p.t.groups;
    uint32_t bits = 0u;
    unsigned long long term = 0ull, behind = 0ull, lagging = 0ull;
    if (active) {
        const int64_t base = p.has_bases != 0 ? p.t.ibase[g] : 0;
        const int64_t d = p.deadline[g];
        Group g64;
        load_group(p.t, g, g64);
        const bool leader = g64.role == RG_LEADER, follower = g64.role == RG_FOLLOWER, has_log = g64.rc > 0, prepared = g64.prepared, ready = leader && prepared;
        const uint32_t pend = g64.pending & ((1u << p.followers) - 1u);
        const int64_t last = g64.last, back = wsub(last, g64.commit);
        // the image the 32-bit body would start from (narrow_body)
        g64.s1 = g64.rc > 1 ? g64.s1 : 0; g64.s2 = g64.rc > 2 ? g64.s2 : 0; g64.s3 = g64.rc > 3 ? g64.s3 : 0;
        const Group rel = group_to_rel(g64, base);
        int64_t lag;
        const bool peers_fit = peers_in_image(p.t, g, prepared, p.followers, base, last, lag);
        const bool in_image = fits32(rel, EV_LIMIT) && small_fields_fit(rel) && (base == 0 || rel.epoch_index > 0) && base >= 0 && peers_fit;
        bits = (follower ? RG_SCAN_FOLLOWER : 0u) | (g64.role == RG_CANDIDATE ? RG_SCAN_CANDIDATE : 0u) | (leader ? RG_SCAN_LEADER : 0u) |
               ((follower && g64.leader == RG_NO_NODE) ? RG_SCAN_NO_LEADER : 0u) | (g64.td ? RG_SCAN_TIMEOUT_DETECTED : 0u) |
               (!has_log ? RG_SCAN_EMPTY_LOG : 0u) | (g64.rc == K ? RG_SCAN_RUNS_FULL : 0u) | ((has_log && back > p.backlog) ? RG_SCAN_BACKLOG : 0u) |
               ((leader && !prepared) ? RG_SCAN_UNPREPARED : 0u) | ((ready && pend != 0u) ? RG_SCAN_PENDING_INSTALL : 0u) |
               ((ready && has_log && lag > p.lag) ? RG_SCAN_LAGGING : 0u) | (!in_image ? RG_SCAN_OFF_IMAGE : 0u) | (base != 0 ? RG_SCAN_HAS_BASE : 0u) |
               (d == 0 ? RG_SCAN_NO_TICKET : 0u) | (d == -1 ? RG_SCAN_TICKET_FIRED : 0u) | ((d > 0 && d <= p.now) ? RG_SCAN_OVERDUE : 0u);
        term = (unsigned long long)g64.term;
        behind = (has_log && back > 0) ? (unsigned long long)back : 0ull;
        lagging = (ready && has_log && lag > 0) ? (unsigned long long)lag : 0ull;
        if (p.bits) p.bits[g] = bits;
    }
    const bool chosen = active & ((p.any == 0u) | ((bits & p.any) != 0u)) & ((bits & p.all) == p.all) & ((bits & p.none) == 0u);
    const unsigned long long ms = __ballot(chosen);
    // (one lane per word of the wavefront's partial summary: lane b < 16 keeps the count of bit b)
    unsigned long long mine = 0ull;
#pragma unroll
    for (uint32_t b = 0; b < 16u; b++) {
        const unsigned long long m = __ballot((bits >> b) & 1u);
        mine = lane == b ? (unsigned long long)__popcll(m) : mine;
    }
    const unsigned long long top_term = scan_wave_max(term), top_behind = scan_wave_max(behind), sum_behind = scan_wave_sum(behind), top_lag = scan_wave_max(lagging);
    mine = lane == 17u ? top_term : (lane == 18u ? top_behind : (lane == 19u ? sum_behind : (lane == 20u ? top_lag : mine)));
    if (lane == 0u) { const uint32_t w = blockIdx.x * 4u + wave; p.wc[w] = (uint32_t)__popcll(ms); p.sel[w] = ms; }
    if (lane < SCAN_WORDS) fold[wave][lane] = mine;
    __syncthreads();
    if (threadIdx.x < SCAN_WORDS) {
        const uint32_t k = threadIdx.x;
        const bool is_max = (k == 17u) | (k == 18u) | (k == 20u);
        unsigned long long v = fold[0][k];
#pragma unroll
        for (uint32_t w = 1; w < 4u; w++) { const unsigned long long o = fold[w][k]; v = is_max ? (o > v ? o : v) : v + o; }
        p.part[(size_t)blockIdx.x * SCAN_WORDS + k] = v;
    }
}

__global__ __launch_bounds__(1024) void scan_summary_kernel(const ScanParams p, uint32_t blocks, uint32_t waves)
{
    __shared__ unsigned long long fold[SCAN_SLICES][32];
    const uint32_t k = threadIdx.x & 31u, slice = threadIdx.x >> 5;
    const bool is_max = (k == 17u) | (k == 18u) | (k == 20u);
    unsigned long long v = 0ull;
    if (k < SCAN_WORDS) {
        for (uint32_t b = slice; b < blocks; b += SCAN_SLICES) { const unsigned long long o = p.part[(size_t)b * SCAN_WORDS + k]; v = is_max ? (o > v ? o : v) : v + o; }
    }
    fold[slice][k] = v;
    __syncthreads();
    if (threadIdx.x < SCAN_WORDS) {
        v = fold[0][k];
        for (uint32_t s = 1; s < SCAN_SLICES; s++) { const unsigned long long o = fold[s][k]; v = is_max ? (o > v ? o : v) : v + o; }
        p.summary[k] = k == 16u ? (unsigned long long)p.wc[waves] : (k > 20u ? 0ull : v);
    }
}

__global__ __launch_bounds__(256) void scan_emit_kernel(const ScanParams p)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, w = g >> 6;
    const unsigned long long ms = p.sel[w];
    if (!((ms >> lane) & 1ull)) return;
    const uint32_t pos = p.wc[w] + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull));
    if (pos < p.list_cap) p.list[pos] = g;
}

hipError_t launch_scan(const ScanParams &p, hipStream_t s)
{
    const uint32_t blocks = (p.t.groups + 255u) / 256u, waves = blocks * 4u;
    hipLaunchKernelGGL(scan_class_kernel, dim3(blocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.wc, waves, p.wc + waves);
    hipLaunchKernelGGL(scan_summary_kernel, dim3(1), dim3(1024), 0, s, p, blocks, waves);
    if (p.list != nullptr && p.list_cap != 0u) hipLaunchKernelGGL(scan_emit_kernel, dim3(blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

// column c of the table for the image: where its element of group 0 lies (workgroup-uniform: c comes from blockIdx)
__device__ __forceinline__ I32x4 *state_column(const DevTable &t, uint32_t c, uint32_t followers)
{
    const size_t G = t.groups;
    I32x4 *col = reinterpret_cast<I32x4 *>(t.term_commit);
    col = c == 1u ? reinterpret_cast<I32x4 *>(t.epoch) : col;
    col = c == 2u ? reinterpret_cast<I32x4 *>(t.window) : col;
    col = c == 3u ? reinterpret_cast<I32x4 *>(t.ident) : col;
    col = c == 4u ? reinterpret_cast<I32x4 *>(t.elect) : col;
    col = c >= 5u ? reinterpret_cast<I32x4 *>(t.runs) + (size_t)(c - 5u) * G : col;
    col = c >= 5u + (uint32_t)K ? reinterpret_cast<I32x4 *>(t.peer_en) + (size_t)(c - 5u - (uint32_t)K) * G : col;
    col = c >= 5u + (uint32_t)K + followers ? reinterpret_cast<I32x4 *>(t.peer_m) + (size_t)(c - 5u - (uint32_t)K - followers) * G : col;
    return col;
}

__global__ __launch_bounds__(256) void state_gather_kernel(const StateListParams p, uint32_t bpc)
{
    const uint32_t c = blockIdx.x / bpc, i = (blockIdx.x % bpc) * 256u + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t g = p.gid[i];
    if (g >= p.t.groups) return;                                  // (the host refused such a list: never a load outside the table)
    p.image[(size_t)c * p.n + i] = state_column(p.t, c, p.followers)[g];
}

__global__ __launch_bounds__(256) void state_scatter_kernel(const StateListParams p, uint32_t bpc)
{
    const uint32_t c = blockIdx.x / bpc, i = (blockIdx.x % bpc) * 256u + threadIdx.x, columns = 5u + (uint32_t)K + 2u * p.followers;
    if (i >= p.n) return;
    const uint32_t g = p.gid[i];
    if (g >= p.t.groups) return;
    if (c < columns) {
        state_column(p.t, c, p.followers)[g] = p.image[(size_t)c * p.n + i];
        return;
    }
    // what rg_load_state leaves beside the state: no timer ticket, the timers' role epoch (ident: column 3, .z), fresh health statistics, nothing in flight
    const size_t G = p.t.groups;
    p.deadline[g] = 0;
    p.timer_epoch[g] = (uint32_t)p.image[(size_t)3 * p.n + i].z;
    for (uint32_t j = 0; j < p.followers; j++) {
        p.ok[j * G + g] = 0; p.fail[j * G + g] = 0; p.recent[j * G + g] = 0;
        if (p.in_flight) p.in_flight[j * G + g] = 0;
    }
}

hipError_t launch_state_gather(const StateListParams &p, hipStream_t s)
{
    if (p.n == 0u) return hipSuccess;
    const uint32_t bpc = (p.n + 255u) / 256u;
    hipLaunchKernelGGL(state_gather_kernel, dim3(bpc * state_list_columns(p.followers)), dim3(256), 0, s, p, bpc);
    return hipGetLastError();
}
hipError_t launch_state_scatter(const StateListParams &p, hipStream_t s)
{
    if (p.n == 0u) return hipSuccess;
    const uint32_t bpc = (p.n + 255u) / 256u;
    hipLaunchKernelGGL(state_scatter_kernel, dim3(bpc * (state_list_columns(p.followers) + 1u)), dim3(256), 0, s, p, bpc);
    return hipGetLastError();
}

#endif  // RG_SCAN_KERNELS

}  // namespace rg
