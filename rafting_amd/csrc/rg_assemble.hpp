// rg_assemble.hpp — arrival-ordered events into the [round][row] columns of a sparse-rounds batch, on the device (rg_assemble32, include/raftgpu.h).
//
// The sequence S of a run: the fired tickets a tick listed (e of them, position j, id 0x80000000 | j), then the arrival log (m events, position e + k, id k).
// Every kernel reads e and m from device memory when it runs (asm_run); every grid is sized from the CAPACITIES and its surplus lanes leave at once. A
// position is the sort key everywhere: positions are distinct, so "the rank of an event among its group's events" is a function of the inputs alone, whatever
// order the atomics below were served in. Ten launches, none of which waits for another workgroup:
//   1. asm_mark_kernel      per position: count the event in cnt[gid]; the first event of a group sets the group's bit in a bitmap (atomicAdd of a bit nobody
//                           else adds); a gid at or above the group count is counted as bad and takes no further part
//   2. asm_words_kernel     per 64-bit word of the bitmap: its popcount; timers_scan_kernel makes them offsets (the scheme of timers_count / _scan / _emit, over
//                           groups / 64 words), the sum is |U|
//   3. asm_rows_kernel      per group (a wavefront per word, gone at once where the word is 0): row = offset + popcount(bits below) — the ascending list. A listed
//                           group (row < C) writes gid[row], takes cnt[gid] positions of the segment pool (one atomicAdd per wavefront: where a segment lies is not
//                           an output) and notes its depth min(cnt, D) in a mark array; cnt[gid] goes back to 0 for step 4
//   4. asm_claim_kernel     per position: a slot in its group's segment (atomicAdd on cnt[gid] again) holds the position; an event of a group beyond the list is
//                           flagged deferred. One lane turns the depth marks into R
//   5. asm_order_kernel     per row: rank every position of its segment by counting the smaller ones; rank < D -> cell (rank, row), else flagged deferred; then the
//                           RG_EV_NONE fill up to R. A row with more than ASM_SMALL events is queued for step 6 instead (any D: its D smallest must be found)
//   6. asm_big_rows_kernel  a workgroup per queued row: the D-th smallest position by an 8-bit radix select over an LDS histogram (4 passes over the segment),
//                           the D positions at or below it ranked in LDS, the rest flagged
//   7. asm_defer_count / timers_scan_kernel / asm_defer_emit: the flagged positions compacted in S order; the last kernel also writes stats and puts back what the
//                           run touched of the scratch: cnt and the bitmap word of every event's group, the scalars — and remembers e and m for rg_route32. The cost of a run follows m + e and groups / 64
//                           (steps 2, 3), never groups x anything.
//
// THE CARRY (rg_assembler_carry_enable; off: everything above, unchanged). A carrying assembler owns two carries of carry_cap complete rows (gid, head, abcd) and a
// count each. A run reads one of them as a THIRD source, between the other two — S = the e fired tickets, the q carried slots (position e + c, id 0x40000000 | c),
// the m arrivals (position e + q + k) — and leaves the events it deferred, in S order, in the other: which is which is the host's call counter, q is read on the
// device. The carrying run is the same ten launches over kernels of its own (asm_*_carry_kernel: the bodies below with the third source compiled in; the plain
// kernels are the bodies with it compiled out) and an eleventh:
//   8. asm_carry_gather_kernel  per position: a deferred event — the p-th of the run's deferred sequence, what deferred[p] names — is stored as a complete row in slot
//                           p of the other carry while p < carry_cap (a fired ticket as the RG_EV_TIMEOUT row asm_put would have made of it); one lane writes that
//                           carry's count. It also leaves rg_route32_carry, per position, where the event went (`where`: 0x80000000 | slot, 0xFFFFFFFE for one
//                           the carry had no room for, 0xFFFFFFFF for any other event that is not a carried one; the cell of a carried event that was placed is
//                           stored by asm_put).
#pragma once

#include "rg_device.hpp"

namespace rg {

constexpr uint32_t ASM_SMALL = 64;              // a row with at most this many events is ordered by one lane (<= 64 x 64 cached loads)
constexpr uint32_t ASM_BIG_BLOCKS = 256;        // workgroups that share the rows with more
constexpr uint32_t ASM_POOL = 0, ASM_N_BIG = 1, ASM_BAD = 2, ASM_MARK = 3, ASM_SCALARS = ASM_MARK + 65, ASM_LAST = ASM_SCALARS;     // the scratch words `scalars`
constexpr uint32_t ASM_EXPIRED_ID = 0x80000000u, ASM_NO_EVENT = 0xFFFFFFFFu;
constexpr uint32_t ASM_CARRIED_ID = 0x40000000u;  // RG_ASM_CARRIED
constexpr uint32_t ASM_WENT_CARRIED = 0x80000000u, ASM_WENT_SPILLED = 0xFFFFFFFEu, ASM_WENT_NOWHERE = 0xFFFFFFFFu;   // `where`: RG_ROUTE_CARRIED, RG_ROUTE_SPILLED, RG_ROUTE_NONE

struct AsmParams {
    // the arrival log and the optional list of fired tickets (rg_arrivals_t)
    const uint32_t *in_count, *in_gid;
    const U32x2 *in_head;
    const I32x4 *in_abcd;
    const uint32_t *ex_gid, *ex_epoch, *ex_count;   // ex_count == nullptr: no second source
    uint32_t in_cap, ex_cap;
    // the batch (rg_assembled_t)
    uint32_t C, D;
    uint32_t *gid, *count, *rounds, *origin, *deferred, *stats;
    U32x2 *head;
    I32x4 *abcd;
    uint32_t deferred_cap;
    // the table and the assembler's scratch
    uint32_t groups, words;                         // words = ceil(groups / 64)
    uint32_t *cnt;                                  // [groups] events per group; 0 between runs
    unsigned long long *bitmap;                     // [words] groups with an event; 0 between runs
    uint32_t *rowof;                                // [groups] row of a group with an event (>= C: beyond the list); meaningful for this run's groups only
    uint32_t *wordoff;                              // [words + 1] popcounts -> offsets, last = |U|
    uint32_t *rowcnt, *segoff;                      // [rows_cap] events and segment start of a listed row
    uint32_t *seg;                                  // [seg_cap] the positions, grouped by row, in the order they were claimed
    uint8_t *flag;                                  // [seg_cap] per position: 1 = deferred
    uint32_t *dcounts;                              // [4 * event workgroups + 1] per-wavefront counts of deferred positions -> offsets, last = their sum
    uint32_t *big;                                  // [big_cap] rows with more than ASM_SMALL events
    uint32_t *scalars;                              // [ASM_SCALARS] 0 between runs, + [ASM_LAST .. ASM_LAST + 3) the e, m and q the last run read, kept for rg_route32 (rg_route.hpp)
    uint32_t rows_cap, seg_cap, big_cap;
    // the carry (cr_count == nullptr: an assembler without one, and the plain kernels, which never read these)
    uint32_t carry_cap;
    const uint32_t *cr_count, *cr_gid;              // the carry this run reads: [1] = q, [carry_cap] rows
    const U32x2 *cr_head;
    const I32x4 *cr_abcd;
    uint32_t *cw_count, *cw_gid;                    // the carry it leaves
    U32x2 *cw_head;
    I32x4 *cw_abcd;
    uint32_t *where;                                // [seg_cap] per position: where the event went, for rg_route32_carry (asm_carry_gather_kernel)
};

hipError_t launch_assemble(const AsmParams &p, hipStream_t s);

#ifdef RG_ASSEMBLE_KERNELS

// K: the third source, the carry, is compiled in (the kernels of a carrying run) or out (q = 0 at compile time: the plain kernels)
struct AsmRun { uint32_t e, q, m, T; };

template <bool K>
__device__ __forceinline__ AsmRun asm_run(const AsmParams &p)
{
    AsmRun r;
    r.e = 0;
    if (p.ex_count) {
        const uint32_t c = *p.ex_count;             // 0xFFFFFFFF: the tick's look-back ran into its bound, the list is not to be trusted (tick_fold_kernel)
        r.e = c == 0xFFFFFFFFu ? 0u : (c < p.ex_cap ? c : p.ex_cap);
    }
    r.q = 0;
    if constexpr (K) {
        const uint32_t c = *p.cr_count;
        r.q = c < p.carry_cap ? c : p.carry_cap;
    }
    const uint32_t c = *p.in_count;
    r.m = c < p.in_cap ? c : p.in_cap;
    r.T = r.e + r.q + r.m;
    return r;
}
template <bool K>
__device__ __forceinline__ uint32_t asm_gid(const AsmParams &p, const AsmRun &r, uint32_t s)
{
    if (s < r.e) return p.ex_gid[s];
    if constexpr (K) { if (s - r.e < r.q) return p.cr_gid[s - r.e]; }
    return p.in_gid[s - r.e - r.q];
}
template <bool K>
__device__ __forceinline__ uint32_t asm_id(const AsmRun &r, uint32_t s)
{
    if (s < r.e) return ASM_EXPIRED_ID | s;
    if constexpr (K) { if (s - r.e < r.q) return ASM_CARRIED_ID | (s - r.e); }
    return s - r.e - r.q;
}

// the event at position s into cell (round, row): a fired ticket becomes its fenced RG_EV_TIMEOUT row, a carried slot and an arrival move verbatim (8-byte and
// 16-byte accesses); a carried slot leaves the route its cell
template <bool K>
__device__ __forceinline__ void asm_put(const AsmParams &p, const AsmRun &r, uint32_t round, uint32_t row, uint32_t s)
{
    const size_t cell = (size_t)round * p.C + row;
    if (s < r.e) {
        p.head[cell] = U32x2{RG_HDR_MAKE(RG_EV_TIMEOUT, 0, 0, 0), p.ex_epoch[s]};
        p.abcd[cell] = I32x4{0, 0, 0, 0};
    } else if (K && s - r.e < r.q) {
        p.head[cell] = p.cr_head[s - r.e];
        p.abcd[cell] = p.cr_abcd[s - r.e];
        p.where[s] = (uint32_t)cell;
    } else {
        p.head[cell] = p.in_head[s - r.e - r.q];
        p.abcd[cell] = p.in_abcd[s - r.e - r.q];
    }
    p.origin[cell] = asm_id<K>(r, s);
}

template <bool K>
__device__ __forceinline__ void asm_mark_body(const AsmParams &p)
{
    const AsmRun r = asm_run<K>(p);
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const bool live = s < r.T;
    const uint32_t g = live ? asm_gid<K>(p, r, s) : 0u;
    const bool bad = live && g >= p.groups;
    const unsigned long long mb = __ballot(bad);
    if (mb != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(&p.scalars[ASM_BAD], (uint32_t)__popcll(mb));
    if (!live) return;
    p.flag[s] = 0;
    if (bad) return;
    if (atomicAdd(&p.cnt[g], 1u) == 0u) atomicAdd(&p.bitmap[g >> 6], 1ull << (g & 63u));
}
__global__ __launch_bounds__(256) void asm_mark_kernel(const AsmParams p) { asm_mark_body<false>(p); }
__global__ __launch_bounds__(256) void asm_mark_carry_kernel(const AsmParams p) { asm_mark_body<true>(p); }

__global__ __launch_bounds__(256) void asm_words_kernel(const AsmParams p)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < p.words) p.wordoff[w] = (uint32_t)__popcll(p.bitmap[w]);
}

__global__ __launch_bounds__(256) void asm_rows_kernel(const AsmParams p)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, w = g >> 6, lane = threadIdx.x & 63u;
    if (g == 0u) { const uint32_t u = p.wordoff[p.words]; *p.count = u < p.C ? u : p.C; }
    if (w >= p.words) return;                       // (per wavefront)
    const unsigned long long word = p.bitmap[w];
    if (word == 0ull) return;                       // (per wavefront)
    const bool marked = ((word >> lane) & 1ull) != 0ull;
    const uint32_t row = p.wordoff[w] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
    const bool listed = marked && row < p.C;
    uint32_t c = 0;
    if (marked) { c = p.cnt[g]; p.cnt[g] = 0u; p.rowof[g] = row; }
    if (!listed) c = 0u;
    uint32_t total = c, before = 0u, deep = c < p.D ? c : p.D;      // butterfly: the wavefront's sum, the sum of the lanes below, the greatest depth
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_xor(total, d, 64), x = __shfl_xor(deep, d, 64);
        if (lane & (uint32_t)d) before += t;
        total += t;
        deep = x > deep ? x : deep;
    }
    uint32_t base = 0u;
    if (lane == 0u && total != 0u) base = atomicAdd(&p.scalars[ASM_POOL], total);
    for (int d = 1; d < 64; d <<= 1) base += __shfl_xor(base, d, 64);      // (every other lane holds 0: all lanes get lane 0's)
    if (lane == 0u) p.scalars[ASM_MARK + deep] = 1u;
    if (listed && row < p.rows_cap) { p.gid[row] = g; p.rowcnt[row] = c; p.segoff[row] = base + before; }
}

template <bool K>
__device__ __forceinline__ void asm_claim_body(const AsmParams &p)
{
    const AsmRun r = asm_run<K>(p);
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s == 0u) {
        uint32_t R = 1u;
        for (uint32_t d = 2u; d <= p.D; d++) R = p.scalars[ASM_MARK + d] != 0u ? d : R;
        *p.rounds = R;
    }
    if (s >= r.T) return;
    const uint32_t g = asm_gid<K>(p, r, s);
    if (g >= p.groups) return;
    const uint32_t row = p.rowof[g];
    if (row >= p.C || row >= p.rows_cap) { p.flag[s] = 1; return; }
    const uint32_t at = p.segoff[row] + atomicAdd(&p.cnt[g], 1u);
    if (at < p.seg_cap) p.seg[at] = s;
}
__global__ __launch_bounds__(256) void asm_claim_kernel(const AsmParams p) { asm_claim_body<false>(p); }
__global__ __launch_bounds__(256) void asm_claim_carry_kernel(const AsmParams p) { asm_claim_body<true>(p); }

template <bool K>
__device__ __forceinline__ void asm_order_body(const AsmParams &p)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = *p.count, R = *p.rounds;
    if (i >= n) return;
    const AsmRun r = asm_run<K>(p);
    const uint32_t c = p.rowcnt[i], off = p.segoff[i];
    if (c > ASM_SMALL) {
        const uint32_t at = atomicAdd(&p.scalars[ASM_N_BIG], 1u);
        if (at < p.big_cap) p.big[at] = i;
        return;                                     // (it uses all D rounds, and D >= R)
    }
    for (uint32_t q = 0; q < c; q++) {
        const uint32_t key = p.seg[off + q];
        if (key >= r.T) continue;                   // (cannot happen while the sources stand still during a run; a caller that breaks that gets wrong rows, not wild stores)
        uint32_t rank = 0;
        for (uint32_t k = 0; k < c; k++) rank += p.seg[off + k] < key ? 1u : 0u;
        if (rank < p.D) asm_put<K>(p, r, rank, i, key); else p.flag[key] = 1;
    }
    for (uint32_t q = c < p.D ? c : p.D; q < R; q++) {
        const size_t cell = (size_t)q * p.C + i;
        p.head[cell] = U32x2{0u, 0u};
        p.abcd[cell] = I32x4{0, 0, 0, 0};
        p.origin[cell] = ASM_NO_EVENT;
    }
}
__global__ __launch_bounds__(256) void asm_order_kernel(const AsmParams p) { asm_order_body<false>(p); }
__global__ __launch_bounds__(256) void asm_order_carry_kernel(const AsmParams p) { asm_order_body<true>(p); }

template <bool K>
__device__ __forceinline__ void asm_big_rows_body(const AsmParams &p)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[64];
    __shared__ uint32_t st[3];                      // the prefix of the D-th smallest position found so far, how many-th it is among those that share it, positions selected
    const AsmRun r = asm_run<K>(p);
    const uint32_t tid = threadIdx.x;
    uint32_t rows = p.scalars[ASM_N_BIG];
    rows = rows < p.big_cap ? rows : p.big_cap;
    for (uint32_t at = blockIdx.x; at < rows; at += gridDim.x) {
        const uint32_t i = p.big[at], c = p.rowcnt[i], off = p.segoff[i];
        if (tid == 0u) { st[0] = 0u; st[1] = p.D; st[2] = 0u; }
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0u;
            __syncthreads();
            const uint32_t prefix = st[0], above = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
            for (uint32_t j = tid; j < c; j += 256u) {
                const uint32_t key = p.seg[off + j];
                if ((key & above) == (prefix & above)) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0u) {
                const uint32_t want = st[1];
                uint32_t cum = 0u, b = 0u;
                for (; b < 255u; b++) {
                    if (cum + hist[b] >= want) break;
                    cum += hist[b];
                }
                st[0] = prefix | (b << shift);
                st[1] = want - cum;
            }
            __syncthreads();
        }
        const uint32_t last = st[0];                // the D-th smallest position of the row: exactly D lie at or below it
        for (uint32_t j = tid; j < c; j += 256u) {
            const uint32_t key = p.seg[off + j];
            if (key >= r.T) continue;
            if (key <= last) {
                const uint32_t k = atomicAdd(&st[2], 1u);
                if (k < 64u) sel[k] = key;
            } else {
                p.flag[key] = 1;
            }
        }
        __syncthreads();
        if (tid < p.D) {
            const uint32_t key = sel[tid];
            uint32_t rank = 0;
            for (uint32_t k = 0; k < p.D; k++) rank += sel[k] < key ? 1u : 0u;
            if (key < r.T && tid < st[2]) asm_put<K>(p, r, rank, i, key);
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void asm_big_rows_kernel(const AsmParams p) { asm_big_rows_body<false>(p); }
__global__ __launch_bounds__(256) void asm_big_rows_carry_kernel(const AsmParams p) { asm_big_rows_body<true>(p); }

template <bool K>
__device__ __forceinline__ void asm_defer_count_body(const AsmParams &p)
{
    const AsmRun r = asm_run<K>(p);
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const unsigned long long m = __ballot(s < r.T && p.flag[s] != 0);
    if ((threadIdx.x & 63u) == 0u) p.dcounts[s >> 6] = (uint32_t)__popcll(m);
}
__global__ __launch_bounds__(256) void asm_defer_count_kernel(const AsmParams p) { asm_defer_count_body<false>(p); }
__global__ __launch_bounds__(256) void asm_defer_count_carry_kernel(const AsmParams p) { asm_defer_count_body<true>(p); }

template <bool K>
__device__ __forceinline__ void asm_defer_emit_body(const AsmParams &p)
{
    const AsmRun r = asm_run<K>(p);
    const uint32_t s = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = s < r.T;
    const bool def = live && p.flag[s] != 0;
    const unsigned long long m = __ballot(def);
    if (def) {
        const uint32_t pos = p.dcounts[s >> 6] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (pos < p.deferred_cap) p.deferred[pos] = asm_id<K>(r, s);
    }
    if (s == 0u) {
        const uint32_t deferred = p.dcounts[gridDim.x * 4u], bad = p.scalars[ASM_BAD];
        p.stats[0] = r.T - bad - deferred; p.stats[1] = deferred; p.stats[2] = bad; p.stats[3] = 0u;
        for (uint32_t k = 0; k < ASM_SCALARS; k++) p.scalars[k] = 0u;
        p.scalars[ASM_LAST] = r.e; p.scalars[ASM_LAST + 1u] = r.m;
        if constexpr (K) {                          // the spilled events: deferred, and beyond what the next carry holds
            p.stats[3] = deferred > p.carry_cap ? deferred - p.carry_cap : 0u;
            p.scalars[ASM_LAST + 2u] = r.q;
        }
    }
    if (!live) return;
    const uint32_t g = asm_gid<K>(p, r, s);            // the scratch this run touched, back to 0 (every event of a group stores the same)
    if (g < p.groups) { p.cnt[g] = 0u; p.bitmap[g >> 6] = 0ull; }
}
__global__ __launch_bounds__(256) void asm_defer_emit_kernel(const AsmParams p) { asm_defer_emit_body<false>(p); }
__global__ __launch_bounds__(256) void asm_defer_emit_carry_kernel(const AsmParams p) { asm_defer_emit_body<true>(p); }

// the deferred events of a carrying run, in S order, into the carry the next run reads; and where every event of the run went, for rg_route32_carry
__global__ __launch_bounds__(256) void asm_carry_gather_kernel(const AsmParams p)
{
    const AsmRun r = asm_run<true>(p);
    const uint32_t s = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = s < r.T;
    const bool def = live && p.flag[s] != 0;
    const unsigned long long m = __ballot(def);
    if (s == 0u) {
        const uint32_t deferred = p.dcounts[gridDim.x * 4u];
        *p.cw_count = deferred < p.carry_cap ? deferred : p.carry_cap;
    }
    if (!live) return;
    const bool carried = s >= r.e && s - r.e < r.q;
    if (!def) {
        if (!carried) p.where[s] = ASM_WENT_NOWHERE;        // (a placed carried slot: asm_put stored its cell)
        return;
    }
    const uint32_t pos = p.dcounts[s >> 6] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos >= p.carry_cap) { p.where[s] = ASM_WENT_SPILLED; return; }
    p.where[s] = ASM_WENT_CARRIED | pos;
    if (s < r.e) {
        p.cw_gid[pos] = p.ex_gid[s];
        p.cw_head[pos] = U32x2{RG_HDR_MAKE(RG_EV_TIMEOUT, 0, 0, 0), p.ex_epoch[s]};
        p.cw_abcd[pos] = I32x4{0, 0, 0, 0};
    } else if (carried) {
        p.cw_gid[pos] = p.cr_gid[s - r.e];
        p.cw_head[pos] = p.cr_head[s - r.e];
        p.cw_abcd[pos] = p.cr_abcd[s - r.e];
    } else {
        p.cw_gid[pos] = p.in_gid[s - r.e - r.q];
        p.cw_head[pos] = p.in_head[s - r.e - r.q];
        p.cw_abcd[pos] = p.in_abcd[s - r.e - r.q];
    }
}

// a carrying run: the same chain over the kernels that read the third source, and the gather behind it
static hipError_t launch_assemble_carry(const AsmParams &p, hipStream_t s)
{
    const uint32_t events = p.in_cap + p.ex_cap + p.carry_cap;
    const uint32_t eb = events ? (events + 255u) / 256u : 1u;
    hipLaunchKernelGGL(asm_mark_carry_kernel, dim3(eb), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_words_kernel, dim3((p.words + 255u) / 256u), dim3(256), 0, s, p);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.wordoff, p.words, p.wordoff + p.words);
    hipLaunchKernelGGL(asm_rows_kernel, dim3((p.words * 64u + 255u) / 256u), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_claim_carry_kernel, dim3(eb), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_order_carry_kernel, dim3((p.C + 255u) / 256u), dim3(256), 0, s, p);
    const uint32_t big = events / (ASM_SMALL + 1u) + 1u;
    hipLaunchKernelGGL(asm_big_rows_carry_kernel, dim3(big < ASM_BIG_BLOCKS ? big : ASM_BIG_BLOCKS), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_defer_count_carry_kernel, dim3(eb), dim3(256), 0, s, p);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.dcounts, eb * 4u, p.dcounts + eb * 4u);
    hipLaunchKernelGGL(asm_defer_emit_carry_kernel, dim3(eb), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_carry_gather_kernel, dim3(eb), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_assemble(const AsmParams &p, hipStream_t s)
{
    if (p.cr_count) return launch_assemble_carry(p, s);
    const uint32_t events = p.in_cap + p.ex_cap;
    const uint32_t eb = events ? (events + 255u) / 256u : 1u;       // (the grids cover the capacities; one workgroup at least: it writes count, rounds and stats)
    hipLaunchKernelGGL(asm_mark_kernel, dim3(eb), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_words_kernel, dim3((p.words + 255u) / 256u), dim3(256), 0, s, p);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.wordoff, p.words, p.wordoff + p.words);
    hipLaunchKernelGGL(asm_rows_kernel, dim3((p.words * 64u + 255u) / 256u), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_claim_kernel, dim3(eb), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_order_kernel, dim3((p.C + 255u) / 256u), dim3(256), 0, s, p);
    const uint32_t big = events / (ASM_SMALL + 1u) + 1u;            // (more rows than that cannot have more than ASM_SMALL events each)
    hipLaunchKernelGGL(asm_big_rows_kernel, dim3(big < ASM_BIG_BLOCKS ? big : ASM_BIG_BLOCKS), dim3(256), 0, s, p);
    hipLaunchKernelGGL(asm_defer_count_kernel, dim3(eb), dim3(256), 0, s, p);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.dcounts, eb * 4u, p.dcounts + eb * 4u);
    hipLaunchKernelGGL(asm_defer_emit_kernel, dim3(eb), dim3(256), 0, s, p);
    return hipGetLastError();
}

#endif  // RG_ASSEMBLE_KERNELS

}  // namespace rg
