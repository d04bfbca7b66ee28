// rg_effects.hpp — what a launch asks a host to DO, as lists, on the device (rg_effects32, include/raftgpu.h): the log writes, the commit advances and the
// cells that need the host, of the compact outcome rows row[D][C] that rg_submit32c*, or a tick, left behind.
//
// n and R are read from the batch's count / rounds as the tick reads them (a NULL word: C / D). Every grid is one-dimensional and sized from C and D. Two domains
// share each kernel, a wavefront w = blockIdx * 4 + wave taking its share of both:
//   - the CELLS, flat: wavefront w < Wc covers the `cspan` consecutive cells from w * cspan on, 64 at a time — consecutive cells are consecutive rows of one round,
//     so the loads are coalesced over i. It leaves at once when its first cell lies at or beyond R * C; a cell whose row lies at or beyond n is not loaded.
//     Ascending w is ascending cell, so one count per wavefront, one prefix sum over the wavefronts (timers_scan_kernel) and a running offset +
//     popcount(ballot below the lane) inside the wavefront give log_list and attention in ascending cell order — the scheme of timers_count / _scan / _emit and of
//     the route — with no atomic anywhere.
//   - the ROWS: wavefront w < Wr covers the `rspan` consecutive rows from w * rspan on, 64 at a time, one lane per row. A lane walks r = 0 .. R - 1 of its row —
//     coalesced over i again — and keeps the LAST round whose flags carry RG_F_COMMIT; the same scheme over the rows gives commit_list in ascending row order. The
//     emit pass loads the 16 bytes of that one cell for commit_index and flags verbatim.
// The spans are chosen per shape (effects_span): 64 while the count arrays, a word per wavefront, stay within EFFECTS_SCAN_WORDS, and doubled until they do, because
// ONE workgroup scans each of them. Every loop is bounded by R or by a span. Five launches, none of which waits for another workgroup:
//   1. effects_count_kernel     per wavefront: lc[w], ac[w] (cells with a log write / with RG_NEED_HOST), cc[w] (rows with a commit)
//   2. timers_scan_kernel x 3   the three count arrays into offsets, their sums behind them
//   3. effects_emit_kernel      per wavefront: the items below their capacities; one lane writes counts
// A pass reads the flags of a cell once per domain: the rows are read twice per pass, four times per call.
#pragma once

#include "rg_device.hpp"

namespace rg {

constexpr uint32_t EFFECTS_SPAN_MIN = 64;           // cells (rows) a wavefront covers, 64 at a time (EffectsParams::cspan / rspan, powers of two)
constexpr uint32_t EFFECTS_SCAN_WORDS = 4096;       // ... chosen so that a count array, a word per wavefront, stays at or below this: one workgroup scans it

struct EffectsParams {
    uint32_t C, D;
    const uint32_t *gid, *count, *rounds;           // nullptr: row i is group i / n = C / R = D
    const I32x4 *row;                               // rg_out32_t, [D][C]
    U32x2 *log_list, *attention;                    // rg_route_item_t
    I32x4 *commit_list;                             // rg_commit_item_t
    uint32_t log_cap, commit_cap, attention_cap;
    uint32_t *counts;                               // [4]
    // scratch (the table's)
    uint32_t cspan, rspan, Wc, Wr;                  // effects_span(); wavefronts of the two domains: ceil(D * C / cspan), ceil(C / rspan)
    uint32_t *lc, *ac;                              // [Wc + 1] per-wavefront counts of log / attention cells -> offsets, last = their sum
    uint32_t *cc;                                   // [Wr + 1] the same for the rows with a commit
};

hipError_t launch_effects(const EffectsParams &p, hipStream_t s);

// the span of a domain of `items` cells (rows): the smallest that keeps its count array — ceil(items / span) words — within EFFECTS_SCAN_WORDS (items < 2^32: at most 2^20)
inline uint32_t effects_span(uint64_t items)
{
    uint32_t span = EFFECTS_SPAN_MIN;
    while ((items + span - 1) / span > EFFECTS_SCAN_WORDS) span *= 2;
    return span;
}

#ifdef RG_EFFECTS_KERNELS

struct EffectsRun { uint32_t n, R; };

__device__ __forceinline__ EffectsRun effects_run(const EffectsParams &p)
{
    EffectsRun u;
    u.n = p.C; u.R = p.D;
    if (p.count) { const uint32_t c = *p.count; u.n = c < p.C ? c : p.C; }
    if (p.rounds) { const uint32_t d = *p.rounds; u.R = d < 1u ? 1u : (d < p.D ? d : p.D); }
    return u;
}

__device__ __forceinline__ bool effects_is_log(uint32_t flags) { return (flags & (RG_F_LOG_APPEND | RG_F_LOG_TRUNC)) != 0u; }
__device__ __forceinline__ bool effects_is_attention(uint32_t flags) { return RG_F_STATUS(flags) == (uint32_t)RG_NEED_HOST; }

// the flags of cell first + lane of the flat domain, 0 for a cell at or beyond `end` (= R * C) or whose row lies at or beyond n; `at` = the cell
__device__ __forceinline__ uint32_t effects_cell_flags(const EffectsParams &p, const EffectsRun &u, uint64_t first, uint64_t end, uint32_t lane, uint32_t &at)
{
    const uint64_t c = first + lane;
    at = (uint32_t)c;
    if (c >= end) return 0u;
    const uint32_t i = at % p.C;
    return i < u.n ? (uint32_t)p.row[at].y : 0u;
}

// row i of the row domain: has it a round r < R with RG_F_COMMIT — `last` = the cell of the last such round
__device__ __forceinline__ bool effects_row_commit(const EffectsParams &p, const EffectsRun &u, uint64_t i, uint32_t &last)
{
    bool has = false;
    last = 0u;
    if (i >= u.n) return false;
#pragma unroll 4
    for (uint32_t r = 0u; r < u.R; r++) {
        const uint32_t at = r * p.C + (uint32_t)i;
        if ((uint32_t)p.row[at].y & RG_F_COMMIT) { has = true; last = at; }
    }
    return has;
}

__global__ __launch_bounds__(256) void effects_count_kernel(const EffectsParams p)
{
    const EffectsRun u = effects_run(p);
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w < p.Wc) {
        const uint64_t end = (uint64_t)u.R * p.C, c0 = (uint64_t)w * p.cspan;
        uint32_t nl = 0u, na = 0u;
        for (uint32_t k0 = 0u; k0 < p.cspan && c0 + k0 < end; k0 += 64u) {          // (per wavefront)
            uint32_t at;
            const uint32_t flags = effects_cell_flags(p, u, c0 + k0, end, lane, at);
            nl += (uint32_t)__popcll(__ballot(effects_is_log(flags)));
            na += (uint32_t)__popcll(__ballot(effects_is_attention(flags)));
        }
        if (lane == 0u) { p.lc[w] = nl; p.ac[w] = na; }
    }
    if (w < p.Wr) {
        const uint64_t i0 = (uint64_t)w * p.rspan;
        uint32_t nc = 0u;
        for (uint32_t k0 = 0u; k0 < p.rspan && i0 + k0 < u.n; k0 += 64u) {          // (per wavefront)
            uint32_t last;
            nc += (uint32_t)__popcll(__ballot(effects_row_commit(p, u, i0 + k0 + lane, last)));
        }
        if (lane == 0u) p.cc[w] = nc;
    }
}

__global__ __launch_bounds__(256) void effects_emit_kernel(const EffectsParams p)
{
    const EffectsRun u = effects_run(p);
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (blockIdx.x == 0u && threadIdx.x == 0u) { p.counts[0] = p.lc[p.Wc]; p.counts[1] = p.cc[p.Wr]; p.counts[2] = p.ac[p.Wc]; p.counts[3] = 0u; }
    if (w < p.Wc) {
        const uint64_t end = (uint64_t)u.R * p.C, c0 = (uint64_t)w * p.cspan;
        uint32_t bl = p.lc[w], ba = p.ac[w];            // where the wavefront's next items go
        for (uint32_t k0 = 0u; k0 < p.cspan && c0 + k0 < end; k0 += 64u) {
            uint32_t at;
            const uint32_t flags = effects_cell_flags(p, u, c0 + k0, end, lane, at);
            const bool hl = effects_is_log(flags), ha = effects_is_attention(flags);
            const unsigned long long ml = __ballot(hl), ma = __ballot(ha);
            if (hl || ha) {
                const uint32_t i = at % p.C;
                const U32x2 item{at, p.gid ? p.gid[i] : i};
                const uint32_t pl = bl + (uint32_t)__popcll(ml & below), pa = ba + (uint32_t)__popcll(ma & below);
                if (hl && pl < p.log_cap) p.log_list[pl] = item;
                if (ha && pa < p.attention_cap) p.attention[pa] = item;
            }
            bl += (uint32_t)__popcll(ml);
            ba += (uint32_t)__popcll(ma);
        }
    }
    if (w < p.Wr) {
        const uint64_t i0 = (uint64_t)w * p.rspan;
        uint32_t bc = p.cc[w];
        for (uint32_t k0 = 0u; k0 < p.rspan && i0 + k0 < u.n; k0 += 64u) {
            const uint32_t i = (uint32_t)(i0 + k0 + lane);
            uint32_t last;
            const bool hc = effects_row_commit(p, u, i0 + k0 + lane, last);
            const unsigned long long mc = __ballot(hc);
            const uint32_t pc = bc + (uint32_t)__popcll(mc & below);
            if (hc && pc < p.commit_cap) {
                const I32x4 v = p.row[last];
                p.commit_list[pc] = I32x4{(int32_t)last, (int32_t)(p.gid ? p.gid[i] : i), v.z, v.y};
            }
            bc += (uint32_t)__popcll(mc);
        }
    }
}

hipError_t launch_effects(const EffectsParams &p, hipStream_t s)
{
    const uint32_t waves = p.Wc > p.Wr ? p.Wc : p.Wr, blocks = (waves + 3u) / 4u;
    hipLaunchKernelGGL(effects_count_kernel, dim3(blocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.lc, p.Wc, p.lc + p.Wc);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.ac, p.Wc, p.ac + p.Wc);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.cc, p.Wr, p.cc + p.Wr);
    hipLaunchKernelGGL(effects_emit_kernel, dim3(blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

#endif  // RG_EFFECTS_KERNELS

}  // namespace rg
