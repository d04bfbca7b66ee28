// rg_route.hpp — the results of a launch that decided an assembled batch, back in arrival order and as lists, on the device (rg_route32, include/raftgpu.h).
//
// The run it routes is the assembler's last: e and m are the two words asm_defer_emit_kernel left in the assembler's scratch (scalars[ASM_LAST ..]), n and R are
// read from the batch's count / rounds as the tick reads them. Every grid is sized from the CAPACITIES and is one-dimensional. A wavefront of the cell domain covers
// `span` consecutive rows of ONE round, 64 at a time, a workgroup 4 * span: (round, block of rows) = (blockIdx / bpr, blockIdx % bpr), bpr = ceil(C / (4 * span));
// the send domain is cut the same way per follower. A wavefront whose first row lies at or beyond n, or whose round at or beyond R, leaves at once. Wavefront
// w = blockIdx * 4 + wave covers ascending cells, so one count per wavefront, one prefix sum over the wavefronts and a running offset + popcount(ballot below the
// lane) inside the wavefront give every list in ascending cell order — the scheme of timers_count / _scan / _emit — with no atomic anywhere. The span is chosen per
// shape (route_span): 64 — a wavefront per 64 cells, no serial walk — while the count arrays stay within 4 096 words, and doubled until they do, because ONE
// workgroup scans each of them: at 1 048 576 groups a word per 64 cells made them 49 152 + 49 152 + 65 536 words and a run 272 us where a span of 1 024 makes it
// 58. Five launches, eight with a send table, none of which waits for another workgroup:
//   1. route_fill_kernel        per arrival / expired entry below m / e: cell = RG_ROUTE_NONE
//   2. route_scatter_kernel     per cell (r < R, i < n), four rows in flight per lane: origin and the 16-byte outcome row are loaded coalesced, the row is stored
//                               as ONE 16-byte store at the entry its origin names (a lane owns a whole row: no row is split across lanes, a destination is written
//                               by exactly one lane), with the cell index and, under RG_F_PERSIST, the persist row; the same pass counts, per wavefront, the cells
//                               with RG_F_PERSIST and those with RG_NEED_HOST
//   3. timers_scan_kernel x 2   the two count arrays into offsets, their sums behind them
//   4. route_emit_kernel        per cell: {cell, gid} into persist_list / attention below their capacities; one lane writes counts
//   5. route_send_count_kernel / timers_scan_kernel / route_send_emit_kernel: per (follower, row < n) of the send table, the rows whose kind is a send, compacted
//                               follower-major; the first lane of a follower's first workgroup writes send_offset
//
// rg_route32_carry (a carrying assembler, rg_assemble.hpp): launch_route as it is — an id with bit 30 set lies at or above any m, the scatter routes it nowhere —
// and one more launch behind it over the positions of the run, sized from the three capacities:
//   6. route_carry_kernel       per position of S, from the word asm_put / asm_carry_gather_kernel left for it (`where`): a fired ticket or an arrival that was
//                               deferred gets RG_ROUTE_CARRIED | slot or RG_ROUTE_SPILLED over the RG_ROUTE_NONE of step 1; a carried slot c < q gets its entry of
//                               the carried columns — the same word, or the cell it was placed in, and then that cell's row and, under RG_F_PERSIST, persist row.
//                               Every destination is written by the one lane that owns the position
#pragma once

#include "rg_device.hpp"

namespace rg {

constexpr uint32_t ROUTE_NONE = 0xFFFFFFFFu, ROUTE_EXPIRED = 0x80000000u;
constexpr uint32_t ROUTE_SPAN_MIN = 64, ROUTE_SPAN_MAX = 4096;    // rows of one round a wavefront covers, 64 at a time (RouteParams::span, a power of two)
constexpr uint32_t ROUTE_SCAN_WORDS = 4096;      // ... chosen so that a count array, a word per wavefront, stays at or below this: one workgroup scans it

struct RouteParams {
    // the batch and what was decided over it (rg_decided_t)
    uint32_t C, D, F;                               // F = cluster - 1
    const uint32_t *gid, *count, *rounds, *origin;
    const I32x4 *row, *persist32;                   // rg_out32_t / rg_persist32_t, [D][C]
    const rg_send_t *send;                          // [F][C]; nullptr: no send list
    // the assembler's last run
    const uint32_t *last;                           // {e, m}
    uint32_t in_cap, ex_cap;
    // the routed columns and lists (rg_routed_t)
    uint32_t *cell, *ex_cell;                       // ex_cell == nullptr: no expired columns
    I32x4 *out_row, *out_persist, *ex_row, *ex_persist;
    U32x2 *persist_list, *attention, *send_list;
    uint32_t persist_cap, attention_cap, send_cap;
    uint32_t *send_offset, *counts;
    // scratch
    uint32_t span, bpr;                             // route_span(); workgroups per round (and per follower): ceil(C / (4 * span))
    uint32_t *pc, *ac;                              // [D * bpr * 4 + 1] per-wavefront counts of persist / attention cells -> offsets, last = their sum
    uint32_t *sc;                                   // [F * bpr * 4 + 1] the same for the send rows
};

hipError_t launch_route(const RouteParams &p, hipStream_t s);

struct RouteCarryParams {
    const uint32_t *last;                           // {e, m, q} of the assembler's last run
    const uint32_t *where;                          // [positions of that run] (AsmParams::where)
    uint32_t in_cap, ex_cap, carry_cap, cells;      // cells = C * D
    const I32x4 *row, *persist32;                   // [D][C]
    uint32_t *cell, *ex_cell;                       // the routed cell columns (ex_cell == nullptr: no expired columns)
    uint32_t *cr_cell;                              // rg_routed_carry_t, [carry_cap]
    I32x4 *cr_row, *cr_persist;
};

hipError_t launch_route_carry(const RouteCarryParams &p, hipStream_t s);

// the span of a shape: the smallest that keeps the longest count array — max(D, F) * ceil(C / (4 * span)) * 4 words — within ROUTE_SCAN_WORDS
inline uint32_t route_span(uint32_t C, uint32_t D, uint32_t F)
{
    const uint64_t most = D > F ? D : F;
    uint32_t span = ROUTE_SPAN_MIN;
    while (span < ROUTE_SPAN_MAX && most * ((C + 4ull * span - 1) / (4ull * span)) * 4 > ROUTE_SCAN_WORDS) span *= 2;
    return span;
}

#ifdef RG_ROUTE_KERNELS

struct RouteRun { uint32_t n, R, e, m; };

__device__ __forceinline__ RouteRun route_run(const RouteParams &p)
{
    RouteRun u;
    const uint32_t c = *p.count, d = *p.rounds, e = p.last[0], m = p.last[1];
    u.n = c < p.C ? c : p.C;
    u.R = d < 1u ? 1u : (d < p.D ? d : p.D);
    u.e = p.ex_cell ? (e < p.ex_cap ? e : p.ex_cap) : 0u;
    u.m = m < p.in_cap ? m : p.in_cap;
    return u;
}

__global__ __launch_bounds__(256) void route_fill_kernel(const RouteParams p)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x, e = p.ex_cell ? p.last[0] : 0u, m = p.last[1];
    if (s < p.in_cap) {
        if (s < m) p.cell[s] = ROUTE_NONE;
    } else if (s - p.in_cap < p.ex_cap) {
        if (s - p.in_cap < e) p.ex_cell[s - p.in_cap] = ROUTE_NONE;
    }
}

// the rows a wavefront covers: p.span consecutive rows of one round (of one follower), 64 at a time; i0 = its first row
__device__ __forceinline__ uint32_t route_first_row(const RouteParams &p) { return (blockIdx.x % p.bpr) * (4u * p.span) + (threadIdx.x >> 6) * p.span; }

__global__ __launch_bounds__(256) void route_scatter_kernel(const RouteParams p)
{
    const RouteRun u = route_run(p);
    const uint32_t r = blockIdx.x / p.bpr, i0 = route_first_row(p), w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t np = 0u, na = 0u;
    if (r < u.R) {
        for (uint32_t k0 = 0u; k0 < p.span && i0 + k0 < u.n; k0 += 4u * 64u) {      // (per wavefront) four 16-byte rows in flight per lane (a span below 256: fewer)
            I32x4 v[4];
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t i = i0 + k0 + (uint32_t)q * 64u + lane;
                v[q] = I32x4{0, 0, 0, 0};
                o[q] = ROUTE_NONE;
                if (i < u.n && k0 + (uint32_t)q * 64u < p.span) { o[q] = p.origin[r * p.C + i]; v[q] = p.row[r * p.C + i]; }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t i = i0 + k0 + (uint32_t)q * 64u + lane, at = r * p.C + i, flags = (uint32_t)v[q].y, k = o[q] & ~ROUTE_EXPIRED;
                const bool live = i < u.n && k0 + (uint32_t)q * 64u < p.span;
                uint32_t *dc = nullptr;
                I32x4 *dr = nullptr, *dp = nullptr;
                if (o[q] & ROUTE_EXPIRED) {             // (0xFFFFFFFF, no event: k = 2^31 - 1, which no e reaches)
                    if (k < u.e) { dc = p.ex_cell; dr = p.ex_row; dp = p.ex_persist; }
                } else if (k < u.m) {
                    dc = p.cell; dr = p.out_row; dp = p.out_persist;
                }
                if (live && dc) {
                    dc[k] = at;
                    dr[k] = v[q];
                    if (flags & RG_F_PERSIST) dp[k] = p.persist32[at];
                }
                np += (uint32_t)__popcll(__ballot(live && (flags & RG_F_PERSIST) != 0u));
                na += (uint32_t)__popcll(__ballot(live && RG_F_STATUS(flags) == (uint32_t)RG_NEED_HOST));
            }
        }
    }
    if (lane == 0u) { p.pc[w] = np; p.ac[w] = na; }
}

__global__ __launch_bounds__(256) void route_emit_kernel(const RouteParams p)
{
    const RouteRun u = route_run(p);
    const uint32_t r = blockIdx.x / p.bpr, i0 = route_first_row(p), w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        const uint32_t W = p.D * p.bpr * 4u;
        p.counts[0] = p.pc[W]; p.counts[1] = p.ac[W]; p.counts[3] = 0u;
        if (!p.send) p.counts[2] = 0u;
    }
    if (r >= u.R || i0 >= u.n) return;              // (per wavefront)
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t bp = p.pc[w], ba = p.ac[w];            // where the wavefront's next items go
    for (uint32_t k0 = 0u; k0 < p.span && i0 + k0 < u.n; k0 += 64u) {
        const uint32_t i = i0 + k0 + lane, at = r * p.C + i;
        const bool live = i < u.n;
        const uint32_t flags = live ? (uint32_t)p.row[at].y : 0u;
        const bool hp = live && (flags & RG_F_PERSIST) != 0u, ha = live && RG_F_STATUS(flags) == (uint32_t)RG_NEED_HOST;
        const unsigned long long mp = __ballot(hp), ma = __ballot(ha);
        if (hp || ha) {
            const U32x2 item{at, p.gid[i]};
            const uint32_t pp = bp + (uint32_t)__popcll(mp & below), pa = ba + (uint32_t)__popcll(ma & below);
            if (hp && pp < p.persist_cap) p.persist_list[pp] = item;
            if (ha && pa < p.attention_cap) p.attention[pa] = item;
        }
        bp += (uint32_t)__popcll(mp);
        ba += (uint32_t)__popcll(ma);
    }
}

__device__ __forceinline__ bool route_is_send(uint32_t kind)
{
    return kind == (uint32_t)RG_SEND_APPEND || kind == (uint32_t)RG_SEND_SNAPSHOT || kind == (uint32_t)RG_SEND_NEED_HOST;
}

__global__ __launch_bounds__(256) void route_send_count_kernel(const RouteParams p)
{
    const uint32_t c = *p.count, n = c < p.C ? c : p.C;
    const uint32_t j = blockIdx.x / p.bpr, i0 = route_first_row(p), w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t ns = 0u;
#pragma unroll 4
    for (uint32_t k0 = 0u; k0 < p.span && i0 + k0 < n; k0 += 64u) {      // (per wavefront)
        const uint32_t i = i0 + k0 + lane;
        ns += (uint32_t)__popcll(__ballot(i < n && route_is_send(p.send[(size_t)j * p.C + i].kind)));
    }
    if (lane == 0u) p.sc[w] = ns;
}

__global__ __launch_bounds__(256) void route_send_emit_kernel(const RouteParams p)
{
    const uint32_t c = *p.count, n = c < p.C ? c : p.C;
    const uint32_t j = blockIdx.x / p.bpr, i0 = route_first_row(p), w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (threadIdx.x == 0u && blockIdx.x % p.bpr == 0u) {
        p.send_offset[j] = p.sc[w];                 // (exclusive prefix: the sends of the followers before j)
        if (blockIdx.x == 0u) { const uint32_t total = p.sc[p.F * p.bpr * 4u]; p.send_offset[p.F] = total; p.counts[2] = total; }
    }
    if (i0 >= n) return;                            // (per wavefront)
    uint32_t bs = p.sc[w];
    for (uint32_t k0 = 0u; k0 < p.span && i0 + k0 < n; k0 += 64u) {
        const uint32_t i = i0 + k0 + lane;
        const bool is = i < n && route_is_send(p.send[(size_t)j * p.C + i].kind);
        const unsigned long long ms = __ballot(is);
        const uint32_t pos = bs + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull));
        if (is && pos < p.send_cap) p.send_list[pos] = U32x2{i, p.gid[i]};
        bs += (uint32_t)__popcll(ms);
    }
}

hipError_t launch_route(const RouteParams &p, hipStream_t s)
{
    const uint32_t events = p.in_cap + p.ex_cap, cells = p.D * p.bpr, W = cells * 4u;
    hipLaunchKernelGGL(route_fill_kernel, dim3(events ? (events + 255u) / 256u : 1u), dim3(256), 0, s, p);
    hipLaunchKernelGGL(route_scatter_kernel, dim3(cells), dim3(256), 0, s, p);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.pc, W, p.pc + W);
    hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.ac, W, p.ac + W);
    hipLaunchKernelGGL(route_emit_kernel, dim3(cells), dim3(256), 0, s, p);
    if (p.send) {
        const uint32_t rows = p.F * p.bpr, Ws = rows * 4u;
        hipLaunchKernelGGL(route_send_count_kernel, dim3(rows), dim3(256), 0, s, p);
        hipLaunchKernelGGL(timers_scan_kernel, dim3(1), dim3(1024), 0, s, p.sc, Ws, p.sc + Ws);
        hipLaunchKernelGGL(route_send_emit_kernel, dim3(rows), dim3(256), 0, s, p);
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void route_carry_kernel(const RouteCarryParams p)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, e = p.last[0], m = p.last[1], q = p.last[2];
    if (t < p.ex_cap) {
        if (t >= e || !p.ex_cell) return;
        const uint32_t w = p.where[t];
        if (w != ROUTE_NONE) p.ex_cell[t] = w;
    } else if (t - p.ex_cap < p.carry_cap) {
        const uint32_t c = t - p.ex_cap;
        if (c >= q) return;
        const uint32_t w = p.where[e + c];
        p.cr_cell[c] = w;
        if (w < p.cells) {
            const I32x4 v = p.row[w];
            p.cr_row[c] = v;
            if ((uint32_t)v.y & RG_F_PERSIST) p.cr_persist[c] = p.persist32[w];
        }
    } else if (t - p.ex_cap - p.carry_cap < p.in_cap) {
        const uint32_t k = t - p.ex_cap - p.carry_cap;
        if (k >= m) return;
        const uint32_t w = p.where[e + q + k];
        if (w != ROUTE_NONE) p.cell[k] = w;
    }
}

hipError_t launch_route_carry(const RouteCarryParams &p, hipStream_t s)
{
    const uint32_t events = p.in_cap + p.ex_cap + p.carry_cap;
    hipLaunchKernelGGL(route_carry_kernel, dim3(events ? (events + 255u) / 256u : 1u), dim3(256), 0, s, p);
    return hipGetLastError();
}

#endif  // RG_ROUTE_KERNELS

}  // namespace rg
