// lev_search.hip -- gfx950 kernels for levenshtein_search over a haystack shard in HBM.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>

#include "hay_line.h"
#include "lds_tab64.h"
#include "lev_filter_body.h"
#include "lev_search_body.h"
#include "lev_search_wave_body.h"
#include "ta_internal.h"

namespace ta {

template <int N, bool TRANS, bool PACKED>
__global__ __launch_bounds__(256) void lev_search_kernel(SearchParams P) {
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t emit_begin = tile * P.tile;
    if (emit_begin >= P.hay_len) return;
    uint64_t emit_end = emit_begin + P.tile;
    if (emit_end > P.hay_len) emit_end = P.hay_len;
    const uint64_t col_begin = emit_begin > P.halo ? emit_begin - P.halo : 0;
    SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, P.anchored};
    ta_match *hits = P.hits;
    unsigned long long *count = P.count;
    const uint64_t base = P.base, emit_from = P.emit_from, cap = P.cap;
    auto emit = [=](uint64_t end, uint32_t len, uint32_t cost) {
        const uint64_t gend = base + end;
        if (gend <= emit_from) return;
        unsigned long long idx = atomicAdd(count, 1ull);
        if (idx < cap) hits[idx] = ta_match{gend - len, gend, cost, 0u};
    };
    if (PACKED) lev_search_tile_packed<N, TRANS>(P.hay, P.needle, P.needle_len, C, col_begin, emit_begin, emit_end, emit);
    else lev_search_tile<N, TRANS>(P.hay, P.needle, P.needle_len, C, col_begin, emit_begin, emit_end, emit);
}

// long needles: the column lives in HBM scratch, element-major so that a wavefront's accesses coalesce
__global__ __launch_bounds__(256) void lev_search_mem_kernel(SearchParams P, uint64_t tiles) {
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= tiles) return;
    const uint64_t emit_begin = tile * P.tile;
    if (emit_begin >= P.hay_len) return;
    uint64_t emit_end = emit_begin + P.tile;
    if (emit_end > P.hay_len) emit_end = P.hay_len;
    const uint64_t col_begin = emit_begin > P.halo ? emit_begin - P.halo : 0;
    SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, P.anchored};
    ta_match *hits = P.hits;
    unsigned long long *count = P.count;
    const uint64_t base = P.base, emit_from = P.emit_from, cap = P.cap;
    lev_search_tile_mem(P.hay, P.needle_dev, P.needle_len, C, P.tc != 0, P.col_scratch + tile, tiles,
                        col_begin, emit_begin, emit_end,
                        [=](uint64_t end, uint32_t len, uint32_t cost) {
                            const uint64_t gend = base + end;
                            if (gend <= emit_from) return;
                            unsigned long long idx = atomicAdd(count, 1ull);
                            if (idx < cap) hits[idx] = ta_match{gend - len, gend, cost, 0u};
                        });
}

template <int N>
static hipError_t launch_n(const SearchParams &P, bool trans, bool packed, uint32_t grid, hipStream_t s) {
    if (packed) {
        if (trans) hipLaunchKernelGGL((lev_search_kernel<N, true, true>), dim3(grid), dim3(256), 0, s, P);
        else hipLaunchKernelGGL((lev_search_kernel<N, false, true>), dim3(grid), dim3(256), 0, s, P);
    } else if constexpr (N % 8 == 0) {
        if (trans) hipLaunchKernelGGL((lev_search_kernel<N, true, false>), dim3(grid), dim3(256), 0, s, P);
        else hipLaunchKernelGGL((lev_search_kernel<N, false, false>), dim3(grid), dim3(256), 0, s, P);
    }
    return hipGetLastError();
}

// packed: cost and length in one VGPR (see lev_search_tile_packed for the validity conditions, checked by the caller)
hipError_t lev_search_launch(const SearchParams &P, bool packed, bool trans, hipStream_t s) {
    if (P.hay_len == 0) return hipSuccess;
    set_last_kernel_name("lev_search%s_kernel", P.needle_len <= 32 ? "" : "_mem");
    const uint64_t tiles = (P.hay_len + P.tile - 1) / P.tile;
    const uint32_t grid = (uint32_t)((tiles + 255) / 256);
    const uint32_t n = P.needle_len;
    if (packed && n <= 32) {              // one instantiation per needle length: straight-line column code
        switch (n) {
#define TA_N(x) case x: return launch_n<x>(P, trans, true, grid, s);
            TA_N(1) TA_N(2) TA_N(3) TA_N(4) TA_N(5) TA_N(6) TA_N(7) TA_N(8) TA_N(9) TA_N(10) TA_N(11) TA_N(12)
            TA_N(13) TA_N(14) TA_N(15) TA_N(16) TA_N(17) TA_N(18) TA_N(19) TA_N(20) TA_N(21) TA_N(22) TA_N(23) TA_N(24)
            TA_N(25) TA_N(26) TA_N(27) TA_N(28) TA_N(29) TA_N(30) TA_N(31) TA_N(32)
#undef TA_N
        }
    }
    if (n <= 8) return launch_n<8>(P, trans, false, grid, s);
    if (n <= 16) return launch_n<16>(P, trans, false, grid, s);
    if (n <= 24) return launch_n<24>(P, trans, false, grid, s);
    if (n <= 32) return launch_n<32>(P, trans, false, grid, s);
    hipLaunchKernelGGL(lev_search_mem_kernel, dim3(grid), dim3(256), 0, s, P, tiles);
    return hipGetLastError();
}

// ---- candidate filter + exact kernel on the flagged blocks (unit-cost families, needle <= 32 bytes)

// One lane scans P.tile end positions (a multiple of 64) after P.halo bytes of left context and appends the index of
// every 64-column block that holds a cost <= k to `list` (lev_filter_body.h).  The 256-entry match table of the
// needle lives in LDS; the haystack is read 16 bytes per lane per load.
// REPL: the match table is kept once per lane of a wavefront (lds_tab64.h: 512 threads, two workgroups = 16 wavefronts per CU);
// without it (TA_FILTER_FLAT=1) one flat 256-entry table, bank conflicts on random bytes.
template <bool TRANS, bool REPL, bool EXACT = false>
__global__ __launch_bounds__(REPL ? 512 : 256) void lev_filter_kernel(SearchParams P, uint32_t *list, uint32_t list_cap, unsigned int *list_count) {
    __shared__ __attribute__((aligned(16))) uint32_t peq[REPL ? 256 * 64 : 256];
    if (REPL) tab64_fill(peq, lev_filter_peq(P.needle, P.needle_len, threadIdx.x >> 1));
    else peq[threadIdx.x] = lev_filter_peq(P.needle, P.needle_len, threadIdx.x);
    __syncthreads();
    const uint32_t lane_off = (threadIdx.x & 63u) * 4u;
    // table entry of byte b (0..3) of dword v
    auto lookup = [&](uint32_t v, int b) -> uint32_t {
        if (REPL) return tab64_lookup(peq, lane_off, v, b);
        return peq[(v >> (8 * b)) & 0xffu];
    };
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t emit_begin = tile * P.tile;
    if (emit_begin >= P.hay_len) return;
    uint64_t emit_end = emit_begin + P.tile;
    if (emit_end > P.hay_len) emit_end = P.hay_len;
    const uint64_t col_begin = emit_begin > P.halo ? emit_begin - P.halo : 0;
    const uint32_t k = P.k;
    const uint8_t *hay = P.hay;
    FilterState st;
    lev_filter_reset(st, P.needle_len);
    for (uint64_t i = col_begin; i < emit_begin; i++) lev_filter_step<TRANS>(st, lookup(hay[i], 0));   // left context
    auto flag = [&](uint64_t col) {
        const unsigned int idx = atomicAdd(list_count, 1u);
        if (idx < list_cap) list[idx] = (uint32_t)(col / FILTER_BLOCK);
    };
    uint64_t i = emit_begin;
    const uint64_t full_end = emit_begin + ((emit_end - emit_begin) & ~(uint64_t)(FILTER_BLOCK - 1));
    static_assert(2 * FILTER_BLOCK == 128, "a line of eight quads is two blocks");
    u32x4u nxt[8], cur[8];
    hay_line_prime<8>(nxt, hay, i, emit_end);                     // a whole 128-byte line per lane, one line ahead (hay_line.h)
    while (i < full_end) {                                        // whole 64-column blocks, two per line
        hay_line_turn<8>(cur, nxt, hay, i, emit_end);
#pragma unroll 1
        for (int blk = 0; blk < 2 && i < full_end; blk++) {
            bool any = false;
            if (EXACT) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const u32x4u v = blk == 0 ? cur[q] : cur[4 + q];
#pragma unroll
                    for (int b = 0; b < 16; b++) any |= lev_filter_step<TRANS>(st, lookup(v[b >> 2], b & 3)) <= k;
                }
            } else {            // the score settled per 32 columns: a lower bound of the block's smallest cost (lev_filter_fold32)
#pragma unroll
                for (int half = 0; half < 2; half++) {
                    uint32_t MH = 0;
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const u32x4u v = blk == 0 ? cur[2 * half + q] : cur[4 + 2 * half + q];
#pragma unroll
                        for (int b = 0; b < 16; b++) lev_filter_step_h<TRANS>(st, lookup(v[b >> 2], b & 3), MH);
                    }
                    any |= lev_filter_fold32(st, MH, k);
                }
            }
            if (any) flag(i);
            i += FILTER_BLOCK;
        }
    }
    if (i < emit_end) {                                           // the shard's last, partial block
        bool any = false;
        for (uint64_t j = i; j < emit_end; j++) any |= lev_filter_step<TRANS>(st, lookup(hay[j], 0)) <= k;
        if (any) flag(i);
    }
}

// needles of 33..512 bytes: NWF-dword vectors, match table (256 x NWF dwords) in LDS built from the device copy of the needle
template <int NWF, bool TRANS>
__global__ __launch_bounds__(256) void lev_filter_kernel_n(SearchParams P, uint32_t *list, uint32_t list_cap, unsigned int *list_count) {
    __shared__ uint32_t peq[256 * NWF];
    for (int w = 0; w < NWF; w++) peq[threadIdx.x * NWF + w] = lev_filter_peq_word(P.needle_dev, P.needle_len, NWF, threadIdx.x, w);
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t emit_begin = tile * P.tile;
    if (emit_begin >= P.hay_len) return;
    uint64_t emit_end = emit_begin + P.tile;
    if (emit_end > P.hay_len) emit_end = P.hay_len;
    const uint64_t col_begin = emit_begin > P.halo ? emit_begin - P.halo : 0;
    const uint32_t k = P.k;
    const uint8_t *hay = P.hay;
    FilterStateN<NWF> st;
    lev_filter_reset_n<NWF>(st, P.needle_len);
    auto stepc = [&](uint32_t c) -> uint32_t {
        uint32_t Eq[NWF];
#pragma unroll
        for (int w = 0; w < NWF; w++) Eq[w] = peq[c * NWF + w];
        return lev_filter_step_n<NWF, TRANS>(st, Eq);
    };
    auto flag = [&](uint64_t col) {
        const unsigned int idx = atomicAdd(list_count, 1u);
        if (idx < list_cap) list[idx] = (uint32_t)(col / FILTER_BLOCK);
    };
    for (uint64_t i = col_begin; i < emit_begin; i++) stepc(hay[i]);               // left context
    uint64_t i = emit_begin;
    const uint64_t full_end = emit_begin + ((emit_end - emit_begin) & ~(uint64_t)(FILTER_BLOCK - 1));
    u32x4u nxt[4], cur[4];
    hay_line_prime<4>(nxt, hay, i, emit_end);
    while (i < full_end) {                                        // whole 64-column blocks, requested one block ahead
        hay_line_turn<4>(cur, nxt, hay, i, emit_end);
        bool any = false;
#pragma unroll 1
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int b = 0; b < 16; b++) any |= stepc((cur[q][b >> 2] >> (8 * (b & 3))) & 0xffu) <= k;
        }
        if (any) flag(i);
        i += FILTER_BLOCK;
    }
    if (i < emit_end) {                                           // the shard's last, partial block
        bool any = false;
        for (uint64_t j = i; j < emit_end; j++) any |= stepc(hay[j]) <= k;
        if (any) flag(i);
    }
}

template <int NWF>
static hipError_t launch_filter_n(const SearchParams &P, bool trans, uint32_t grid, uint32_t *list, uint32_t list_cap,
                                  unsigned int *list_count, hipStream_t s) {
    if (trans) hipLaunchKernelGGL((lev_filter_kernel_n<NWF, true>), dim3(grid), dim3(256), 0, s, P, list, list_cap, list_count);
    else hipLaunchKernelGGL((lev_filter_kernel_n<NWF, false>), dim3(grid), dim3(256), 0, s, P, list, list_cap, list_count);
    return hipGetLastError();
}

hipError_t lev_filter_launch(const SearchParams &P, bool trans, uint32_t *list, uint32_t list_cap, unsigned int *list_count,
                             hipStream_t s) {
    if (P.hay_len == 0) return hipSuccess;
    const uint64_t tiles = (P.hay_len + P.tile - 1) / P.tile;
    const uint32_t grid = (uint32_t)((tiles + 255) / 256);
    set_last_kernel_name("lev_filter_kernel%s", P.needle_len <= 32 ? "" : "_n");
    switch ((P.needle_len + 31u) / 32u) {
        case 1:
            if (!env_str("TA_FILTER_FLAT")) {
                const uint32_t g2 = (uint32_t)((tiles + 511) / 512);
                if (env_str("TA_FILTER_EXACT")) {   // A/B: the score per column (flags exactly the blocks that hold a hit)
                    if (trans) hipLaunchKernelGGL((lev_filter_kernel<true, true, true>), dim3(g2), dim3(512), 0, s, P, list, list_cap, list_count);
                    else hipLaunchKernelGGL((lev_filter_kernel<false, true, true>), dim3(g2), dim3(512), 0, s, P, list, list_cap, list_count);
                    return hipGetLastError();
                }
                if (trans) hipLaunchKernelGGL((lev_filter_kernel<true, true>), dim3(g2), dim3(512), 0, s, P, list, list_cap, list_count);
                else hipLaunchKernelGGL((lev_filter_kernel<false, true>), dim3(g2), dim3(512), 0, s, P, list, list_cap, list_count);
                return hipGetLastError();
            }
            // A/B (TA_FILTER_FLAT=1): the flat 256-entry table (bank conflicts on random bytes), 256 threads per workgroup
            if (trans) hipLaunchKernelGGL((lev_filter_kernel<true, false, true>), dim3(grid), dim3(256), 0, s, P, list, list_cap, list_count);
            else hipLaunchKernelGGL((lev_filter_kernel<false, false, true>), dim3(grid), dim3(256), 0, s, P, list, list_cap, list_count);
            return hipGetLastError();
        case 2: return launch_filter_n<2>(P, trans, grid, list, list_cap, list_count, s);
        case 3: return launch_filter_n<3>(P, trans, grid, list, list_cap, list_count, s);
        case 4: return launch_filter_n<4>(P, trans, grid, list, list_cap, list_count, s);
        case 5: return launch_filter_n<5>(P, trans, grid, list, list_cap, list_count, s);
        case 6: return launch_filter_n<6>(P, trans, grid, list, list_cap, list_count, s);
        case 7: return launch_filter_n<7>(P, trans, grid, list, list_cap, list_count, s);
        case 8: return launch_filter_n<8>(P, trans, grid, list, list_cap, list_count, s);
        case 9: case 10: case 11: case 12: return launch_filter_n<12>(P, trans, grid, list, list_cap, list_count, s);     // needles of up to 384 bytes
        case 13: case 14: case 15: case 16: return launch_filter_n<16>(P, trans, grid, list, list_cap, list_count, s);    // up to 512 (round 5; the table: 16 KB of LDS)
        default: return hipErrorInvalidValue;
    }
}

// the memory-backed exact kernel (needles > 32 bytes) on the flagged blocks
__global__ __launch_bounds__(64) void lev_search_mem_list_kernel(SearchParams P, const uint32_t *list, uint32_t n_list) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_list) return;
    const uint64_t emit_begin = (uint64_t)list[t] * FILTER_BLOCK;
    uint64_t emit_end = emit_begin + FILTER_BLOCK;
    if (emit_end > P.hay_len) emit_end = P.hay_len;
    const uint64_t col_begin = emit_begin > P.halo ? emit_begin - P.halo : 0;
    SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, P.anchored};
    ta_match *hits = P.hits;
    unsigned long long *count = P.count;
    const uint64_t base = P.base, emit_from = P.emit_from, cap = P.cap;
    lev_search_tile_mem(P.hay, P.needle_dev, P.needle_len, C, P.tc != 0, P.col_scratch + t, n_list, col_begin, emit_begin, emit_end,
                        [=](uint64_t end, uint32_t len, uint32_t cost) {
                            const uint64_t gend = base + end;
                            if (gend <= emit_from) return;
                            unsigned long long idx = atomicAdd(count, 1ull);
                            if (idx < cap) hits[idx] = ta_match{gend - len, gend, cost, 0u};
                        });
}

// ---- the exact (cost, length) kernel on the flagged 64-column blocks: ONE WAVEFRONT per block (lev_search_wave_body.h)
//
// Persistent grid (SRCH_WAVE_GRID workgroups of 4 wavefronts): the number of flagged blocks is read ON THE DEVICE -- the
// host never waits between the filter and this kernel.  The last workgroup to finish writes the report (hit count, and for
// a Best pass the hits with the smallest k) into host-mapped pinned memory: one stream synchronisation tells the host
// everything, no copy.  When the filter flagged so many blocks that the lane-per-tile kernel over everything is cheaper,
// nothing is searched and the report says so.
//
// No device-wide fence anywhere: an agent-scope release on gfx950 is an L2 write-back (buffer_wbl2), and one per wavefront
// made this kernel 300 us long.  What crosses workgroups goes through agent-scope atomics instead: the hit cursor, the
// Best passes' hit records and block slots (stored with agent-scope atomic stores = write-through), the done counter.
// Best passes (only the hits with the smallest k can survive the Best fold): no running minimum, no second cursor -- a block
// leaves ONE 16-byte slot {its best cost, its hit count, where its hits start} (agent-scope atomic stores = write-through, like
// its hit records), the last workgroup takes the minimum over the n_list slots and picks the hits of that cost out of the few
// blocks that reach it.  (A running atomicMax plus a candidate cursor cost every block two more serial round trips: 45 us
// against 31 us for the All-mode kernel, profiles/r03/ab_search.md.)
constexpr uint32_t SRCH_WAVE_GRID = 512;
constexpr uint32_t SRCH_WAVE_DENSE_MUL = 5;          // a block costs ~5x its columns in the lane-per-tile kernel's currency

static __device__ __forceinline__ void store_match_agent(ta_match *dst, uint64_t start, uint64_t end, uint32_t k) {
    unsigned long long *w = (unsigned long long *)dst;
    __hip_atomic_store(w, (unsigned long long)start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 1, (unsigned long long)end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 2, (unsigned long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool TRANS, bool BEST>
__global__ __launch_bounds__(256) void lev_search_wave_kernel(SearchParams P, const uint32_t *list, uint32_t cap_list, SearchCtl *ctl,
                                                              SearchSlot *slots, uint8_t *report, uint32_t done_groups) {
    __shared__ uint32_t s_last, s_sel;
    __shared__ __attribute__((aligned(16))) uint32_t s_row[4][64];        // per wavefront: the last row's values of a block's emitted columns
    (void)store_match_agent;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), n_waves = gridDim.x * 4u;   // wave-uniform: scalar loop control
    const uint32_t t_enter = (uint32_t)__builtin_amdgcn_s_memrealtime();
    const uint32_t n_list = ctl->n_list;                                   // written by the filter kernel before this launch
    const uint64_t per_block = (uint64_t)FILTER_BLOCK + P.halo + P.needle_len;
    const bool dense = n_list > cap_list || (uint64_t)n_list * per_block * SRCH_WAVE_DENSE_MUL >= P.hay_len;
    if (!dense) {
        // the needle, one byte per lane, straight from the kernarg segment (P is the first argument)
        const uint8_t *needle = (const uint8_t *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SearchParams, needle);
        const SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, 0u};
        ta_match *hits = P.hits;
        const uint64_t base = P.base, emit_from = P.emit_from, cap = P.cap;
        for (uint32_t t = wave; t < n_list; t += n_waves) {
            const uint64_t emit_begin = (uint64_t)list[t] * FILTER_BLOCK;
            uint64_t emit_end = emit_begin + FILTER_BLOCK;
            if (emit_end > P.hay_len) emit_end = P.hay_len;
            const uint64_t col_begin = emit_begin > P.halo ? emit_begin - P.halo : 0;
            if (BEST && t < SEARCH_SLOT_CAP && lane == 0)                  // "no hits" until the block says otherwise (no fill needed)
                __hip_atomic_store((unsigned long long *)(slots + t), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lev_search_block_wave<DevWave, TRANS>(P.hay, needle, P.needle_len, C, col_begin, emit_begin, emit_end, (uint8_t *)s_row[threadIdx.x >> 6],
                [=](bool hit, uint32_t key, uint32_t col) {               // lane t: emitted column t of the block
                    const uint64_t gend = base + col_begin + col + 1;
                    const uint32_t cost = key >> 16, len = 0xFFFFu - (key & 0xFFFFu);
                    const bool mine = hit && gend > emit_from;
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
                    if (m == 0) return;
                    const uint32_t cnt = (uint32_t)__builtin_popcountll(m), rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                    const uint32_t leader = (uint32_t)__builtin_ctzll(m);
                    unsigned long long idx0 = 0;
                    if (lane == leader) idx0 = atomicAdd(&ctl->count, (unsigned long long)cnt);
                    idx0 = ((unsigned long long)__builtin_amdgcn_readlane((uint32_t)(idx0 >> 32), leader) << 32) |
                           (unsigned long long)__builtin_amdgcn_readlane((uint32_t)idx0, leader);
                    if (mine && idx0 + rank < cap) {
                        if (BEST) store_match_agent(hits + idx0 + rank, gend - len, gend, cost);     // the last workgroup may read it
                        else hits[idx0 + rank] = ta_match{gend - len, gend, cost, 0u};
                    }
                    if (BEST && t < SEARCH_SLOT_CAP) {
                        const uint32_t inv = DevWave::wave_max(mine ? 0xFFFFFFFFu - cost : 0u);      // 0xFFFFFFFF - the block's best cost
                        if (lane == leader) {
                            unsigned long long *sw = (unsigned long long *)(slots + t);
                            __hip_atomic_store(sw, ((unsigned long long)cnt << 32) | (0xFFFFFFFFu - inv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(sw + 1, idx0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                });
        }
    }
    if (wave == 0 && lane == 0) {
        __hip_atomic_store(&ctl->pad[0], t_enter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ctl->pad[1], (uint32_t)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // last workgroup out writes the report.  Every store that another workgroup reads later was an agent-scope atomic store and this
    // wavefront's own memory operations are waited for (s_waitcnt 0); on top of that:
    // Bit 31 of done_groups (the default; TA_SRCH_NO_FENCE=1 clears it): thread 0 of every workgroup issues ONE agent-scope release fence in
    // front of its counter bump and the last workgroup an acquire fence behind it -- the release / acquire pair the language memory model
    // asks for, per workgroup, not per wavefront (per wavefront it made the kernel 300 us long; per workgroup it costs 2-6 us per pass).
    const bool fenced = (done_groups & 0x80000000u) != 0u;
    done_groups &= 0x7FFFFFFFu;
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) {       // two levels: the last workgroup of a group bumps the groups' counter
        if (fenced) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const uint32_t g = blockIdx.x % done_groups, members = gridDim.x / done_groups + (g < gridDim.x % done_groups ? 1u : 0u);
        uint32_t last = 0;
        if (__hip_atomic_fetch_add(&ctl->done[g * 16u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1u)
            last = __hip_atomic_fetch_add(&ctl->done2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == done_groups - 1u ? 1u : 0u;
        s_last = last;
    }
    s_sel = 0;
    __syncthreads();
    if (!s_last) return;
    if (fenced) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t t_report = (uint32_t)__builtin_amdgcn_s_memrealtime();
    const unsigned long long count = __hip_atomic_load(&ctl->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SearchReport *rep = (SearchReport *)report;
    uint32_t sel_state = 0, min_k = 0xFFFFFFFFu, n_cand_seen = 0;
    if (BEST && !dense) {
        if (count <= P.cap && n_list <= SEARCH_SLOT_CAP) {
            __shared__ uint32_t s_min;
            if (threadIdx.x == 0) s_min = 0xFFFFFFFFu;
            __syncthreads();
            const unsigned long long *sw = (const unsigned long long *)slots;
            uint32_t mine_min = 0xFFFFFFFFu;
            for (uint32_t i0 = 0; i0 < n_list; i0 += 1024u) {          // four loads in flight per thread: other workgroups wrote the
                unsigned long long w[4];                                 // slots, they are read past the L1 / this XCD's L2
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t i = i0 + 256u * (uint32_t)j + threadIdx.x;
                    w[j] = i < n_list ? __hip_atomic_load(sw + 2 * (uint64_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                }
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if ((uint32_t)(w[j] >> 32) != 0u && (uint32_t)w[j] < mine_min) mine_min = (uint32_t)w[j];
            }
            if (mine_min != 0xFFFFFFFFu) atomicMin(&s_min, mine_min);
            __syncthreads();
            min_k = s_min;
            ta_match *sel = (ta_match *)(report + sizeof(SearchReport));
            const unsigned long long *hw = (const unsigned long long *)P.hits;
            if (min_k != 0xFFFFFFFFu) {
                for (uint32_t i = threadIdx.x; i < n_list; i += 256u) {
                    const unsigned long long w = __hip_atomic_load(sw + 2 * (uint64_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t cnt = (uint32_t)(w >> 32);
                    if (cnt == 0u || (uint32_t)w != min_k) continue;
                    const unsigned long long idx0 = __hip_atomic_load(sw + 2 * (uint64_t)i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (uint32_t q = 0; q < cnt; q++) {
                        const unsigned long long w2 = __hip_atomic_load(hw + 3 * (idx0 + q) + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((uint32_t)w2 != min_k) continue;
                        const unsigned long long w0 = __hip_atomic_load(hw + 3 * (idx0 + q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const unsigned long long w1 = __hip_atomic_load(hw + 3 * (idx0 + q) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const uint32_t pos = atomicAdd(&s_sel, 1u);
                        if (pos < SEARCH_REPORT_SEL) sel[pos] = ta_match{w0, w1, (uint32_t)w2, 0u};
                    }
                }
            }
            __syncthreads();
            sel_state = s_sel <= SEARCH_REPORT_SEL ? 1u : 2u;
            n_cand_seen = n_list;
        } else {
            sel_state = 2u;
        }
    }
    if (threadIdx.x == 0) {
        rep->count = count; rep->n_list = n_list; rep->dense = dense ? 1u : 0u;
        rep->sel_count = s_sel; rep->sel_state = sel_state; rep->min_k = min_k; rep->n_slots = n_cand_seen;
        rep->t[0] = __hip_atomic_load(&ctl->pad[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rep->t[1] = __hip_atomic_load(&ctl->pad[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rep->t[2] = t_report; rep->t[3] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    }
}

hipError_t lev_search_wave_launch(const SearchParams &P, bool trans, bool best, const uint32_t *list, uint32_t cap_list,
                                  SearchCtl *ctl, SearchSlot *slots, uint8_t *report_dev, hipStream_t s) {
    if (P.needle_len == 0 || P.needle_len > 64 || FILTER_BLOCK + P.halo > SRCH_WAVE_MAX_COLS) return hipErrorInvalidValue;
    uint32_t g = SRCH_WAVE_GRID, done_groups = SEARCH_DONE_GROUPS;
    if (const char *e = env_str("TA_SRCH_GRID")) { const int v = atoi(e); if (v >= 1 && v <= 4096) g = (uint32_t)v; }
    if (const char *e = env_str("TA_SRCH_DONE_GROUPS")) { const int v = atoi(e); if (v >= 1 && v <= (int)SEARCH_DONE_GROUPS) done_groups = (uint32_t)v; }
    if (done_groups > g) done_groups = g;
    if (!env_str("TA_SRCH_NO_FENCE")) done_groups |= 0x80000000u;    // (2-6 us of a 0.49 ms pass: profiles/r04/raw/probe_search_fence.txt)
    const dim3 grid(g), block(256);
    if (trans) {
        if (best) hipLaunchKernelGGL((lev_search_wave_kernel<true, true>), grid, block, 0, s, P, list, cap_list, ctl, slots, report_dev, done_groups);
        else hipLaunchKernelGGL((lev_search_wave_kernel<true, false>), grid, block, 0, s, P, list, cap_list, ctl, slots, report_dev, done_groups);
    } else {
        if (best) hipLaunchKernelGGL((lev_search_wave_kernel<false, true>), grid, block, 0, s, P, list, cap_list, ctl, slots, report_dev, done_groups);
        else hipLaunchKernelGGL((lev_search_wave_kernel<false, false>), grid, block, 0, s, P, list, cap_list, ctl, slots, report_dev, done_groups);
    }
    return hipGetLastError();
}

// needles beyond the wavefront kernel's 64 rows: the memory-backed column, one lane per flagged block
hipError_t lev_search_list_launch(const SearchParams &P, bool /*trans*/, const uint32_t *list, uint32_t n_list, hipStream_t s) {
    if (n_list == 0) return hipSuccess;
    if (P.needle_len <= 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lev_search_mem_list_kernel, dim3((n_list + 63) / 64), dim3(64), 0, s, P, list, n_list);
    return hipGetLastError();
}

}  // namespace ta
