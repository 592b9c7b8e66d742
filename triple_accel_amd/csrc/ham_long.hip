// ham_long.hip -- hamming(a, b) of long strings: every pair cut into slices of S bytes, one wavefront per slice (ham_long_body.h), the
// slices of the whole batch spread over a capped, grid-strided launch.  hamming_batch_kernel (util_kernels.hip) gives a
// pair one wavefront whatever its length; this form gives a pair ceil(len / S) of them.
//
//   plan    (CSR batches only) one block: start[i] = the first slice id of pair i, start[n] = their number, start[n + 1] = the slice
//           length the batch runs with -- S, doubled until the batch has at most HAM_LONG_MAX_SLICES + n slices, so that the partial
//           counts fit a scratch whose size the host knows without knowing the lengths.  Every pair owns at least one slice: empty
//           pairs and pairs of unequal lengths too.  Strided batches need no plan: slice id = pair * slices_per_pair + slice.
//   slices  ham_long_kernel: a wavefront takes the slice ids w, w + G, w + 2G, ... (G wavefronts in the grid), finds a slice's pair
//           (a division, or a binary search in start[]), counts and stores partial[id].  Nothing of a pair of unequal lengths is read.
//   finish  ham_long_finish_kernel: out[i] = the sum of pair i's partial counts, or TA_NONE where the lengths differ -- the ONE store
//           to out[i] of the whole call (no atomics, no fill: the slot's earlier content never matters).
// Replaces hamming_simd_parallel / Avx::count_mismatches (src/hamming.rs:317, src/jewel.rs:2320-2365); result contract hamming_naive
// (src/hamming.rs:36-47).
#include <hip/hip_runtime.h>

#include "dev_str.h"
#include "ham_long_body.h"
#include "ta_internal.h"

namespace ta {

// CSR batches (n <= HAM_CSR_MAX_PAIRS): the prefix sums of max(1, ceil(len_i / S)).  One block of 1,024 threads that loops.
__global__ __launch_bounds__(1024) void ham_long_plan_kernel(StrView a, StrView b, uint32_t n, uint32_t S0, uint32_t *start) {
    __shared__ uint32_t s[1024];
    __shared__ unsigned long long bytes;
    const uint32_t t = threadIdx.x;
    if (t == 0) bytes = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (uint32_t i = t; i < n; i += 1024u) {
        const uint8_t *p;
        uint64_t la, lb;
        dev_str(a, i, p, la);
        dev_str(b, i, p, lb);
        if (la == lb) mine += la;
    }
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    if ((t & 63u) == 0 && mine) atomicAdd(&bytes, mine);          // (LDS)
    __syncthreads();
    const uint32_t S = ham_long_slice_bytes(bytes, S0);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t i = base + t;
        uint32_t c = 0;
        if (i < n) {
            const uint8_t *p;
            uint64_t la, lb;
            dev_str(a, i, p, la);
            dev_str(b, i, p, lb);
            c = la == lb && la ? (uint32_t)((la + S - 1) / S) : 1u;
        }
        s[t] = c;
        __syncthreads();
        for (uint32_t d = 1; d < 1024u; d <<= 1) {
            const uint32_t v = t >= d ? s[t - d] : 0u;
            __syncthreads();
            s[t] += v;
            __syncthreads();
        }
        if (i < n) start[i] = carry + s[t] - c;
        carry += s[1023];
        __syncthreads();
    }
    if (t == 0) { start[n] = carry; start[n + 1] = S; }
}

struct HamLongParams {
    StrView a, b;
    uint32_t n;
    uint32_t S;                   // strided: the slice length (plan: start[n + 1])
    uint32_t spp;                 // strided: slices per pair (at least 1)
    uint32_t total;               // strided: n * spp (plan: start[n])
    const uint32_t *start;        // the plan of a CSR batch, or nullptr
    uint32_t *partial;            // one count per slice id
};

__global__ __launch_bounds__(256) void ham_long_kernel(HamLongParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), G = gridDim.x * 4u;
    const uint32_t total = P.start ? P.start[P.n] : P.total, S = P.start ? P.start[P.n + 1] : P.S;
    for (uint32_t id = wave; id < total; id += G) {
        uint32_t pair, sl;
        if (P.start) {
            uint32_t lo = 0, hi = P.n;                             // the last pair whose first slice is at or before id
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (P.start[mid] <= id) lo = mid; else hi = mid;
            }
            pair = lo;
            sl = id - P.start[lo];
        } else {
            pair = id / P.spp;
            sl = id - pair * P.spp;
        }
        const uint8_t *pa, *pb;
        uint64_t la, lb;
        dev_str(P.a, pair, pa, la);
        dev_str(P.b, pair, pb, lb);
        uint32_t cnt = 0;
        const uint64_t at = (uint64_t)sl * S;
        if (la == lb && at < la) {                                 // assert!(len == b.len()): nothing of a mismatched pair is read
            const uint64_t rest = la - at;
            cnt = HamLong<DevWave>::slice(pa + at, pb + at, rest < S ? (uint32_t)rest : S);
        }
        if (lane == 0) P.partial[id] = cnt;
    }
}

// tpp threads per pair: 64 (a wavefront, four pairs per workgroup), or a workgroup of 256 or 1,024
__global__ __launch_bounds__(1024) void ham_long_finish_kernel(HamLongParams P, uint32_t *out, uint32_t tpp) {
    __shared__ uint32_t part[16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t pair = tpp == 64u ? blockIdx.x * 4u + w : blockIdx.x, t = tpp == 64u ? lane : threadIdx.x;
    const bool valid = pair < P.n;
    uint32_t sum = 0;
    bool same = false;
    if (valid) {
        const uint8_t *p;
        uint64_t la, lb;
        dev_str(P.a, pair, p, la);
        dev_str(P.b, pair, p, lb);
        same = la == lb;
        const uint32_t s0 = P.start ? P.start[pair] : pair * P.spp, s1 = P.start ? P.start[pair + 1] : s0 + P.spp;
        if (same) {
            uint32_t i = s0 + t;
            for (; i + 7u * tpp < s1; i += 8u * tpp) {             // eight loads in flight
                uint32_t v[8];
#pragma unroll
                for (uint32_t q = 0; q < 8; q++) v[q] = P.partial[i + q * tpp];
#pragma unroll
                for (uint32_t q = 0; q < 8; q++) sum += v[q];
            }
            for (; i < s1; i += tpp) sum += P.partial[i];
        }
    }
    for (uint32_t m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if (tpp == 64u) {
        if (lane == 0 && valid) out[pair] = same ? sum : 0xFFFFFFFFu;   // src/hamming.rs:38
        return;
    }
    if (lane == 0) part[w] = sum;
    __syncthreads();
    if (threadIdx.x == 0 && valid) {
        uint32_t all = 0;
        for (uint32_t q = 0; q < tpp / 64u; q++) all += part[q];
        out[pair] = same ? all : 0xFFFFFFFFu;
    }
}

static uint32_t hl_grid_waves() {
    const int cap = env_int("TA_HAM_GRID");                        // (TA_TUNING) wavefronts in the grid
    return cap > 0 ? (uint32_t)cap : HAM_LONG_GRID_WAVES;
}
static void hl_launch_slices(const HamLongParams &P, uint32_t total_bound, hipStream_t st) {
    uint32_t waves = hl_grid_waves();
    if (waves > total_bound) waves = total_bound;
    hipLaunchKernelGGL(ham_long_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, st, P);
}
static void hl_launch_finish(const HamLongParams &P, uint32_t *out, hipStream_t st) {
    // few pairs: a workgroup per pair.  A 1 GiB pair has 65,536 partial counts: 64 per thread of 1,024, eight loads at a time -- with 256
    // threads and four loads the sum took 39 us of the pair's 396 (profiles/r11/ab_hamming_long.md); a pair of a few slices gains nothing
    // from the bigger workgroup.  Many pairs: a wavefront per pair.
    if (P.n <= 64u && (P.start || P.spp >= 4096u)) hipLaunchKernelGGL(ham_long_finish_kernel, dim3(P.n), dim3(1024), 0, st, P, out, 1024u);
    else if (P.n <= 1024u) hipLaunchKernelGGL(ham_long_finish_kernel, dim3(P.n), dim3(256), 0, st, P, out, 256u);
    else hipLaunchKernelGGL(ham_long_finish_kernel, dim3((P.n + 3u) / 4u), dim3(256), 0, st, P, out, 64u);
}

// words of scratch the sliced form of this batch needs (0: it cannot take the batch -- more than 2^31 slices)
uint64_t ham_long_scratch_words(const StrView &a, const StrView &b, uint32_t n, uint32_t S0) {
    if (a.off || b.off) return (uint64_t)HAM_LONG_MAX_SLICES + 3ull * n + 8u;            // start[n + 2] | partial[<= MAX_SLICES + 2 n]
    const uint64_t len = a.len == b.len ? a.len : 0;
    const uint32_t S = ham_long_slice_bytes(len * n, S0);
    const uint64_t spp = len ? (len + S - 1) / S : 1, total = spp * n;
    return total > 0x7FFFFFFFull ? 0 : total;
}

// scratch: ham_long_scratch_words(...) u32 of device memory, dead once the finish kernel has run
hipError_t ham_long_launch(const StrView &a, const StrView &b, uint32_t n, uint32_t S0, uint32_t *scratch, uint32_t *out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    HamLongParams P = {};
    P.a = a; P.b = b; P.n = n;
    uint32_t bound;
    if (a.off || b.off) {
        P.start = scratch;
        P.partial = scratch + n + 2u;
        hipLaunchKernelGGL(ham_long_plan_kernel, dim3(1), dim3(1024), 0, st, a, b, n, S0, scratch);
        bound = 0xFFFFFFFFu;                                        // (the slice count is on the device only)
    } else {
        const uint64_t len = a.len == b.len ? a.len : 0;
        P.S = ham_long_slice_bytes(len * n, S0);
        P.spp = len ? (uint32_t)((len + P.S - 1) / P.S) : 1u;
        P.total = bound = P.spp * n;
        P.partial = scratch;
    }
    set_last_kernel_name("ham_long_kernel");
    hl_launch_slices(P, bound, st);
    hl_launch_finish(P, out, st);
    return hipGetLastError();
}

// One chunk of a pair that comes through a staging buffer piece by piece (ta_hamming on host pointers): its slices' counts go to
// partial[0 .. ceil(len / S)); ham_long_sum_launch adds up all the chunks' counts at the end.
hipError_t ham_long_chunk_launch(const uint8_t *a, const uint8_t *b, uint64_t len, uint32_t S, uint32_t *partial, hipStream_t st) {
    if (len == 0) return hipSuccess;
    HamLongParams P = {};
    P.a = StrView{a, nullptr, 0, len}; P.b = StrView{b, nullptr, 0, len}; P.n = 1;
    P.S = S; P.spp = (uint32_t)((len + S - 1) / S); P.total = P.spp; P.partial = partial;
    set_last_kernel_name("ham_long_kernel");
    hl_launch_slices(P, P.total, st);
    return hipGetLastError();
}
hipError_t ham_long_sum_launch(const uint32_t *partial, uint32_t n_partial, uint32_t *out, hipStream_t st) {
    HamLongParams P = {};
    P.a = StrView{nullptr, nullptr, 0, 0}; P.b = P.a; P.n = 1;     // (one "pair" of equal lengths whose slices are all the chunks')
    P.spp = n_partial; P.total = n_partial; P.partial = const_cast<uint32_t *>(partial);
    hl_launch_finish(P, out, st);
    return hipGetLastError();
}

}  // namespace ta
