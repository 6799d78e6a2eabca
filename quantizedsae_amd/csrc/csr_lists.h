// csr_lists.h -- per-unit lists in row order from a unit-major row bitmap: the mark, count and scan steps that the
// trainers' CSR builds (train.hip) and the tokens-per-feature lists of the analysis (token_lists.hip) share.
//
// bitmap[h][w] bit (r & 31) of word w = r >> 5: row r selected unit h.  The position of row r in unit h's list is
// offsets[h] + (set bits of row h before bit r): lists come out ordered by row, whatever order the threads ran in.  The
// only atomics are the integer ORs of the mark, whose result does not depend on their order.
#pragma once
#include "common.h"

namespace qsae {

__device__ __forceinline__ int clamp_unit(int h, int H) { return h < 0 ? 0 : (h >= H ? H - 1 : h); }

// One thread per entry e = r k + j of idx [B][k].  FILTER false: every entry marks its unit, clamped into [0, H) (the
// trainers, whose idx comes from their own top-k).  FILTER true: an entry marks only when val[e] > 0 (val == nullptr:
// always; NaN, 0.0 and -0.0 do not) and its unit lies in [0, H).  W = words per bitmap row.
template <bool FILTER>
__global__ void __launch_bounds__(256)
csr_mark_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, long long Bk, int k, int H, int W,
                uint32_t* __restrict__ bitmap) {
    const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= Bk) return;
    int h = idx[e];
    if (FILTER) {
        if (h < 0 || h >= H || (val && !(val[e] > 0.0f))) return;
    } else {
        h = clamp_unit(h, H);
    }
    const int r = static_cast<int>(e / k);
    atomicOr(bitmap + static_cast<long long>(h) * W + (r >> 5), 1u << (r & 31));
}

// Inclusive scan over the 64 lanes of a wave; every lane of the wave takes part.
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// one wave per unit: inclusive wave scan of the word popcounts, carried across rounds of 64 words.  prefix[h][w] = set
// bits of row h before word w (nullptr: not wanted), counts[h] = set bits of row h.
static __global__ void __launch_bounds__(256)
csr_count_kernel(const uint32_t* __restrict__ bitmap, int H, int W, int* __restrict__ prefix, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= H) return;                                    // wave-uniform
    const uint32_t* row = bitmap + static_cast<long long>(h) * W;
    int* pre = prefix ? prefix + static_cast<long long>(h) * W : nullptr;
    int carry = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {                   // every lane runs every round
        const int w = w0 + lane;
        const int c = w < W ? __popc(row[w]) : 0;
        const int incl = wave_inclusive_scan(c, lane);
        if (pre && w < W) pre[w] = carry + incl - c;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) counts[h] = carry;
}

// Exclusive scan of value(0 .. n - 1) into out[0..n] (out[n] = total) by one workgroup of 1024 threads.  A thread reads
// value(i) of its own range before it writes out[i], so out may be the array that value() reads at index i.
template <typename OutT, typename F>
__device__ __forceinline__ void scan_block(F value, int n, OutT* out) {
    __shared__ OutT s_w[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (n + 1023) / 1024;
    const int beg = min(n, t * per), end = min(n, beg + per);
    OutT s = 0;
    for (int i = beg; i < end; ++i) s += value(i);
    OutT incl = s;
    for (int off = 1; off < 64; off <<= 1) {
        const OutT u = __shfl_up(incl, off, 64);
        if (lane >= off) incl += u;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    OutT base = 0;
    for (int w = 0; w < wave; ++w) base += s_w[w];
    OutT run = base + incl - s;
    for (int i = beg; i < end; ++i) {
        const OutT v = value(i);
        out[i] = run;
        run += v;
    }
    if (t == 1023) out[n] = run;
}

}  // namespace qsae
