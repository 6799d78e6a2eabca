// watch.hip -- the distributions of a model in training (what `wandb.watch(model, log="all")` logs every log_freq steps in
// the reference's Trainer, training/trainer.py:51): for every tensor of a list of fp32 tensors of
// any sizes, in one call, the 64-bin histogram of its finite elements between their minimum and maximum, the counts of
// finite / non-finite / zero elements, and mean and sum of squared deviations in fp64.  Two streaming passes over the
// data and two small joins; nothing is read back.
//
// The bin rule is the one torch.histc applies on the CPU (torch 2.10), every operation in fp32, one rounding each (the
// build passes -ffp-contract=off, the division is the correctly rounded one):
//     q = ((x - lo) * float(bins)) / (hi - lo);   bin = int(q), and bin == bins (x == hi) goes to bins - 1.
// The other candidate, ((x - lo) / (hi - lo)) * bins, differs from torch on some inputs (tests/watch_util.py keeps one).
// With lo == hi torch widens the range: lo' = fl(lo - 1), or the float below lo where that is lo again (lo itself where
// that float is -inf), and hi' likewise upwards; q is formed with lo' and hi' - lo'.  Below 2^24 in magnitude that is
// [lo - 1, lo + 1] and every element lands in bin bins / 2.  Where hi - lo overflows fp32, torch counts nothing and so
// does this kernel.  Where hi - lo is finite but (x - lo) * bins overflows, torch converts an infinity to an integer,
// which is undefined; here such an element goes to bin 0.  A zero minimum or maximum is reported as +0.0.
//
// Layout of the work.  Tensor t is cut into chunks of kWsChunk = 8192 elements; a workgroup of 256 threads owns one
// chunk, in 8 slabs of 1024: thread j takes the 4 consecutive elements 4 j .. 4 j + 3 of every slab (one 16-byte load
// when the tensor starts on a 16-byte boundary and the 4 elements exist, 4 scalar loads otherwise: the same elements in
// the same order, hence the same bits).  Workgroups find their (tensor, chunk) through a table of chunk prefix counts
// that travels in the kernel arguments, kWsTable = 32 tensors per launch; longer lists take several launches.
//
// Order of the fp64 sums (the scheme of evaluation.hip and trainer.hip): a thread adds its finite elements in ascending
// (slab, element) order from 0.0; the 64 lane sums of a wave are joined by a butterfly (xor 32, 16, ..., 1), the 4 wave
// sums added in ascending order: that is a chunk's partial.  One workgroup per tensor then lets thread j add the chunk
// partials j, j + 256, ... in ascending order from 0.0 and joins the 256 threads the same way.  mean = S / n_finite in
// fp64; pass 2 adds (double(x) - mean)^2 (one fp64 subtraction, one multiplication, one addition) in the same order.
// No float atomics.  Counts go through integer atomics, which do not depend on order: a per-workgroup histogram in LDS,
// where the lanes of a wave that hit the same bin issue ONE add of their number (a ballot over the bin index: the
// gradients of the top-k models are mostly exact zeros, and 64 lanes adding 1 to one LDS word would serialise), then
// one 64-bit global add per non-empty bin and workgroup.
#include "common.h"
#include <math.h>

namespace qsae {

typedef float ws_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWsWaves = 4;
constexpr int kWsThreads = 64 * kWsWaves;
constexpr int kWsSlabs = 8;
constexpr long long kWsSlab = kWsThreads * 4;                         // elements of one slab: 4 consecutive per thread
constexpr long long kWsChunk = kWsSlab * kWsSlabs;                    // elements of one workgroup
constexpr int kWsTable = 32;                                          // tensors of one launch
constexpr int kWsMaxBins = 256;
constexpr int kWsMaxTensors = 65536;
constexpr long long kWsMaxElems = 1ll << 40;                          // per tensor
constexpr long long kWsMaxChunks = 1ll << 30;                         // of one call
constexpr int kWsHead = QSAE_TENSOR_STATS_HEAD;                       // result words in front of a tensor's counts
// result words of a tensor (8 bytes each): fp64 images of lo and hi, mean, m2; int64 n_finite, n_nonfinite, n_zero, 0
constexpr int kWsLo = 0, kWsHi = 1, kWsMean = 2, kWsM2 = 3, kWsFinite = 4, kWsNonfinite = 5, kWsZero = 6;

struct WatchTable {
    const float* p[kWsTable];
    long long n[kWsTable];
    int chunk0[kWsTable + 1];         // first workgroup of tensor i in this launch; chunk0[count] = the launch's workgroups
    int count;                        // tensors of this launch
    int first;                        // index of tensor 0 of this launch in the call's list
    int chunk_base;                   // index of workgroup 0's chunk among the call's chunks
};

// what pass 2 needs of a tensor, written by the first join
struct WatchRec {
    double mean;
    float rlo, width;                 // q = (x - rlo) * bins / width
    int binned;                       // 0: no histogram (no finite element, or hi - lo overflows)
    int pad;
};

struct WatchParts {                   // per chunk of the call
    double* sum;
    double* m2;
    float* mn;
    float* mx;
    int* fin;
    int* zero;
};

__device__ __forceinline__ double ws_wave_add(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int ws_wave_add_i(int v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float ws_wave_min(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float ws_wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// the 64 lane sums by a butterfly, then the 4 wave sums in ascending wave order; valid in thread 0.  Every thread of the
// workgroup comes here.
__device__ __forceinline__ double ws_block_add(double v, double* s_w) {
    v = ws_wave_add(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = s_w[0];
        for (int w = 1; w < kWsWaves; ++w) r = r + s_w[w];
    }
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool ws_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// the tensor of workgroup b: the largest i < count with chunk0[i] <= b (tensors without elements own no workgroup)
__device__ __forceinline__ int ws_find(const WatchTable& tb, int b) {
    int i = 0;
    for (int step = kWsTable / 2; step >= 1; step >>= 1)
        if (i + step < tb.count && tb.chunk0[i + step] <= b) i += step;
    return i;
}

// 4 elements from e0 (a multiple of 4); those at or past n read as 0 and are not used
__device__ __forceinline__ void ws_load4(const float* __restrict__ p, long long e0, long long n, bool vec, float (&v)[4]) {
    if (vec && e0 + 3 < n) {
        const ws_f32x4 q = *reinterpret_cast<const ws_f32x4*>(p + e0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = e0 + j < n ? p[e0 + j] : 0.f;
    }
}

// ---- pass 1: minimum, maximum, counts and the sum of a chunk ---------------------------------------------------------------
__global__ void __launch_bounds__(kWsThreads)
watch_pass1_kernel(WatchTable tb, WatchParts parts) {
    __shared__ double s_w[kWsWaves];
    __shared__ float s_mn[kWsWaves], s_mx[kWsWaves];
    __shared__ int s_fin[kWsWaves], s_zero[kWsWaves];
    const int b = static_cast<int>(blockIdx.x), i = ws_find(tb, b);
    const float* __restrict__ p = tb.p[i];
    const long long n = tb.n[i];
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
    const long long chunk_at = static_cast<long long>(b - tb.chunk0[i]) * kWsChunk;
    double acc = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    int fin = 0, zero = 0;
    for (int k = 0; k < kWsSlabs; ++k) {
        const long long e0 = chunk_at + k * kWsSlab + 4 * static_cast<long long>(threadIdx.x);
        if (e0 >= n) break;
        float v[4];
        ws_load4(p, e0, n, vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = v[j];
            if (e0 + j < n && ws_finite(x)) {
                acc = acc + static_cast<double>(x);
                mn = fminf(mn, x);
                mx = fmaxf(mx, x);
                fin += 1;
                zero += (x == 0.0f) ? 1 : 0;
            }
        }
    }
    const double sum = ws_block_add(acc, s_w);
    mn = ws_wave_min(mn); mx = ws_wave_max(mx);
    fin = ws_wave_add_i(fin); zero = ws_wave_add_i(zero);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s_mn[w] = mn; s_mx[w] = mx; s_fin[w] = fin; s_zero[w] = zero;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long g = static_cast<long long>(tb.chunk_base) + b;
    for (int w = 1; w < kWsWaves; ++w) {
        mn = fminf(mn, s_mn[w]); mx = fmaxf(mx, s_mx[w]);
        fin += s_fin[w]; zero += s_zero[w];
    }
    parts.sum[g] = sum;
    parts.mn[g] = mn; parts.mx[g] = mx;
    parts.fin[g] = fin; parts.zero[g] = zero;
}

// the float below / above v, v itself where that is infinite (v finite)
__device__ __forceinline__ float ws_below(float v) {
    const uint32_t u = __float_as_uint(v);
    const float r = (v == 0.0f) ? __uint_as_float(0x80000001u) : __uint_as_float((u & 0x80000000u) ? u + 1u : u - 1u);
    return ws_finite(r) ? r : v;
}
__device__ __forceinline__ float ws_above(float v) {
    const uint32_t u = __float_as_uint(v);
    const float r = (v == 0.0f) ? __uint_as_float(0x00000001u) : __uint_as_float((u & 0x80000000u) ? u - 1u : u + 1u);
    return ws_finite(r) ? r : v;
}

// ---- join 1: one workgroup per tensor of the launch -> lo, hi, the range of the bins, the mean, the counts ------------------
__global__ void __launch_bounds__(kWsThreads)
watch_join1_kernel(WatchTable tb, WatchParts parts, WatchRec* __restrict__ recs, unsigned long long* __restrict__ result, int words) {
    __shared__ double s_w[kWsWaves];
    __shared__ float s_mn[kWsThreads], s_mx[kWsThreads];
    __shared__ long long s_fin[kWsThreads], s_zero[kWsThreads];
    const int i = static_cast<int>(blockIdx.x), t = static_cast<int>(threadIdx.x);
    const long long c0 = static_cast<long long>(tb.chunk_base) + tb.chunk0[i], c1 = static_cast<long long>(tb.chunk_base) + tb.chunk0[i + 1];
    double acc = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    long long fin = 0, zero = 0;
    for (long long c = c0 + t; c < c1; c += kWsThreads) {
        acc = acc + parts.sum[c];
        mn = fminf(mn, parts.mn[c]); mx = fmaxf(mx, parts.mx[c]);
        fin += parts.fin[c]; zero += parts.zero[c];
    }
    const double S = ws_block_add(acc, s_w);
    s_mn[t] = mn; s_mx[t] = mx; s_fin[t] = fin; s_zero[t] = zero;
    __syncthreads();
    if (t != 0) return;
    for (int j = 1; j < kWsThreads; ++j) {
        mn = fminf(mn, s_mn[j]); mx = fmaxf(mx, s_mx[j]);
        fin += s_fin[j]; zero += s_zero[j];
    }
    WatchRec rec;
    rec.mean = 0.0; rec.rlo = 0.f; rec.width = 0.f; rec.binned = 0; rec.pad = 0;
    unsigned long long* out = result + static_cast<long long>(tb.first + i) * words;
    double lo_d = 0.0, hi_d = 0.0;
    if (fin > 0) {
        float lo = mn, hi = mx;
        if (lo == 0.0f) lo = 0.0f;                             // -0.0 -> +0.0
        if (hi == 0.0f) hi = 0.0f;
        float rlo = lo, rhi = hi;
        if (lo == hi) {
            rlo = lo - 1.0f;
            if (rlo == lo) rlo = ws_below(lo);
            rhi = hi + 1.0f;
            if (rhi == hi) rhi = ws_above(hi);
        }
        const float width = rhi - rlo;
        rec.mean = S / static_cast<double>(fin);
        rec.rlo = rlo; rec.width = width;
        rec.binned = ws_finite(width) ? 1 : 0;
        lo_d = static_cast<double>(lo); hi_d = static_cast<double>(hi);
    }
    recs[tb.first + i] = rec;
    unsigned long long u;
    memcpy(&u, &lo_d, 8); out[kWsLo] = u;
    memcpy(&u, &hi_d, 8); out[kWsHi] = u;
    memcpy(&u, &rec.mean, 8); out[kWsMean] = u;
    out[kWsFinite] = static_cast<unsigned long long>(fin);
    out[kWsNonfinite] = static_cast<unsigned long long>(tb.n[i] - fin);
    out[kWsZero] = static_cast<unsigned long long>(zero);
}

// ---- pass 2: the bins and the squared deviations of a chunk -----------------------------------------------------------------
__global__ void __launch_bounds__(kWsThreads)
watch_pass2_kernel(WatchTable tb, WatchParts parts, const WatchRec* __restrict__ recs, unsigned long long* __restrict__ result,
                   int words, int bins) {
    __shared__ double s_w[kWsWaves];
    __shared__ int s_hist[kWsMaxBins];
    const int b = static_cast<int>(blockIdx.x), i = ws_find(tb, b), lane = static_cast<int>(threadIdx.x) & 63;
    const float* __restrict__ p = tb.p[i];
    const long long n = tb.n[i];
    const WatchRec rec = recs[tb.first + i];
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
    const long long chunk_at = static_cast<long long>(b - tb.chunk0[i]) * kWsChunk;
    const float fbins = static_cast<float>(bins);
    const bool binned = rec.binned != 0;                       // the same for the whole workgroup
    if (threadIdx.x < kWsMaxBins) s_hist[threadIdx.x] = 0;
    __syncthreads();
    double acc = 0.0;
    for (int k = 0; k < kWsSlabs; ++k) {
        const long long e0 = chunk_at + k * kWsSlab + 4 * static_cast<long long>(threadIdx.x);
        float v[4];
        if (e0 < n) ws_load4(p, e0, n, vec, v);
        else v[0] = v[1] = v[2] = v[3] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = v[j];
            const bool use = e0 + j < n && ws_finite(x);
            int bin = 0;
            if (use) {
                const double d = static_cast<double>(x) - rec.mean;
                const double dd = d * d;
                acc = acc + dd;
                const float num = x - rec.rlo;
                const float scaled = num * fbins;
                const float q = scaled / rec.width;
                bin = (q >= 0.0f && q < fbins + 1.0f) ? static_cast<int>(q) : 0;            // q infinite or NaN: bin 0
                if (bin == bins) bin = bins - 1;
            }
            if (binned) {
                // the lanes that hold the same bin add their number once; every lane of the wave is here
                unsigned long long todo = __ballot(use);
                while (todo != 0ull) {
                    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
                    const int lb = __shfl(bin, leader, 64);
                    const unsigned long long same = __ballot(use && bin == lb);
                    if (lane == leader) atomicAdd(&s_hist[lb], __popcll(same));
                    todo &= ~same;
                }
            }
        }
    }
    const double m2 = ws_block_add(acc, s_w);                  // its barriers also end the LDS adds
    if (threadIdx.x == 0) parts.m2[static_cast<long long>(tb.chunk_base) + b] = m2;
    if (binned && static_cast<int>(threadIdx.x) < bins) {
        const int c = s_hist[threadIdx.x];
        if (c != 0)
            atomicAdd(result + static_cast<long long>(tb.first + i) * words + kWsHead + threadIdx.x, static_cast<unsigned long long>(c));
    }
}

// ---- join 2: one workgroup per tensor of the launch -> m2 ---------------------------------------------------------------------
__global__ void __launch_bounds__(kWsThreads)
watch_join2_kernel(WatchTable tb, WatchParts parts, unsigned long long* __restrict__ result, int words) {
    __shared__ double s_w[kWsWaves];
    const int i = static_cast<int>(blockIdx.x), t = static_cast<int>(threadIdx.x);
    const long long c0 = static_cast<long long>(tb.chunk_base) + tb.chunk0[i], c1 = static_cast<long long>(tb.chunk_base) + tb.chunk0[i + 1];
    double acc = 0.0;
    for (long long c = c0 + t; c < c1; c += kWsThreads) acc = acc + parts.m2[c];
    const double m2 = ws_block_add(acc, s_w);
    if (t != 0) return;
    unsigned long long u;
    memcpy(&u, &m2, 8);
    result[static_cast<long long>(tb.first + i) * words + kWsM2] = u;
}

inline size_t ws_align256(size_t v) { return (v + 255) / 256 * 256; }
inline long long ws_chunks(long long n) { return (n + kWsChunk - 1) / kWsChunk; }

// -> the chunks of the call, or -1 where a count or the total is outside what one call takes
inline long long ws_total_chunks(const int64_t* counts, int T) {
    long long total = 0;
    for (int t = 0; t < T; ++t) {
        if (counts[t] < 0 || counts[t] > kWsMaxElems) return -1;
        total += ws_chunks(counts[t]);
        if (total > kWsMaxChunks) return -1;
    }
    return total;
}

inline size_t ws_bytes(long long chunks, int T) {
    // sum, m2 (8 bytes), min, max, finite, zero (4 bytes) per chunk, then one record per tensor
    return 2 * ws_align256(static_cast<size_t>(chunks) * 8) + 4 * ws_align256(static_cast<size_t>(chunks) * 4) +
           ws_align256(static_cast<size_t>(T) * sizeof(WatchRec));
}

}  // namespace qsae

using namespace qsae;

extern "C" size_t qsae_tensor_stats_workspace_bytes(const int64_t* counts, int T) {
    if (T < 0 || T > kWsMaxTensors || (T > 0 && !counts)) return 0;
    const long long chunks = ws_total_chunks(counts, T);
    if (chunks <= 0) return 0;
    return ws_bytes(chunks, T);
}

extern "C" int qsae_tensor_stats(const void* const* ptrs, const int64_t* counts, int T, int dtype, int bins, void* result,
                                 void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(T >= 0, "T >= 0 required");
    QSAE_CHECK_ARG(bins >= 1 && bins <= kWsMaxBins, "1 <= bins <= 256");
    QSAE_CHECK_SUPPORTED(dtype == 0, "dtype 0 (fp32)");
    QSAE_CHECK_SUPPORTED(T <= kWsMaxTensors, "T <= 65536");
    if (T == 0) return QSAE_OK;
    QSAE_CHECK_ARG(ptrs && counts, "null pointer");
    bool any = false;
    for (int t = 0; t < T; ++t) {
        QSAE_CHECK_ARG(counts[t] >= 0, "negative element count");
        QSAE_CHECK_ARG(counts[t] == 0 || ptrs[t], "null tensor pointer with a non-zero count");
        QSAE_CHECK_ARG(counts[t] == 0 || (reinterpret_cast<uintptr_t>(ptrs[t]) & 3u) == 0, "tensors must be 4-byte aligned");
        any = any || counts[t] > 0;
    }
    const long long chunks = ws_total_chunks(counts, T);
    QSAE_CHECK_SUPPORTED(chunks >= 0, "at most 2^40 elements per tensor and 2^30 chunks of 8192 elements per call");
    if (!any) return QSAE_OK;
    QSAE_CHECK_ARG(result && (reinterpret_cast<uintptr_t>(result) & 7u) == 0, "result must be non-null and 8-byte aligned");
    if (!workspace || workspace_bytes < ws_bytes(chunks, T) || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than qsae_tensor_stats_workspace_bytes", __func__);
    hipStream_t s = as_stream(stream);
    const int words = kWsHead + bins;
    unsigned long long* res = static_cast<unsigned long long*>(result);
    char* w = static_cast<char*>(workspace);
    WatchParts parts;
    parts.sum = reinterpret_cast<double*>(w);  w += ws_align256(static_cast<size_t>(chunks) * 8);
    parts.m2 = reinterpret_cast<double*>(w);   w += ws_align256(static_cast<size_t>(chunks) * 8);
    parts.mn = reinterpret_cast<float*>(w);    w += ws_align256(static_cast<size_t>(chunks) * 4);
    parts.mx = reinterpret_cast<float*>(w);    w += ws_align256(static_cast<size_t>(chunks) * 4);
    parts.fin = reinterpret_cast<int*>(w);     w += ws_align256(static_cast<size_t>(chunks) * 4);
    parts.zero = reinterpret_cast<int*>(w);    w += ws_align256(static_cast<size_t>(chunks) * 4);
    WatchRec* recs = reinterpret_cast<WatchRec*>(w);
    QSAE_HIP(hipMemsetAsync(result, 0, static_cast<size_t>(T) * words * 8, s));
    // groups of up to kWsTable tensors whose workgroups fit one grid; pass 1 and its join of every group first, then pass 2
    for (int pass = 0; pass < 2; ++pass) {
        long long chunk_base = 0;
        for (int first = 0; first < T; first += kWsTable) {
            WatchTable tb;
            tb.count = T - first < kWsTable ? T - first : kWsTable;
            tb.first = first;
            tb.chunk_base = static_cast<int>(chunk_base);
            long long at = 0;
            for (int i = 0; i < kWsTable; ++i) {
                const bool in = i < tb.count;
                tb.p[i] = in ? static_cast<const float*>(ptrs[first + i]) : nullptr;
                tb.n[i] = in ? counts[first + i] : 0;
                tb.chunk0[i] = static_cast<int>(at);
                at += ws_chunks(tb.n[i]);
            }
            tb.chunk0[kWsTable] = static_cast<int>(at);
            const dim3 block(kWsThreads), per_tensor(tb.count);
            if (pass == 0) {
                if (at > 0) {
                    hipLaunchKernelGGL(watch_pass1_kernel, dim3(static_cast<unsigned>(at)), block, 0, s, tb, parts);
                    QSAE_LAUNCH_CHECK();
                }
                hipLaunchKernelGGL(watch_join1_kernel, per_tensor, block, 0, s, tb, parts, recs, res, words);
                QSAE_LAUNCH_CHECK();
            } else if (at > 0) {
                hipLaunchKernelGGL(watch_pass2_kernel, dim3(static_cast<unsigned>(at)), block, 0, s, tb, parts,
                                   static_cast<const WatchRec*>(recs), res, words, bins);
                QSAE_LAUNCH_CHECK();
                hipLaunchKernelGGL(watch_join2_kernel, per_tensor, block, 0, s, tb, parts, res, words);
                QSAE_LAUNCH_CHECK();
            }
            chunk_base += at;
        }
    }
    return QSAE_OK;
}
