// trainer.hip -- what the training loop does around forward_train (training/trainer.py:73-173):
// which rows of a resident chunk hold a NaN (qsae_rows_nan_bitmap, once per chunk instead of isnan().any() per step), the
// shuffled batch gathered from the chunk and widened to fp32 (qsae_gather_rows, instead of 8192 __getitem__ calls and a
// collate), and the reconstruction losses of every level with their gradients in one pass (qsae_trainer_loss, instead of
// one mse_loss and its backward per level).
//
// No float atomics anywhere; the order of every sum is a function of the shapes alone (and of the constants below), so
// the same input gives the same bits on every run.
#include "common.h"

// elements of one workgroup of qsae_trainer_loss = 256 threads x 4 elements x this many slabs
#ifndef QSAE_TRAINER_LOSS_SLABS
#define QSAE_TRAINER_LOSS_SLABS 4
#endif

namespace qsae {

constexpr int kTrWaves = 4;                    // waves of a workgroup, everywhere in this file
constexpr int kTrThreads = 64 * kTrWaves;
constexpr int kNanRowsPerWave = 8;             // 4 waves x 8 rows = the 32 rows of one bitmap word
constexpr int kLossMaxLevels = 8;
constexpr long long kLossSlab = kTrThreads * 4;                       // elements of one slab: 4 consecutive per thread
constexpr long long kLossBlockElems = kLossSlab * QSAE_TRAINER_LOSS_SLABS;

enum TrType { kTrF32 = 0, kTrF16 = 1, kTrBF16 = 2 };

// ---- NaN tests on the stored bits (no conversion; inf is not NaN) ---------------------------------------------------
template <int T>
__device__ __forceinline__ bool word_has_nan(uint32_t w) {
    if constexpr (T == kTrF32) {
        return (w & 0x7FFFFFFFu) > 0x7F800000u;
    } else {
        constexpr uint32_t inf = T == kTrF16 ? 0x7C00u : 0x7F80u;      // two 16-bit elements per word
        return (w & 0x7FFFu) > inf || ((w >> 16) & 0x7FFFu) > inf;
    }
}
template <int T>
__device__ __forceinline__ bool elem_is_nan(const void* src, size_t i) {
    if constexpr (T == kTrF32) {
        return (static_cast<const uint32_t*>(src)[i] & 0x7FFFFFFFu) > 0x7F800000u;
    } else {
        constexpr uint32_t inf = T == kTrF16 ? 0x7C00u : 0x7F80u;
        return (static_cast<const unsigned short*>(src)[i] & 0x7FFFu) > inf;
    }
}

// One workgroup per bitmap word: wave w takes the rows 32 word + 8 w .. + 7 one after another, lane l the 16-byte pieces
// l, l + 64, ... of a row (VEC: every row starts on a 16-byte boundary and is a whole number of pieces) or the elements
// l, l + 64, ...; a ballot joins the lanes.  Thread 0 stores the word: every word is written exactly once, rows at or
// past n_rows give 0 bits and are never read.
template <int T, bool VEC>
__global__ void __launch_bounds__(kTrThreads)
rows_nan_bitmap_kernel(const void* __restrict__ src, long long n_rows, int D, uint32_t* __restrict__ bits) {
    __shared__ uint32_t s_part[kTrWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr size_t esize = T == kTrF32 ? 4 : 2;
    const size_t row_bytes = static_cast<size_t>(D) * esize;
    uint32_t mine = 0;
    for (int j = 0; j < kNanRowsPerWave; ++j) {
        const long long row = static_cast<long long>(blockIdx.x) * 32 + wave * kNanRowsPerWave + j;
        bool nan = false;
        if (row < n_rows) {
            if (VEC) {
                const uint4* p = reinterpret_cast<const uint4*>(static_cast<const char*>(src) + static_cast<size_t>(row) * row_bytes);
                const int pieces = static_cast<int>(row_bytes >> 4);
                for (int c = lane; c < pieces; c += 64) {
                    const uint4 q = p[c];
                    nan = nan || word_has_nan<T>(q.x) || word_has_nan<T>(q.y) || word_has_nan<T>(q.z) || word_has_nan<T>(q.w);
                }
            } else {
                const size_t base = static_cast<size_t>(row) * D;
                for (int d = lane; d < D; d += 64) nan = nan || elem_is_nan<T>(src, base + d);
            }
        }
        if (__ballot(nan) != 0ull) mine |= 1u << (wave * kNanRowsPerWave + j);
    }
    if (lane == 0) s_part[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) bits[blockIdx.x] = s_part[0] | s_part[1] | s_part[2] | s_part[3];
}

// ---- gather ---------------------------------------------------------------------------------------------------------
// u: the 16 stored bits.  The widening is exact for every value; of the NaNs, bf16 ones keep sign and payload and fp16
// ones do when they are quiet (the conversion instruction quiets a signalling NaN).
template <int T>
__device__ __forceinline__ float half_bits_to_float(uint32_t u) {
    if constexpr (T == kTrF16) {
        const unsigned short us = static_cast<unsigned short>(u);
        _Float16 hv;
        memcpy(&hv, &us, 2);
        return static_cast<float>(hv);
    } else {
        return __uint_as_float(u << 16);
    }
}

// One wave per output row.  VEC: lane l takes the 16-byte pieces l, l + 64, ... of the source row (4 fp32 or 8 16-bit
// elements) and stores one or two 16-byte pieces of out; otherwise element by element.  An index outside [0, n_rows) is
// not dereferenced: the row is written as zeros and lane 0 ORs bit 0 into *flag.
template <int T, bool VEC>
__global__ void __launch_bounds__(kTrThreads)
gather_rows_kernel(const void* __restrict__ src, long long n_rows, int D, const long long* __restrict__ idx, int B,
                   float* __restrict__ out, uint32_t* __restrict__ flag) {
    const int b = blockIdx.x * kTrWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const long long r = idx[b];
    const bool ok = r >= 0 && r < n_rows;
    float* o = out + static_cast<size_t>(b) * D;
    if (!ok && lane == 0) atomicOr(flag, 1u);
    if (VEC) {
        constexpr int per = T == kTrF32 ? 4 : 8;                           // elements of one 16-byte source piece
        const int pieces = D / per;
        const uint4* p = reinterpret_cast<const uint4*>(static_cast<const char*>(src) +
                                                        (ok ? static_cast<size_t>(r) : 0) * D * (T == kTrF32 ? 4 : 2));
        uint4* q = reinterpret_cast<uint4*>(o);
        for (int c = lane; c < pieces; c += 64) {
            const uint4 v = ok ? p[c] : make_uint4(0u, 0u, 0u, 0u);
            if constexpr (T == kTrF32) {
                q[c] = v;
            } else {
                q[2 * c] = make_uint4(__float_as_uint(half_bits_to_float<T>(v.x & 0xFFFFu)), __float_as_uint(half_bits_to_float<T>(v.x >> 16)),
                                      __float_as_uint(half_bits_to_float<T>(v.y & 0xFFFFu)), __float_as_uint(half_bits_to_float<T>(v.y >> 16)));
                q[2 * c + 1] = make_uint4(__float_as_uint(half_bits_to_float<T>(v.z & 0xFFFFu)), __float_as_uint(half_bits_to_float<T>(v.z >> 16)),
                                          __float_as_uint(half_bits_to_float<T>(v.w & 0xFFFFu)), __float_as_uint(half_bits_to_float<T>(v.w >> 16)));
            }
        }
    } else {
        const size_t base = (ok ? static_cast<size_t>(r) : 0) * D;
        for (int d = lane; d < D; d += 64) {
            float v = 0.f;
            if (ok) {
                if constexpr (T == kTrF32) v = static_cast<const float*>(src)[base + d];
                else v = half_bits_to_float<T>(static_cast<const unsigned short*>(src)[base + d]);
            }
            o[d] = v;
        }
    }
}

// ---- loss and gradient ----------------------------------------------------------------------------------------------
struct LossPtrs {
    const float* r[kLossMaxLevels];
    float* g[kLossMaxLevels];
};

__device__ __forceinline__ double tr_wave_add(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

// the 64 lane sums by a butterfly (xor 32, 16, ..., 1), then the 4 wave sums in ascending wave order; the result is
// valid in thread 0.  Every thread of the workgroup comes here.
__device__ __forceinline__ double tr_block_add(double v, double* s_w) {
    v = tr_wave_add(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = s_w[0];
        for (int w = 1; w < kTrWaves; ++w) r = r + s_w[w];
    }
    __syncthreads();
    return r;
}

// Workgroup b owns the elements [b T, (b + 1) T), T = kLossBlockElems, in slabs of 1024: thread t takes the 4 consecutive
// elements 4 t .. 4 t + 3 of every slab (one 16-byte load per tensor when VEC, 4 scalar loads otherwise: the same
// elements in the same order, hence the same bits) and adds fp64(fp32((r - t)^2)) per level in ascending (slab, element)
// order.  partials[level][b] = the workgroup's sum by tr_block_add.  Every line below is one IEEE fp32 operation (the
// build passes -ffp-contract=off).
template <int NL, bool VEC>
__global__ void __launch_bounds__(kTrThreads)
trainer_loss_kernel(const float* __restrict__ x, LossPtrs ptrs, long long N, int mode, float s, double* __restrict__ partials) {
    __shared__ double s_w[kTrWaves];
    double acc[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) acc[i] = 0.0;
    const long long block0 = static_cast<long long>(blockIdx.x) * kLossBlockElems;
    for (int k = 0; k < QSAE_TRAINER_LOSS_SLABS; ++k) {
        const long long e0 = block0 + k * kLossSlab + 4 * static_cast<long long>(threadIdx.x);
        if (e0 >= N) break;
        const bool whole = e0 + 3 < N;
        float t[4];
        if (VEC && whole) {
            const uint4 q = *reinterpret_cast<const uint4*>(x + e0);
            t[0] = __uint_as_float(q.x); t[1] = __uint_as_float(q.y); t[2] = __uint_as_float(q.z); t[3] = __uint_as_float(q.w);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = e0 + j < N ? x[e0 + j] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            float r[4], g[4];
            if (VEC && whole) {
                const uint4 q = *reinterpret_cast<const uint4*>(ptrs.r[i] + e0);
                r[0] = __uint_as_float(q.x); r[1] = __uint_as_float(q.y); r[2] = __uint_as_float(q.z); r[3] = __uint_as_float(q.w);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = e0 + j < N ? ptrs.r[i][e0 + j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = r[j] - t[j];
                g[j] = d * s;
                const float sq = d * d;
                if (e0 + j < N) acc[i] = acc[i] + static_cast<double>(sq);
                if (mode == 1) {                                        // the rq_sae chain: qsae_residual_update's arithmetic
                    const float u = t[j] - r[j];
                    t[j] = u * 2.0f;
                }
            }
            if (VEC && whole) {
                *reinterpret_cast<uint4*>(ptrs.g[i] + e0) = make_uint4(__float_as_uint(g[0]), __float_as_uint(g[1]),
                                                                      __float_as_uint(g[2]), __float_as_uint(g[3]));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e0 + j < N) ptrs.g[i][e0 + j] = g[j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const double sum = tr_block_add(acc[i], s_w);
        if (threadIdx.x == 0) partials[static_cast<long long>(i) * gridDim.x + blockIdx.x] = sum;
    }
}

// One workgroup per level: thread t adds the partials t, t + 256, ... in ascending order, tr_block_add joins the threads,
// losses[level] = fp32((coef * S) / N) with both operations in fp64.
__global__ void __launch_bounds__(kTrThreads)
trainer_loss_join_kernel(const double* __restrict__ partials, int blocks, double coef, double count, float* __restrict__ losses) {
    __shared__ double s_w[kTrWaves];
    const double* p = partials + static_cast<long long>(blockIdx.x) * blocks;
    double acc = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kTrThreads) acc = acc + p[b];
    const double S = tr_block_add(acc, s_w);
    if (threadIdx.x == 0) {
        const double cs = coef * S;
        losses[blockIdx.x] = static_cast<float>(cs / count);
    }
}

inline size_t tr_align256(size_t v) { return (v + 255) / 256 * 256; }

template <int NL>
void launch_trainer_loss(bool vec, unsigned blocks, hipStream_t st, const float* x, const LossPtrs& ptrs, long long N, int mode,
                         float s, double* partials) {
    if (vec) hipLaunchKernelGGL((trainer_loss_kernel<NL, true>), dim3(blocks), dim3(kTrThreads), 0, st, x, ptrs, N, mode, s, partials);
    else hipLaunchKernelGGL((trainer_loss_kernel<NL, false>), dim3(blocks), dim3(kTrThreads), 0, st, x, ptrs, N, mode, s, partials);
}

}  // namespace qsae

using namespace qsae;

static bool tr_dtype_ok(int dtype) { return dtype == kTrF32 || dtype == kTrF16 || dtype == kTrBF16; }
static size_t tr_esize(int dtype) { return dtype == kTrF32 ? 4 : 2; }
// the bitmap's workgroups (one per word) ride on gridDim.x
static const long long kTrMaxRows = 32ll * 0x7FFFFFFFll;

extern "C" int qsae_rows_nan_bitmap(const void* src, int dtype, int64_t n_rows, int D, uint32_t* bits, qsae_stream_t stream) {
    QSAE_CHECK_ARG(n_rows >= 0 && D > 0, "n_rows >= 0 and D > 0 required");
    QSAE_CHECK_SUPPORTED(tr_dtype_ok(dtype), "dtype 0 (fp32), 1 (fp16) or 2 (bf16)");
    QSAE_CHECK_SUPPORTED(n_rows <= kTrMaxRows, "n_rows <= 32 * (2^31 - 1)");
    if (n_rows == 0) return QSAE_OK;
    QSAE_CHECK_ARG(src && bits, "null pointer");
    const size_t esize = tr_esize(dtype);
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(src) & (esize - 1)) == 0 && (reinterpret_cast<uintptr_t>(bits) & 3u) == 0,
                   "src must be aligned to its element, bits to 4 bytes");
    const bool vec = aligned16(src) && (static_cast<size_t>(D) * esize) % 16 == 0;
    const dim3 grid(static_cast<unsigned>((n_rows + 31) / 32)), block(kTrThreads);
    hipStream_t s = as_stream(stream);
    const long long n = n_rows;
#define QSAE_TR_NAN(T)                                                                                                 \
    do {                                                                                                               \
        if (vec) hipLaunchKernelGGL((rows_nan_bitmap_kernel<T, true>), grid, block, 0, s, src, n, D, bits);            \
        else hipLaunchKernelGGL((rows_nan_bitmap_kernel<T, false>), grid, block, 0, s, src, n, D, bits);               \
    } while (0)
    switch (dtype) {
        case kTrF32: QSAE_TR_NAN(kTrF32); break;
        case kTrF16: QSAE_TR_NAN(kTrF16); break;
        default: QSAE_TR_NAN(kTrBF16); break;
    }
#undef QSAE_TR_NAN
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_gather_rows(const void* src, int dtype, int64_t n_rows, int D, const int64_t* idx, int B, float* out,
                                uint32_t* flag, qsae_stream_t stream) {
    QSAE_CHECK_ARG(n_rows >= 0 && D > 0 && B >= 0, "n_rows >= 0, D > 0 and B >= 0 required");
    QSAE_CHECK_SUPPORTED(tr_dtype_ok(dtype), "dtype 0 (fp32), 1 (fp16) or 2 (bf16)");
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(idx && out && flag && (src || n_rows == 0), "null pointer");
    const size_t esize = tr_esize(dtype);
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(src) & (esize - 1)) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(idx) & 7u) == 0 && (reinterpret_cast<uintptr_t>(flag) & 3u) == 0,
                   "src, out and flag must be aligned to their element, idx to 8 bytes");
    // whole 16-byte pieces on both sides: source rows of 4 fp32 / 8 16-bit elements per piece, out rows of 4 floats
    const bool vec = aligned16(src) && aligned16(out) && (static_cast<size_t>(D) * esize) % 16 == 0;
    const dim3 grid((static_cast<unsigned>(B) + kTrWaves - 1) / kTrWaves), block(kTrThreads);
    hipStream_t s = as_stream(stream);
    const long long n = n_rows;
    const long long* ix = reinterpret_cast<const long long*>(idx);
#define QSAE_TR_GATHER(T)                                                                                              \
    do {                                                                                                               \
        if (vec) hipLaunchKernelGGL((gather_rows_kernel<T, true>), grid, block, 0, s, src, n, D, ix, B, out, flag);    \
        else hipLaunchKernelGGL((gather_rows_kernel<T, false>), grid, block, 0, s, src, n, D, ix, B, out, flag);       \
    } while (0)
    switch (dtype) {
        case kTrF32: QSAE_TR_GATHER(kTrF32); break;
        case kTrF16: QSAE_TR_GATHER(kTrF16); break;
        default: QSAE_TR_GATHER(kTrBF16); break;
    }
#undef QSAE_TR_GATHER
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

static bool trainer_loss_shape_ok(int n, int B, int D) {
    // the workgroups ride on gridDim.x
    return n >= 0 && n <= kLossMaxLevels && B >= 0 && D > 0 &&
           (static_cast<long long>(B) * D + kLossBlockElems - 1) / kLossBlockElems <= 0x7FFFFFFFll;
}

extern "C" size_t qsae_trainer_loss_workspace_bytes(int n, int B, int D) {
    if (!trainer_loss_shape_ok(n, B, D)) return 0;
    const size_t blocks = static_cast<size_t>((static_cast<long long>(B) * D + kLossBlockElems - 1) / kLossBlockElems);
    return tr_align256(static_cast<size_t>(n) * blocks * 8);
}

extern "C" int qsae_trainer_loss(const float* x, const float* const* recon_ptrs, int n, int B, int D, int mode, double coef,
                                 float* const* grads_ptrs, float* losses, void* workspace, size_t workspace_bytes,
                                 qsae_stream_t stream) {
    QSAE_CHECK_ARG(n >= 0 && B >= 0 && D > 0, "n >= 0, B >= 0 and D > 0 required");
    QSAE_CHECK_SUPPORTED(n <= kLossMaxLevels, "n <= 8");
    QSAE_CHECK_SUPPORTED(mode == 0 || mode == 1, "mode 0 (every level against x) or 1 (the doubled residual chain)");
    QSAE_CHECK_SUPPORTED(trainer_loss_shape_ok(n, B, D), "B * D too large for one launch");
    if (n == 0 || B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(x && recon_ptrs && grads_ptrs && losses, "null pointer");
    LossPtrs ptrs;
    bool vec = aligned16(x);
    for (int i = 0; i < kLossMaxLevels; ++i) {
        ptrs.r[i] = i < n ? recon_ptrs[i] : nullptr;
        ptrs.g[i] = i < n ? grads_ptrs[i] : nullptr;
        if (i < n) {
            QSAE_CHECK_ARG(ptrs.r[i] && ptrs.g[i], "null reconstruction or gradient pointer");
            QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(ptrs.r[i]) & 3u) == 0 && (reinterpret_cast<uintptr_t>(ptrs.g[i]) & 3u) == 0,
                           "reconstructions and gradients must be 4-byte aligned");
            vec = vec && aligned16(ptrs.r[i]) && aligned16(ptrs.g[i]);
        }
    }
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(losses) & 3u) == 0,
                   "x and losses must be 4-byte aligned");
    if (!workspace || workspace_bytes < qsae_trainer_loss_workspace_bytes(n, B, D) || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than qsae_trainer_loss_workspace_bytes", __func__);
    const long long N = static_cast<long long>(B) * D;
    const unsigned blocks = static_cast<unsigned>((N + kLossBlockElems - 1) / kLossBlockElems);
    const float s = static_cast<float>(2.0 * coef / static_cast<double>(N));
    double* partials = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    switch (n) {
        case 1: launch_trainer_loss<1>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
        case 2: launch_trainer_loss<2>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
        case 3: launch_trainer_loss<3>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
        case 4: launch_trainer_loss<4>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
        case 5: launch_trainer_loss<5>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
        case 6: launch_trainer_loss<6>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
        case 7: launch_trainer_loss<7>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
        default: launch_trainer_loss<8>(vec, blocks, st, x, ptrs, N, mode, s, partials); break;
    }
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(trainer_loss_join_kernel, dim3(n), dim3(kTrThreads), 0, st, static_cast<const double*>(partials),
                       static_cast<int>(blocks), coef, static_cast<double>(N), losses);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}
