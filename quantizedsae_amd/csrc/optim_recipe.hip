// optim_recipe.hip -- what the top-k SAE papers put around the Adam step (include/qsae_optim.h):
// qsaeo_grad_norm, the joint gradient norm in fp64 and its clip coefficient as one device word; qsaeo_adam_step and
// qsaeo_adam_step_prefilter, the steps of optim.hip with that word as a factor of the gradient and an exponential moving
// average of the weights as one more stream of the same pass; qsaeo_project_columns, which removes from the decoder
// gradient its component parallel to each atom.  No float atomics; every sum has the fixed order the header states.
#include "adam_elem.h"
#include "../../include/qsae_optim.h"
#include <math.h>

// workgroups of one qsaeo_adam_step launch at the most (qsae_adam_step's cap)
#ifndef QSAE_ADAM_MAX_BLOCKS
#define QSAE_ADAM_MAX_BLOCKS 4096
#endif

namespace qsae {

// ---- the flat step ----------------------------------------------------------------------------------------------------
// One element of the recipe: the clip coefficient (one multiplication), the step, the average.
template <bool COEF, bool EMA>
__device__ __forceinline__ void recipe_elem(float& p, float g, float& m, float& v, float& e, const AdamScalars& a, float c,
                                            float omd) {
    if (COEF) g = g * c;
    adam_elem(p, g, m, v, a);
    if (EMA) ema_elem(e, p, omd);
}

// adam_step_kernel of optim.hip with the two optional streams.  VEC: p, g, m, v (and ema) 16-byte aligned, four elements
// per load; otherwise one.  The elements past the last whole vector are taken one by one by the first workgroup.
template <bool VEC, bool COEF, bool EMA>
__global__ void __launch_bounds__(256)
recipe_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                   long long n, AdamScalars a, const float* __restrict__ coef, float* __restrict__ ema, float omd) {
    const long long tid = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long stride = static_cast<long long>(gridDim.x) * 256;
    const float c = COEF ? *coef : 1.0f;
    float none = 0.f;
    if (VEC) {
        const long long n4 = n >> 2;
        for (long long i = tid; i < n4; i += stride) {
            f32x4 pp = reinterpret_cast<f32x4*>(p)[i], mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
            const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
            f32x4 ee = pp;
            if (EMA) ee = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = pp[j], mj = mm[j], vj = vv[j], ej = ee[j];
                recipe_elem<COEF, EMA>(pj, gg[j], mj, vj, ej, a, c, omd);
                pp[j] = pj; mm[j] = mj; vv[j] = vj; ee[j] = ej;
            }
            reinterpret_cast<f32x4*>(p)[i] = pp;
            reinterpret_cast<f32x4*>(m)[i] = mm;
            reinterpret_cast<f32x4*>(v)[i] = vv;
            if (EMA) reinterpret_cast<f32x4*>(ema)[i] = ee;
        }
        const long long i = (n4 << 2) + tid;          // tail: at most 3 elements
        if (tid < 4 && i < n) recipe_elem<COEF, EMA>(p[i], g[i], m[i], v[i], EMA ? ema[i] : none, a, c, omd);
    } else {
        for (long long i = tid; i < n; i += stride)
            recipe_elem<COEF, EMA>(p[i], g[i], m[i], v[i], EMA ? ema[i] : none, a, c, omd);
    }
}

// ---- the encoder pair of a top-k model ------------------------------------------------------------------------------
// (A) of optim.hip with the two streams: one wave per hidden unit, lane l takes d = l, l + 64, ...; the new values enter
// pack_w's statistics from the registers they were just stored from.
template <bool COEF, bool EMA>
__global__ void __launch_bounds__(256)
recipe_pref_update_kernel(float* __restrict__ W, const float* __restrict__ gW, float* __restrict__ mW, float* __restrict__ vW,
                          float* __restrict__ bias, const float* __restrict__ gb, float* __restrict__ mb,
                          float* __restrict__ vb, int H, int D, AdamScalars a, const float* __restrict__ coef,
                          float* __restrict__ emaW, float* __restrict__ emab, float omd, unsigned* __restrict__ meta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float c = COEF ? *coef : 1.0f;
    float mx = 0.f, ss = 0.f, babs = 0.f;
    if (row < H) {
        const int64_t base = static_cast<int64_t>(row) * D;
#pragma unroll 4
        for (int d = lane; d < D; d += 64) {
            float w = W[base + d], m = mW[base + d], v = vW[base + d], e = 0.f;
            if (EMA) e = emaW[base + d];
            recipe_elem<COEF, EMA>(w, gW[base + d], m, v, e, a, c, omd);
            W[base + d] = w; mW[base + d] = m; vW[base + d] = v;
            if (EMA) emaW[base + d] = e;
            pref_w_stat_step(w, mx, ss);
        }
        pref_w_stat_join(mx, ss);
        if (bias && lane == 0) {
            float b = bias[row], m = mb[row], v = vb[row], e = 0.f;
            if (EMA) e = emab[row];
            recipe_elem<COEF, EMA>(b, gb[row], m, v, e, a, c, omd);
            bias[row] = b; mb[row] = m; vb[row] = v;
            if (EMA) emab[row] = e;
            babs = fabsf(b);
        }
    }
    block_max3(__float_as_uint(mx), __float_as_uint(babs), __float_as_uint(row < H ? pref_w_row_norm(ss) : 0.f),
               &meta[0], bias ? &meta[2] : nullptr, &meta[1]);
}

// (B) of optim.hip: the row's fp16 copy under sw = pow2_scale_for(max |W'|) and its distance from the row
__global__ void __launch_bounds__(256)
recipe_pref_cast_err_kernel(const float* __restrict__ W, int H, int D, const float* __restrict__ meta_in,
                            _Float16* __restrict__ Wq, unsigned* __restrict__ err_out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float sw = pow2_scale_for(meta_in[0]);
    const bool usable = sw > 0.f;                 // non-finite weights: every row is flagged anyway, meta[3] stays 0
    float ff = 0.f;
    if (row < H) {
        const int64_t base = static_cast<int64_t>(row) * D;
        const float back = usable ? 1.0f / sw : 0.f;
#pragma unroll 4
        for (int d = lane; d < D; d += 64) {
            const float w = W[base + d];
            Wq[base + d] = pref_w_cast(w, sw);
            if (usable) pref_w_err_step(w, sw, back, ff);
        }
        ff = pref_w_err_join(ff);
    }
    const unsigned e = (usable && row < H) ? __float_as_uint(pref_w_row_err(ff)) : 0u;
    block_max3(e, 0u, 0u, err_out, nullptr, nullptr);
}

// meta[0]: max |W'| -> the scale every wave of (B) derived from it
__global__ void recipe_pref_finish_kernel(float* __restrict__ meta) {
    if (threadIdx.x == 0 && blockIdx.x == 0) meta[0] = pow2_scale_for(meta[0]);
}

// ---- the projection of the decoder gradient --------------------------------------------------------------------------
// A workgroup owns a strip of kPjCols = 64 columns: thread t holds the four columns 4 (t & 15) .. + 3 of the strip (one
// 16-byte load per row and matrix) and walks the rows of chain r = t >> 4, d = r, r + 16, ...: a wave reads 4 rows of 256
// contiguous bytes per trip.  The 16 chains of a column meet in LDS and every thread adds them in ascending r; the second
// walk over the strip rewrites G.  At 512 x 32768 that is 512 workgroups with 32 trips a thread; the strip's second read
// is served by whichever cache still holds it (two matrices of 128 KiB per workgroup).
constexpr int kPjGroups = QSAEO_PROJECT_GROUPS;
constexpr int kPjQuads = 16;
constexpr int kPjCols = 4 * kPjQuads;

__global__ void __launch_bounds__(256)
project_columns_kernel(const float* __restrict__ W, float* __restrict__ G, int D, int H, int64_t ld) {
    __shared__ f32x4 s_part[kPjGroups][kPjQuads];
    const int quad = threadIdx.x & (kPjQuads - 1), r = threadIdx.x >> 4;
    const int64_t col = static_cast<int64_t>(blockIdx.x) * kPjCols + 4 * quad;
    const bool live = col < H;                               // H is a multiple of 4: a quad is inside or outside
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        for (int d = r; d < D; d += kPjGroups) {
            const int64_t at = static_cast<int64_t>(d) * ld + col;
            const f32x4 w = *reinterpret_cast<const f32x4*>(W + at), g = *reinterpret_cast<const f32x4*>(G + at);
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = fmaf(g[j], w[j], c[j]);
        }
    }
    s_part[r][quad] = c;
    __syncthreads();
    if (!live) return;
    f32x4 dot = s_part[0][quad];
    for (int k = 1; k < kPjGroups; ++k) {
        const f32x4 o = s_part[k][quad];
#pragma unroll
        for (int j = 0; j < 4; ++j) dot[j] = dot[j] + o[j];
    }
    if (dot[0] == 0.f && dot[1] == 0.f && dot[2] == 0.f && dot[3] == 0.f) return;      // nothing of this quad changes
    for (int d = r; d < D; d += kPjGroups) {
        const int64_t at = static_cast<int64_t>(d) * ld + col;
        const f32x4 w = *reinterpret_cast<const f32x4*>(W + at);
        f32x4 g = *reinterpret_cast<const f32x4*>(G + at);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = dot[j] == 0.f ? g[j] : fmaf(-dot[j], w[j], g[j]);
        *reinterpret_cast<f32x4*>(G + at) = g;
    }
}

// ---- the joint gradient norm ---------------------------------------------------------------------------------------------
// The layout of watch.hip's passes: a workgroup of 256 threads owns a chunk of 8192 elements in 8 slabs of 1024, thread
// j the elements 4 j .. 4 j + 3 of every slab; workgroups find their (tensor, chunk) through a table of chunk prefix counts
// that travels in the kernel arguments, 32 tensors per launch.
constexpr int kGnWaves = 4;
constexpr int kGnThreads = 64 * kGnWaves;
constexpr int kGnSlabs = 8;
constexpr long long kGnSlab = kGnThreads * 4;
constexpr long long kGnChunk = kGnSlab * kGnSlabs;
constexpr int kGnTable = 32;
constexpr int kGnMaxTensors = 65536;
constexpr long long kGnMaxElems = 1ll << 40;
constexpr long long kGnMaxChunks = 1ll << 30;
constexpr int kGnHead = QSAEO_NORM_HEAD;

struct NormTable {
    const float* p[kGnTable];
    long long n[kGnTable];
    int chunk0[kGnTable + 1];         // first workgroup of tensor i in this launch; chunk0[count] = the launch's workgroups
    int count;                        // tensors of this launch
    int first;                        // index of tensor 0 of this launch in the call's list
    int chunk_base;                   // index of workgroup 0's chunk among the call's chunks
};

// the 64 lane sums by a butterfly, then the 4 wave sums in ascending wave order; valid in thread 0
__device__ __forceinline__ double gn_block_add(double v, double* s_w) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = s_w[0];
        for (int w = 1; w < kGnWaves; ++w) r = r + s_w[w];
    }
    return r;
}

// the tensor of workgroup b: the largest i < count with chunk0[i] <= b (tensors without elements own no workgroup)
__device__ __forceinline__ int gn_find(const NormTable& tb, int b) {
    int i = 0;
    for (int step = kGnTable / 2; step >= 1; step >>= 1)
        if (i + step < tb.count && tb.chunk0[i + step] <= b) i += step;
    return i;
}

__global__ void __launch_bounds__(kGnThreads)
grad_norm_pass_kernel(NormTable tb, double* __restrict__ parts) {
    __shared__ double s_w[kGnWaves];
    const int b = static_cast<int>(blockIdx.x), i = gn_find(tb, b);
    const float* __restrict__ p = tb.p[i];
    const long long n = tb.n[i];
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
    const long long chunk_at = static_cast<long long>(b - tb.chunk0[i]) * kGnChunk;
    double acc = 0.0;
    for (int k = 0; k < kGnSlabs; ++k) {
        const long long e0 = chunk_at + k * kGnSlab + 4 * static_cast<long long>(threadIdx.x);
        if (e0 >= n) break;
        float x[4];
        if (vec && e0 + 3 < n) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p + e0);
            x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = e0 + j < n ? p[e0 + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e0 + j < n) {
                const double xd = static_cast<double>(x[j]);
                const double sq = xd * xd;
                acc = acc + sq;
            }
        }
    }
    const double sum = gn_block_add(acc, s_w);
    if (threadIdx.x == 0) parts[static_cast<long long>(tb.chunk_base) + b] = sum;
}

// one workgroup per tensor of the launch -> the tensor's sum of squares
__global__ void __launch_bounds__(kGnThreads)
grad_norm_join_kernel(NormTable tb, const double* __restrict__ parts, double* __restrict__ report) {
    __shared__ double s_w[kGnWaves];
    const int i = static_cast<int>(blockIdx.x), t = static_cast<int>(threadIdx.x);
    const long long c0 = static_cast<long long>(tb.chunk_base) + tb.chunk0[i], c1 = static_cast<long long>(tb.chunk_base) + tb.chunk0[i + 1];
    double acc = 0.0;
    for (long long c = c0 + t; c < c1; c += kGnThreads) acc = acc + parts[c];
    const double S = gn_block_add(acc, s_w);
    if (t == 0) report[kGnHead + tb.first + i] = S;
}

// the tensors' sums in ascending order, the norm and the coefficient: one thread
__global__ void grad_norm_finish_kernel(double* __restrict__ report, int T, double max_norm, float* __restrict__ coef) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double total = 0.0;
    for (int t = 0; t < T; ++t) total = total + report[kGnHead + t];
    const double norm = sqrt(total);
    const double den = norm + 1e-6;
    const double c = max_norm / den;
    float cf;
    if (c >= 1.0) cf = 1.0f;
    else if (c != c) cf = __uint_as_float(0x7FC00000u);
    else cf = static_cast<float>(c);
    *coef = cf;
    report[0] = total;
    report[1] = norm;
    report[2] = static_cast<double>(cf);
    reinterpret_cast<long long*>(report)[3] = (cf == 1.0f) ? 0ll : 1ll;
}

inline size_t gn_align256(size_t v) { return (v + 255) / 256 * 256; }
inline long long gn_chunks(long long n) { return (n + kGnChunk - 1) / kGnChunk; }

// -> the chunks of the call, or -1 where a count or the total is outside what one call takes
inline long long gn_total_chunks(const int64_t* counts, int T) {
    long long total = 0;
    for (int t = 0; t < T; ++t) {
        if (counts[t] < 0 || counts[t] > kGnMaxElems) return -1;
        total += gn_chunks(counts[t]);
        if (total > kGnMaxChunks) return -1;
    }
    return total;
}
inline size_t gn_bytes(long long chunks) { return gn_align256(static_cast<size_t>(chunks > 0 ? chunks : 1) * 8); }

template <bool VEC, bool COEF>
inline void launch_recipe_step(bool with_ema, unsigned blocks, hipStream_t s, float* p, const float* g, float* m, float* v,
                               long long n, const AdamScalars& a, const float* coef, float* ema, float omd) {
    if (with_ema)
        hipLaunchKernelGGL((recipe_step_kernel<VEC, COEF, true>), dim3(blocks), dim3(256), 0, s, p, g, m, v, n, a, coef, ema, omd);
    else
        hipLaunchKernelGGL((recipe_step_kernel<VEC, COEF, false>), dim3(blocks), dim3(256), 0, s, p, g, m, v, n, a, coef, ema, omd);
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaeo_adam_step(float* p, const float* g, float* m, float* v, long long n, float one_minus_b1, float b2,
                               float one_minus_b2, float bc2_sqrt, float eps, float step_size, const float* coef, float* ema,
                               float one_minus_decay, qsae_stream_t stream) {
    QSAE_CHECK_ARG(n >= 0, "n >= 0");
    if (n == 0) return QSAE_OK;                  // nothing to do (an empty tensor's pointers may be null), nothing launched
    QSAE_CHECK_ARG(p && g && m && v, "non-null p, g, m, v");
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 3u) == 0, "coef 4-byte aligned");
    const AdamScalars a{one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size};
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ema);
    const long long work = vec ? (n + 3) / 4 : n;
    long long blocks = (work + 255) / 256;
    if (blocks > QSAE_ADAM_MAX_BLOCKS) blocks = QSAE_ADAM_MAX_BLOCKS;
    hipStream_t s = as_stream(stream);
    const unsigned nb = static_cast<unsigned>(blocks);
    if (vec && coef) launch_recipe_step<true, true>(ema != nullptr, nb, s, p, g, m, v, n, a, coef, ema, one_minus_decay);
    else if (vec) launch_recipe_step<true, false>(ema != nullptr, nb, s, p, g, m, v, n, a, coef, ema, one_minus_decay);
    else if (coef) launch_recipe_step<false, true>(ema != nullptr, nb, s, p, g, m, v, n, a, coef, ema, one_minus_decay);
    else launch_recipe_step<false, false>(ema != nullptr, nb, s, p, g, m, v, n, a, coef, ema, one_minus_decay);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsaeo_adam_step_prefilter(float* W, const float* gW, float* mW, float* vW, float* bias, const float* gb,
                                         float* mb, float* vb, int H, int D, float one_minus_b1, float b2,
                                         float one_minus_b2, float bc2_sqrt, float eps, float step_size, const float* coef,
                                         float* emaW, float* emab, float one_minus_decay, void* Wq, float* meta,
                                         qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && W && gW && mW && vW && Wq && meta, "H > 0, D > 0, non-null W, gW, mW, vW, Wq, meta");
    QSAE_CHECK_ARG((bias && gb && mb && vb) || (!bias && !gb && !mb && !vb), "bias, gb, mb, vb all null or all non-null");
    QSAE_CHECK_ARG(aligned16(W) && aligned16(Wq), "W and Wq 16-byte aligned");
    QSAE_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 3u) == 0, "coef 4-byte aligned");
    QSAE_CHECK_ARG((emab != nullptr) == (emaW != nullptr && bias != nullptr), "emab non-null exactly where emaW and bias are");
    const AdamScalars a{one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size};
    hipStream_t s = as_stream(stream);
    const dim3 grid((H + 3) / 4), block(256);
    unsigned* um = reinterpret_cast<unsigned*>(meta);
    QSAE_HIP(hipMemsetAsync(meta, 0, 4 * sizeof(float), s));
#define QSAEO_PREF_UPDATE(C, E)                                                                                          \
    hipLaunchKernelGGL((recipe_pref_update_kernel<C, E>), grid, block, 0, s, W, gW, mW, vW, bias, gb, mb, vb, H, D, a, coef, \
                       emaW, emab, one_minus_decay, um)
    if (coef && emaW) QSAEO_PREF_UPDATE(true, true);
    else if (coef) QSAEO_PREF_UPDATE(true, false);
    else if (emaW) QSAEO_PREF_UPDATE(false, true);
    else QSAEO_PREF_UPDATE(false, false);
#undef QSAEO_PREF_UPDATE
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(recipe_pref_cast_err_kernel, grid, block, 0, s, static_cast<const float*>(W), H, D,
                       static_cast<const float*>(meta), static_cast<_Float16*>(Wq), um + 3);
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(recipe_pref_finish_kernel, dim3(1), dim3(64), 0, s, meta);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsaeo_project_columns(const float* W, float* G, int D, int H, int64_t ld, qsae_stream_t stream) {
    QSAE_CHECK_ARG(D >= 0 && H >= 0, "D >= 0, H >= 0");
    if (D == 0 || H == 0) return QSAE_OK;
    QSAE_CHECK_SUPPORTED(H % 4 == 0, "H a multiple of 4");
    QSAE_CHECK_ARG(ld >= H && ld % 4 == 0, "ld >= H and a multiple of 4");
    QSAE_CHECK_ARG(W && G, "non-null W, G");
    QSAE_CHECK_ARG(aligned16(W) && aligned16(G), "W and G 16-byte aligned");
    QSAE_CHECK_ARG(W != G, "W and G are different matrices");
    hipLaunchKernelGGL(project_columns_kernel, dim3(static_cast<unsigned>((H + kPjCols - 1) / kPjCols)), dim3(256), 0,
                       as_stream(stream), W, G, D, H, ld);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsaeo_grad_norm_workspace_bytes(const int64_t* counts, int T) {
    if (T <= 0 || T > kGnMaxTensors || !counts) return 0;
    const long long chunks = gn_total_chunks(counts, T);
    if (chunks < 0) return 0;
    return gn_bytes(chunks);
}

extern "C" int qsaeo_grad_norm(const void* const* ptrs, const int64_t* counts, int T, double max_norm, float* coef,
                               void* report, void* workspace, size_t workspace_bytes, qsae_stream_t stream) {
    QSAE_CHECK_ARG(T >= 0, "T >= 0 required");
    QSAE_CHECK_SUPPORTED(T <= kGnMaxTensors, "T <= 65536");
    if (T == 0) return QSAE_OK;
    QSAE_CHECK_ARG(ptrs && counts, "null pointer");
    for (int t = 0; t < T; ++t) {
        QSAE_CHECK_ARG(counts[t] >= 0, "negative element count");
        QSAE_CHECK_ARG(counts[t] == 0 || ptrs[t], "null tensor pointer with a non-zero count");
        QSAE_CHECK_ARG(counts[t] == 0 || (reinterpret_cast<uintptr_t>(ptrs[t]) & 3u) == 0, "tensors must be 4-byte aligned");
    }
    const long long chunks = gn_total_chunks(counts, T);
    QSAE_CHECK_SUPPORTED(chunks >= 0, "at most 2^40 elements per tensor and 2^30 chunks of 8192 elements per call");
    QSAE_CHECK_ARG(max_norm >= 0.0, "max_norm >= 0");
    QSAE_CHECK_ARG(coef && (reinterpret_cast<uintptr_t>(coef) & 3u) == 0, "coef must be non-null and 4-byte aligned");
    QSAE_CHECK_ARG(report && (reinterpret_cast<uintptr_t>(report) & 7u) == 0, "report must be non-null and 8-byte aligned");
    if (!workspace || workspace_bytes < gn_bytes(chunks) || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing, misaligned or smaller than qsaeo_grad_norm_workspace_bytes", __func__);
    hipStream_t s = as_stream(stream);
    double* parts = static_cast<double*>(workspace);
    double* rep = static_cast<double*>(report);
    long long chunk_base = 0;
    for (int first = 0; first < T; first += kGnTable) {
        NormTable tb;
        tb.count = T - first < kGnTable ? T - first : kGnTable;
        tb.first = first;
        tb.chunk_base = static_cast<int>(chunk_base);
        long long at = 0;
        for (int i = 0; i < kGnTable; ++i) {
            const bool in = i < tb.count;
            tb.p[i] = in ? static_cast<const float*>(ptrs[first + i]) : nullptr;
            tb.n[i] = in ? counts[first + i] : 0;
            tb.chunk0[i] = static_cast<int>(at);
            at += gn_chunks(tb.n[i]);
        }
        tb.chunk0[kGnTable] = static_cast<int>(at);
        if (at > 0) {
            hipLaunchKernelGGL(grad_norm_pass_kernel, dim3(static_cast<unsigned>(at)), dim3(kGnThreads), 0, s, tb, parts);
            QSAE_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(grad_norm_join_kernel, dim3(tb.count), dim3(kGnThreads), 0, s, tb,
                           static_cast<const double*>(parts), rep);
        QSAE_LAUNCH_CHECK();
        chunk_base += at;
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(64), 0, s, rep, T, max_norm, coef);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}
