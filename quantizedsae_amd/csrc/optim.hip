// optim.hip -- the Adam step in one pass: qsae_adam_step over a flat fp32 tensor, and qsae_adam_step_prefilter, which
// steps the top-k encoder's weight and bias and leaves the fp16 candidate-pass copy (Wq, meta) of the new values -- what
// qsae_prefilter_pack_w would build from them in three more passes over the weight.
#include "prefilter_common.h"

// workgroups of one qsae_adam_step launch at the most (the rest of a large tensor is taken in grid-stride trips)
#ifndef QSAE_ADAM_MAX_BLOCKS
#define QSAE_ADAM_MAX_BLOCKS 4096
#endif

namespace qsae {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The six scalars of a step, each rounded to fp32 once by the caller (doubles on the host: step_size = lr / (1 - b1^t),
// bc2_sqrt = sqrt(1 - b2^t)).
struct AdamScalars {
    float one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size;
};

// One element.  Every line is one IEEE fp32 operation (the build passes -ffp-contract=off; divide and sqrt are the
// correctly rounded ones, subnormals are kept): the op sequence of torch's single-tensor Adam without amsgrad, maximize
// or weight decay -- lerp of the first moment, mul + addcmul of the second, sqrt / bias correction + eps, addcdiv.
// NaN and inf go where the operations take them.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& a) {
    const float d = g - m;
    const float dm = d * a.one_minus_b1;
    m = m + dm;
    const float av = v * a.b2;
    const float q = g * g;
    const float qv = q * a.one_minus_b2;
    v = av + qv;
    const float s = sqrtf(v);
    const float r = s / a.bc2_sqrt;
    const float den = r + a.eps;
    const float u = m / den;
    const float su = a.step_size * u;
    p = p - su;
}

// VEC: all four pointers 16-byte aligned, four elements per load; otherwise one.  The elements past the last whole
// vector are taken one by one by the first workgroup.  Same arithmetic per element, hence the same bits.
template <bool VEC>
__global__ void __launch_bounds__(256)
adam_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                 long long n, AdamScalars a) {
    const long long tid = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long stride = static_cast<long long>(gridDim.x) * 256;
    if (VEC) {
        const long long n4 = n >> 2;
        for (long long i = tid; i < n4; i += stride) {
            f32x4 pp = reinterpret_cast<f32x4*>(p)[i], mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
            const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = pp[j], mj = mm[j], vj = vv[j];
                adam_elem(pj, gg[j], mj, vj, a);
                pp[j] = pj; mm[j] = mj; vv[j] = vj;
            }
            reinterpret_cast<f32x4*>(p)[i] = pp;
            reinterpret_cast<f32x4*>(m)[i] = mm;
            reinterpret_cast<f32x4*>(v)[i] = vv;
        }
        const long long i = (n4 << 2) + tid;          // tail: at most 3 elements
        if (tid < 4 && i < n) adam_elem(p[i], g[i], m[i], v[i], a);
    } else {
        for (long long i = tid; i < n; i += stride) adam_elem(p[i], g[i], m[i], v[i], a);
    }
}

// ---- the encoder pair of a top-k model ------------------------------------------------------------------------------
// The maxima over the workgroup's four waves of three non-negative (or NaN) floats, ordered by their bit patterns like
// pack_w's atomics order them, then one atomicMax per quantity and workgroup (none where the target is null).  Maxima do
// not depend on the order.  Every thread of the workgroup comes here (idle waves bring zeros).
__device__ __forceinline__ void block_max3(unsigned a, unsigned b, unsigned c, unsigned* wa, unsigned* wb, unsigned* wc) {
    __shared__ unsigned part[3][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { part[0][wave] = a; part[1][wave] = b; part[2][wave] = c; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned* target = threadIdx.x == 0 ? wa : threadIdx.x == 1 ? wb : wc;
        const unsigned* q = part[threadIdx.x];
        unsigned r = q[0];
        for (int w = 1; w < 4; ++w) r = q[w] > r ? q[w] : r;
        if (target) atomicMax(target, r);
    }
}

// (A) one wave per hidden unit: Adam on the row (lane l takes d = l, l + 64, ...: the lane assignment of pack_w's
// statistics, which the new values enter from the registers they were just stored from) and on its bias element.
// meta[0] carries max |W'| until adam_pref_finish_kernel turns it into the scale; meta[3] is left to (B).
__global__ void __launch_bounds__(256)
adam_pref_update_kernel(float* __restrict__ W, const float* __restrict__ gW, float* __restrict__ mW, float* __restrict__ vW,
                        float* __restrict__ bias, const float* __restrict__ gb, float* __restrict__ mb,
                        float* __restrict__ vb, int H, int D, AdamScalars a, unsigned* __restrict__ meta) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    float mx = 0.f, ss = 0.f, babs = 0.f;
    if (row < H) {
        const int64_t base = static_cast<int64_t>(row) * D;
#pragma unroll 4
        for (int d = lane; d < D; d += 64) {
            float w = W[base + d], m = mW[base + d], v = vW[base + d];
            adam_elem(w, gW[base + d], m, v, a);
            W[base + d] = w; mW[base + d] = m; vW[base + d] = v;
            pref_w_stat_step(w, mx, ss);
        }
        pref_w_stat_join(mx, ss);
        if (bias && lane == 0) {
            float b = bias[row], m = mb[row], v = vb[row];
            adam_elem(b, gb[row], m, v, a);
            bias[row] = b; mb[row] = m; vb[row] = v;
            babs = fabsf(b);
        }
    }
    block_max3(__float_as_uint(mx), __float_as_uint(babs), __float_as_uint(row < H ? pref_w_row_norm(ss) : 0.f),
               &meta[0], bias ? &meta[2] : nullptr, &meta[1]);
}

// (B) one wave per hidden unit: the row's fp16 copy under sw = pow2_scale_for(max |W'|) and its distance from the row
__global__ void __launch_bounds__(256)
adam_pref_cast_err_kernel(const float* __restrict__ W, int H, int D, const float* __restrict__ meta_in,
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
__global__ void adam_pref_finish_kernel(float* __restrict__ meta) {
    if (threadIdx.x == 0 && blockIdx.x == 0) meta[0] = pow2_scale_for(meta[0]);
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsae_adam_step(float* p, const float* g, float* m, float* v, long long n, float one_minus_b1, float b2,
                              float one_minus_b2, float bc2_sqrt, float eps, float step_size, qsae_stream_t stream) {
    QSAE_CHECK_ARG(n >= 0, "n >= 0");
    if (n == 0) return QSAE_OK;                  // nothing to do (an empty tensor's pointers may be null), nothing launched
    QSAE_CHECK_ARG(p && g && m && v, "non-null p, g, m, v");
    const AdamScalars a{one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size};
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
    const long long work = vec ? (n + 3) / 4 : n;
    long long blocks = (work + 255) / 256;
    if (blocks > QSAE_ADAM_MAX_BLOCKS) blocks = QSAE_ADAM_MAX_BLOCKS;
    hipStream_t s = as_stream(stream);
    if (vec)
        hipLaunchKernelGGL(adam_step_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, p, g, m, v, n, a);
    else
        hipLaunchKernelGGL(adam_step_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, p, g, m, v, n, a);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" int qsae_adam_step_prefilter(float* W, const float* gW, float* mW, float* vW, float* bias, const float* gb,
                                        float* mb, float* vb, int H, int D, float one_minus_b1, float b2,
                                        float one_minus_b2, float bc2_sqrt, float eps, float step_size, void* Wq,
                                        float* meta, qsae_stream_t stream) {
    QSAE_CHECK_ARG(H > 0 && D > 0 && W && gW && mW && vW && Wq && meta, "H > 0, D > 0, non-null W, gW, mW, vW, Wq, meta");
    QSAE_CHECK_ARG((bias && gb && mb && vb) || (!bias && !gb && !mb && !vb), "bias, gb, mb, vb all null or all non-null");
    QSAE_CHECK_ARG(aligned16(W) && aligned16(Wq), "W and Wq 16-byte aligned");
    const AdamScalars a{one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size};
    hipStream_t s = as_stream(stream);
    const dim3 grid((H + 3) / 4), block(256);
    QSAE_HIP(hipMemsetAsync(meta, 0, 4 * sizeof(float), s));
    hipLaunchKernelGGL(adam_pref_update_kernel, grid, block, 0, s, W, gW, mW, vW, bias, gb, mb, vb, H, D, a,
                       reinterpret_cast<unsigned*>(meta));
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(adam_pref_cast_err_kernel, grid, block, 0, s, static_cast<const float*>(W), H, D,
                       static_cast<const float*>(meta), static_cast<_Float16*>(Wq), reinterpret_cast<unsigned*>(meta + 3));
    QSAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(adam_pref_finish_kernel, dim3(1), dim3(64), 0, s, meta);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}
