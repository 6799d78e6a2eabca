// train_row.h -- one activation row of the trainers' row gradient (gv and dx; notation in train.hip): the body that
// train_row_kernel (train.hip, qsae_train_row_grad) and the ragged row kernel of the batch-wide top-k (batch_topk.hip,
// qsaeb_row_grad_ragged) share.  One body, two callers: the same chains, hence the same bits.
#pragma once

#include "common.h"
#include "csr_lists.h"

namespace qsae {

constexpr int kTrainMaxK = 256;
constexpr int kRowWaves = 4;            // activation rows of a workgroup: one wave per row

typedef float tr_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ tr_f32x4 ld4(const float* p) { return *reinterpret_cast<const tr_f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, tr_f32x4 v) { *reinterpret_cast<tr_f32x4*>(p) = v; }
__device__ __forceinline__ tr_f32x4 fma4(float a, tr_f32x4 w, tr_f32x4 acc) {
    tr_f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = fmaf(a, w[e], acc[e]);
    return r;
}

// All threads of the workgroup (64 kRowWaves) call this: it contains workgroup barriers, and a wave whose row is out of range
// passes active = false and only takes part in them.  Row r walks its first k entries (wave-uniform; the waves of a workgroup
// may differ) of idx and gv, whose rows are ld entries apart.  Lane l owns columns 4 (l + 64 i) .. + 3; each dot product is
// the lane's chain over its columns, then a butterfly (every lane of the wave takes part in every shuffle, whatever D is).
__device__ __forceinline__ void train_row_body(bool active, int r, const int32_t* __restrict__ idx, int k, int ld, int H, int D,
                                               const float* __restrict__ table, float step, const float* __restrict__ gR,
                                               const float* __restrict__ gL, long long gl_ld, const float* __restrict__ Wenc,
                                               float* __restrict__ gv, float* __restrict__ dx) {
    __shared__ int s_h[kRowWaves][kTrainMaxK];
    __shared__ float s_g[kRowWaves][kTrainMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D4 = D / 4;
    if (active)
        for (int j = lane; j < k; j += 64) s_h[wave][j] = clamp_unit(idx[static_cast<long long>(r) * ld + j], H);
    __syncthreads();
    if (active) {
        const float* g = gR ? gR + static_cast<long long>(r) * D : nullptr;
        for (int j0 = 0; j0 < k; j0 += 4) {
            float part[4] = {0.f, 0.f, 0.f, 0.f};
            if (g) {
                int hh[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) hh[u] = s_h[wave][min(j0 + u, k - 1)];
                for (int c = lane; c < D4; c += 64) {
                    const tr_f32x4 a = ld4(g + 4 * c);
                    tr_f32x4 t[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) t[u] = ld4(table + static_cast<long long>(hh[u]) * D + 4 * c);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) part[u] = fmaf(a[e], t[u][e], part[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    for (int off = 32; off > 0; off >>= 1) part[u] += __shfl_xor(part[u], off, 64);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                if (j < k) {
                    float val = g ? step * part[u] : 0.0f;
                    if (gL) val = gL[static_cast<long long>(r) * gl_ld + s_h[wave][j]] + val;
                    if (lane == 0) {
                        gv[static_cast<long long>(r) * ld + j] = val;
                        s_g[wave][j] = val;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (active && dx) {
        for (int c = lane; c < D4; c += 64) {
            tr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < k; ++j)
                acc = fma4(s_g[wave][j], ld4(Wenc + static_cast<long long>(s_h[wave][j]) * D + 4 * c), acc);
            st4(dx + static_cast<long long>(r) * D + 4 * c, acc);
        }
    }
}

}  // namespace qsae
