// unit_levels.h -- the unit -> gradient-row lookup of the nested-dictionary objective (include/qsae_nested.h), shared by the
// unit kernels of train.hip, which take it as one more operand, and by nested.hip, which fills it in.
#pragma once

#include "common.h"

namespace qsae {

constexpr int kMaxLevels = 8;

// n == 0: one gradient tensor [B][D] for every unit (the plain objective).  Otherwise level(h) = the number of bounds <= h
// (bounds ascending, the last one == H), and unit h reads the tensor at base + level(h) * stride.
struct UnitLevels {
    long long stride;          // floats between two levels: B * D
    int n;
    int bounds[kMaxLevels];
};

__host__ __device__ inline int unit_level(const UnitLevels& lv, int h) {
    int l = 0;
#pragma unroll
    for (int i = 0; i < kMaxLevels; ++i) l += (i < lv.n - 1 && lv.bounds[i] <= h) ? 1 : 0;      // never past the last level
    return l;
}

// The unit sums of train.hip with g_recon = G[level(h)] (G [lv.n][B][D] or nullptr), launched without further checks: the
// operands are those of qsae_train_unit_grad / qsae_train_table_unit_grad, already validated by the caller, and the workspace
// holds what their sizers ask for.
hipError_t train_unit_grad_levels(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                                  const float* x, const float* G, const UnitLevels& lv, const float* logits, int H, int D,
                                  int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc, float* dlogits,
                                  void* workspace, hipStream_t s);
hipError_t train_table_unit_grad_levels(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                                        int k, const float* x, const float* G, const UnitLevels& lv, int H, int D, float* dW_enc,
                                        float* db_enc, float* dW_dec, long long dW_dec_ld, void* workspace, hipStream_t s);

// The same with an entry-keyed lookup (include/qsae_multik.h): pts.bounds are the rank prefixes ks, and entry e of a list (the
// flat index r k + j) reads g_recon = G[unit_level(pts, e % k)], the point of its rank, instead of the level of its unit.
hipError_t train_unit_grad_ranks(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                                 const float* x, const float* G, const UnitLevels& pts, const float* logits, int H, int D,
                                 int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc, float* dlogits,
                                 void* workspace, hipStream_t s);
hipError_t train_table_unit_grad_ranks(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                                       int k, const float* x, const float* G, const UnitLevels& pts, int H, int D, float* dW_enc,
                                       float* db_enc, float* dW_dec, long long dW_dec_ld, void* workspace, hipStream_t s);

}  // namespace qsae
