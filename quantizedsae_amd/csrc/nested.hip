// nested.hip -- the nested-dictionary (Matryoshka) objective of the top-k SAEs (include/qsae_nested.h): one reconstruction per
// dictionary prefix from ONE walk over a row's list, and the gradient of a loss that sums over the prefixes.
//
// Forward.  The sparse decoders sum a row's entries as one fmaf chain in ascending unit index (decode_row.h), so the
// reconstruction from the units below a bound is a prefix of that chain.  One wave per activation row sorts the k pairs by unit
// id in LDS (ids outside the dictionary are dropped there), counts the entries below every bound -- wave-uniform numbers -- and
// runs the chain ONCE per column group: when the walk reaches the count of a level, the accumulator is scaled, biased and stored
// as that level's row, and the chain goes on from the same registers.  Every dictionary row is gathered once, whatever the number
// of levels; no accumulator is indexed at run time.  The list reaches the lanes through LDS broadcasts, not through v_readlane,
// so a lane that owns no column may leave the walk (the hazard of decode_row_sorted_wide does not arise).
//
// Backward.  The gradient that reaches the dictionary row of unit h is the sum of the level gradients from level(h) on:
// G[l] = g[l] + G[l + 1].  nested_row_kernel writes these suffix sums for its row and then is train_row_kernel (train.hip) with
// g_recon = G[level(h)] per entry; a lane reads back only the columns it wrote itself.  The unit sums are the kernels of
// train.hip with the same lookup (unit_levels.h).
//
// The bodies of both kernels live in nested_rows.h, shared with nested_ragged.hip (the same walk over the first counts[r]
// entries of a row); here the list length is k for every row.
#include "level_entry.h"
#include "../../include/qsae_nested.h"

namespace qsae {

static_assert(kNestedMaxK == QSAEN_MAX_K, "nested_rows.h and qsae_nested.h name the same limit");
static_assert(kMaxLevels == QSAEN_MAX_LEVELS, "unit_levels.h and qsae_nested.h name the same limit");
static_assert(kLevelMaxD == QSAEN_MAX_D, "level_entry.h and qsae_nested.h name the same limit");

// recon [lv.n][B][D]; the body (nested_rows.h) with every row walking all k entries of its list
template <int MODE>
__global__ void __launch_bounds__(64 * kNestedWaves)
nested_decode_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, int B, int k, int H, NestedDict d,
                     const float* __restrict__ bias, UnitLevels lv, float* __restrict__ recon) {
    const long long row = static_cast<long long>(blockIdx.x) * kNestedWaves + (threadIdx.x >> 6);
    nested_decode_body<MODE>(row < B, row, idx, val, k, k, B, H, d, bias, lv, recon, nullptr);
}

// One wave per row, four rows per workgroup: G, gv and dx of the body (nested_rows.h) over all k entries
__global__ void __launch_bounds__(64 * kNestedWaves)
nested_row_kernel(const int32_t* __restrict__ idx, int B, int k, int H, int D, const float* __restrict__ table, float step,
                  LevelGrads gl, UnitLevels lv, const float* __restrict__ gL, long long gl_ld, const float* __restrict__ Wenc,
                  float* G, float* __restrict__ gv, float* __restrict__ dx) {
    const int r = blockIdx.x * kNestedWaves + (threadIdx.x >> 6);
    nested_row_body(r < B, r, idx, k, k, B, H, D, table, step, gl, lv, gL, gl_ld, Wenc, G, gv, dx);
}

// recon [n_levels][B][D] after the checks of level_entry.h
static int decode_nested(const char* who, const int32_t* idx, const float* val, int B, int k, NestedDict d, int H,
                         const float* bias, const int* bounds, int n_levels, float* recon, qsae_stream_t stream) {
    UnitLevels lv;
    if (const int rc = level_limits(who, kNestedRules, false, B, k, H, d.D, is_packed(d), d.n, bounds, n_levels, &lv); rc != QSAE_OK)
        return rc;
    if (B == 0) return QSAE_OK;
    if (!recon || (k > 0 && (!idx || !val)) || (!d.packed && !d.table))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (misaligned(idx, 4) || misaligned(val, 4) || misaligned(bias, 4) || misaligned(recon, 16) || misaligned(d.packed, 4) ||
        misaligned(d.table, 16))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: a pointer is not aligned as the header asks", who);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(B) + kNestedWaves - 1) / kNestedWaves)), block(64 * kNestedWaves);
    for_dict_mode(d, [&](auto mode) {
        hipLaunchKernelGGL(nested_decode_kernel<decltype(mode)::value>, grid, block, 0, as_stream(stream), idx, val, B, k, H, d,
                           bias, lv, recon);
    });
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaen_decode_nested_binary(const int32_t* idx, const float* val, int B, int k, const uint8_t* packed, int H, int D,
                                          int n_bits, float step, const float* dec_bias, const int* bounds, int n_levels,
                                          float* recon, qsae_stream_t stream) {
    return decode_nested(__func__, idx, val, B, k, packed_dict(packed, D, n_bits, step), H, dec_bias, bounds, n_levels, recon,
                         stream);
}

extern "C" int qsaen_decode_nested_table(const int32_t* idx, const float* val, int B, int k, const float* table, int H, int D,
                                         float scale, const float* dec_bias, const int* bounds, int n_levels, float* recon,
                                         qsae_stream_t stream) {
    return decode_nested(__func__, idx, val, B, k, table_dict(table, D, scale), H, dec_bias, bounds, n_levels, recon, stream);
}

extern "C" int qsaen_row_grad_nested(const int32_t* idx, int B, int k, const float* table, int H, int D, float step,
                                     const float* const* g_levels, const int* bounds, int n_levels, const float* g_latent,
                                     int64_t g_latent_ld, const float* W_enc, float* G, float* gv, float* dx,
                                     qsae_stream_t stream) {
    return row_grad_levels(__func__, kNestedRules, false, false, "g_levels", idx, nullptr, B, k, table, H, D, g_levels, bounds,
                           n_levels, g_latent, g_latent_ld, W_enc, G, gv, dx, [&](const LevelGrads& gl, const UnitLevels& lv) {
        hipLaunchKernelGGL(nested_row_kernel, dim3((B + kNestedWaves - 1) / kNestedWaves), dim3(64 * kNestedWaves), 0,
                           as_stream(stream), idx, B, k, H, D, table, step, gl, lv, g_latent,
                           static_cast<long long>(g_latent_ld), W_enc, G, gv, dx);
    });
}

extern "C" size_t qsaen_train_unit_grad_nested_workspace_bytes(int B, int k, int H, int D) {
    return unit_grad_levels_bytes(kNestedRules, B, k, H, D);
}

extern "C" size_t qsaen_train_table_unit_grad_nested_workspace_bytes(int B, int k, int H, int D) {
    return table_unit_grad_levels_bytes(kNestedRules, B, k, H, D);
}

extern "C" int qsaen_train_unit_grad_nested(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv,
                                            int B, int k, const float* x, const float* G, const int* bounds, int n_levels,
                                            const float* logits, int H, int D, int n_bits, float step, const float* g_polarize,
                                            float* dW_enc, float* db_enc, float* dlogits, void* workspace,
                                            size_t workspace_bytes, qsae_stream_t stream) {
    UnitLevels lv;
    if (const int rc = unit_grad_levels_checks(__func__, kNestedRules, offsets, entries, val, gv, B, k, x, G, bounds, n_levels,
                                               logits, H, D, n_bits, dW_enc, dlogits, workspace, workspace_bytes, &lv);
        rc != QSAE_OK)
        return rc;
    QSAE_HIP(train_unit_grad_levels(offsets, entries, val, gv, B, k, x, G, lv, logits, H, D, n_bits, step, g_polarize, dW_enc,
                                    db_enc, dlogits, workspace, as_stream(stream)));
    return QSAE_OK;
}

extern "C" int qsaen_train_table_unit_grad_nested(const int32_t* offsets, const int32_t* entries, const float* val,
                                                  const float* gv, int B, int k, const float* x, const float* G,
                                                  const int* bounds, int n_levels, int H, int D, float* dW_enc, float* db_enc,
                                                  float* dW_dec, int64_t dW_dec_ld, void* workspace, size_t workspace_bytes,
                                                  qsae_stream_t stream) {
    UnitLevels lv;
    if (const int rc = table_unit_grad_levels_checks(__func__, kNestedRules, offsets, entries, val, gv, B, k, x, G, bounds,
                                                     n_levels, H, D, dW_enc, dW_dec, dW_dec_ld, workspace, workspace_bytes, &lv);
        rc != QSAE_OK)
        return rc;
    QSAE_HIP(train_table_unit_grad_levels(offsets, entries, val, gv, B, k, x, G, lv, H, D, dW_enc, db_enc, dW_dec,
                                          static_cast<long long>(dW_dec_ld), workspace, as_stream(stream)));
    return QSAE_OK;
}
