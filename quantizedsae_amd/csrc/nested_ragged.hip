// nested_ragged.hip -- the nested-dictionary objective over the ragged rows of BatchTopK (include/qsae_nested_batch.h): row r
// decodes, and is differentiated over, the first counts[r] entries of its top-K list.
//
// The kernels are the bodies of nested.hip (nested_rows.h: one wave per activation row, four rows per workgroup) with the list
// length per wave, c(r) = min(max(counts[r], 0), K), instead of one k per launch -- hence the bits qsaen_decode_nested_* and
// qsaen_row_grad_nested give for the truncated lists.  The rank pass loops over i < c(r), the chain walks the counts of the
// kept entries below every bound, and an entry behind the prefix is never loaded, so neither is its dictionary row.  The waves
// of a workgroup now differ in their lengths; the bodies keep every barrier outside the work that depends on the length, so
// a wave with row >= B or c(r) == 0 still reaches each of them.  The decode also stores the per-level counts it walks by
// (one lane, no atomics); the row kernel writes gv behind the prefix as +0.
#include "level_entry.h"
#include "../../include/qsae_nested_batch.h"

namespace qsae {

static_assert(kNestedMaxK == QSAEM_MAX_K, "nested_rows.h and qsae_nested_batch.h name the same limit");
static_assert(kMaxLevels == QSAEM_MAX_LEVELS, "unit_levels.h and qsae_nested_batch.h name the same limit");
static_assert(kLevelMaxD == QSAEM_MAX_D, "level_entry.h and qsae_nested_batch.h name the same limit");

__device__ __forceinline__ int ragged_count(const int32_t* __restrict__ counts, bool active, long long row, int K) {
    if (!active) return 0;
    const int c = counts[row];
    return c < 0 ? 0 : (c > K ? K : c);
}

// recon [lv.n][B][D], counts_below [lv.n][B] or nullptr
template <int MODE>
__global__ void __launch_bounds__(64 * kNestedWaves)
nested_ragged_decode_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val, const int32_t* __restrict__ counts,
                            int B, int K, int H, NestedDict d, const float* __restrict__ bias, UnitLevels lv,
                            float* __restrict__ recon, int32_t* __restrict__ counts_below) {
    const long long row = static_cast<long long>(blockIdx.x) * kNestedWaves + (threadIdx.x >> 6);
    const bool active = row < B;
    const int c = ragged_count(counts, active, row, K);    // wave-uniform; the waves of a workgroup differ
    nested_decode_body<MODE>(active, row, idx, val, c, K, B, H, d, bias, lv, recon, counts_below);
}

__global__ void __launch_bounds__(64 * kNestedWaves)
nested_ragged_row_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ counts, int B, int K, int H, int D,
                         const float* __restrict__ table, float step, LevelGrads gl, UnitLevels lv, const float* __restrict__ gL,
                         long long gl_ld, const float* __restrict__ Wenc, float* G, float* __restrict__ gv,
                         float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kNestedWaves + (threadIdx.x >> 6);
    const bool active = r < B;
    const int c = ragged_count(counts, active, r, K);
    if (active)                                            // behind the prefix: +0 (the body writes only j < c)
        for (int j = c + lane; j < K; j += 64) gv[static_cast<long long>(r) * K + j] = 0.0f;
    nested_row_body(active, r, idx, c, K, B, H, D, table, step, gl, lv, gL, gl_ld, Wenc, G, gv, dx);
}

// recon [n_levels][B][D], counts_below [n_levels][B] or nullptr, after the checks of level_entry.h
static int decode_nested_ragged(const char* who, const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                NestedDict d, int H, const float* bias, const int* bounds, int n_levels, float* recon,
                                int32_t* counts_below, qsae_stream_t stream) {
    UnitLevels lv;
    if (const int rc = level_limits(who, kNestedRaggedRules, false, B, K, H, d.D, is_packed(d), d.n, bounds, n_levels, &lv);
        rc != QSAE_OK)
        return rc;
    if (B == 0) return QSAE_OK;
    if (!idx || !val || !counts || !recon || (!d.packed && !d.table))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (misaligned(idx, 4) || misaligned(val, 4) || misaligned(counts, 4) || misaligned(bias, 4) || misaligned(recon, 16) ||
        misaligned(counts_below, 4) || misaligned(d.packed, 4) || misaligned(d.table, 16))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: a pointer is not aligned as the header asks", who);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(B) + kNestedWaves - 1) / kNestedWaves)), block(64 * kNestedWaves);
    for_dict_mode(d, [&](auto mode) {
        hipLaunchKernelGGL(nested_ragged_decode_kernel<decltype(mode)::value>, grid, block, 0, as_stream(stream), idx, val, counts,
                           B, K, H, d, bias, lv, recon, counts_below);
    });
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaem_decode_nested_ragged_binary(const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                                 const uint8_t* packed, int H, int D, int n_bits, float step,
                                                 const float* dec_bias, const int* bounds, int n_levels, float* recon,
                                                 int32_t* counts_below, qsae_stream_t stream) {
    return decode_nested_ragged(__func__, idx, val, counts, B, K, packed_dict(packed, D, n_bits, step), H, dec_bias, bounds,
                                n_levels, recon, counts_below, stream);
}

extern "C" int qsaem_decode_nested_ragged_table(const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                                const float* table, int H, int D, float scale, const float* dec_bias,
                                                const int* bounds, int n_levels, float* recon, int32_t* counts_below,
                                                qsae_stream_t stream) {
    return decode_nested_ragged(__func__, idx, val, counts, B, K, table_dict(table, D, scale), H, dec_bias, bounds, n_levels,
                                recon, counts_below, stream);
}

extern "C" int qsaem_row_grad_nested_ragged(const int32_t* idx, const int32_t* counts, int B, int K, const float* table, int H,
                                            int D, float step, const float* const* g_levels, const int* bounds, int n_levels,
                                            const float* g_latent, int64_t g_latent_ld, const float* W_enc, float* G, float* gv,
                                            float* dx, qsae_stream_t stream) {
    return row_grad_levels(__func__, kNestedRaggedRules, true, true, "g_levels", idx, counts, B, K, table, H, D, g_levels, bounds,
                           n_levels, g_latent, g_latent_ld, W_enc, G, gv, dx, [&](const LevelGrads& gl, const UnitLevels& lv) {
        hipLaunchKernelGGL(nested_ragged_row_kernel, dim3((B + kNestedWaves - 1) / kNestedWaves), dim3(64 * kNestedWaves), 0,
                           as_stream(stream), idx, counts, B, K, H, D, table, step, gl, lv, g_latent,
                           static_cast<long long>(g_latent_ld), W_enc, G, gv, dx);
    });
}
