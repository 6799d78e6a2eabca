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
#include "nested_rows.h"
#include "../../include/qsae_nested_batch.h"

namespace qsae {

static_assert(kNestedMaxK == QSAEM_MAX_K, "nested_rows.h and qsae_nested_batch.h name the same limit");
static_assert(kMaxLevels == QSAEM_MAX_LEVELS, "unit_levels.h and qsae_nested_batch.h name the same limit");

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

// ---- the checks every entry point shares, in the order the header states ---------------------------------------------------
inline bool nr_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// limits (from the sizes alone), then the host array bounds -> lv
static int nested_ragged_limits(const char* who, int B, int K, int H, int D, bool packed, int n_bits, const int* bounds,
                                int n_levels, UnitLevels* lv) {
    if (B < 0 || K < 1 || H < 1) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0, K >= 1 and H >= 1 required", who);
    if (K > QSAEM_MAX_K) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: K <= 256", who);
    if (n_levels < 1 || n_levels > kMaxLevels) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_levels <= 8", who);
    if (D < 4 || D % 4 != 0 || D > QSAEM_MAX_D) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: D a positive multiple of 4 up to 4096", who);
    if (packed && (n_bits < 1 || n_bits > 8)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_bits <= 8", who);
    if (static_cast<long long>(B) * K >= (1LL << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * K < 2^31", who);
    if (!bounds) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: bounds is null", who);
    lv->stride = static_cast<long long>(B) * D;
    lv->n = n_levels;
    for (int i = 0; i < kMaxLevels; ++i) lv->bounds[i] = i < n_levels ? bounds[i] : 0;
    for (int i = 0; i < n_levels; ++i)
        if (bounds[i] <= (i > 0 ? bounds[i - 1] : 0))
            return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 0 < bounds[0] < ... < bounds[n_levels - 1] == H required", who);
    if (bounds[n_levels - 1] != H)
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 0 < bounds[0] < ... < bounds[n_levels - 1] == H required", who);
    return QSAE_OK;
}

static int decode_nested_ragged(const char* who, const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                NestedDict d, int H, const float* bias, const int* bounds, int n_levels, float* recon,
                                int32_t* counts_below, qsae_stream_t stream) {
    const bool packed = d.table == nullptr && d.n != 0;
    UnitLevels lv;
    if (const int rc = nested_ragged_limits(who, B, K, H, d.D, packed, d.n, bounds, n_levels, &lv); rc != QSAE_OK) return rc;
    if (B == 0) return QSAE_OK;
    if (!idx || !val || !counts || !recon || (!d.packed && !d.table))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (nr_misaligned(idx, 4) || nr_misaligned(val, 4) || nr_misaligned(counts, 4) || nr_misaligned(bias, 4) ||
        nr_misaligned(recon, 16) || nr_misaligned(counts_below, 4) || nr_misaligned(d.packed, 4) || nr_misaligned(d.table, 16))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: a pointer is not aligned as the header asks", who);
    hipStream_t s = as_stream(stream);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(B) + kNestedWaves - 1) / kNestedWaves)), block(64 * kNestedWaves);
#define QSAEM_LAUNCH(MODE) hipLaunchKernelGGL(nested_ragged_decode_kernel<MODE>, grid, block, 0, s, idx, val, counts, B, K, H, d, \
                                              bias, lv, recon, counts_below)
    switch (packed ? field_width(d.n) : 0) {
        case 0: QSAEM_LAUNCH(0); break;
        case 1: QSAEM_LAUNCH(1); break;
        case 2: QSAEM_LAUNCH(2); break;
        case 4: QSAEM_LAUNCH(4); break;
        default: QSAEM_LAUNCH(8); break;
    }
#undef QSAEM_LAUNCH
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaem_decode_nested_ragged_binary(const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                                 const uint8_t* packed, int H, int D, int n_bits, float step,
                                                 const float* dec_bias, const int* bounds, int n_levels, float* recon,
                                                 int32_t* counts_below, qsae_stream_t stream) {
    const bool bits_ok = n_bits >= 1 && n_bits <= 8;
    // n == 0 marks the table form, so a refused n_bits travels as -1
    const NestedDict d{reinterpret_cast<const uint32_t*>(packed), nullptr,
                       (bits_ok && D > 0 && D <= QSAEM_MAX_D) ? (D * field_width(n_bits) + 31) / 32 : 0,    // qsae_binary_row_bytes / 4
                       bits_ok ? n_bits : -1, D, step};
    return decode_nested_ragged(__func__, idx, val, counts, B, K, d, H, dec_bias, bounds, n_levels, recon, counts_below, stream);
}

extern "C" int qsaem_decode_nested_ragged_table(const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                                const float* table, int H, int D, float scale, const float* dec_bias,
                                                const int* bounds, int n_levels, float* recon, int32_t* counts_below,
                                                qsae_stream_t stream) {
    const NestedDict d{nullptr, table, 0, 0, D, scale};
    return decode_nested_ragged(__func__, idx, val, counts, B, K, d, H, dec_bias, bounds, n_levels, recon, counts_below, stream);
}

extern "C" int qsaem_row_grad_nested_ragged(const int32_t* idx, const int32_t* counts, int B, int K, const float* table, int H,
                                            int D, float step, const float* const* g_levels, const int* bounds, int n_levels,
                                            const float* g_latent, int64_t g_latent_ld, const float* W_enc, float* G, float* gv,
                                            float* dx, qsae_stream_t stream) {
    UnitLevels lv;
    if (const int rc = nested_ragged_limits(__func__, B, K, H, D, false, 0, bounds, n_levels, &lv); rc != QSAE_OK) return rc;
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(g_levels != nullptr, "g_levels is null");
    LevelGrads gl;
    for (int l = 0; l < kMaxLevels; ++l) gl.p[l] = l < n_levels ? g_levels[l] : nullptr;
    QSAE_CHECK_ARG(idx && counts && table && G && gv, "null pointer");
    QSAE_CHECK_ARG(!dx || W_enc, "dx needs W_enc");
    bool g_ok = true;
    for (int l = 0; l < kMaxLevels; ++l) g_ok = g_ok && aligned16(gl.p[l]);
    QSAE_CHECK_ARG(g_ok && aligned16(table) && aligned16(G) && (!dx || (aligned16(dx) && aligned16(W_enc))),
                   "table, g_levels, G, W_enc and dx must be 16-byte aligned");
    QSAE_CHECK_ARG(!nr_misaligned(idx, 4) && !nr_misaligned(counts, 4) && !nr_misaligned(gv, 4) && !nr_misaligned(g_latent, 4),
                   "idx, counts, gv and g_latent must be 4-byte aligned");
    QSAE_CHECK_ARG(!g_latent || g_latent_ld >= 0, "g_latent_ld >= 0 required");
    hipLaunchKernelGGL(nested_ragged_row_kernel, dim3((B + kNestedWaves - 1) / kNestedWaves), dim3(64 * kNestedWaves), 0,
                       as_stream(stream), idx, counts, B, K, H, D, table, step, gl, lv, g_latent,
                       static_cast<long long>(g_latent_ld), W_enc, G, gv, dx);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}
