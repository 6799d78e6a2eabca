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
#include "nested_rows.h"
#include "../../include/qsae_nested.h"

namespace qsae {

static_assert(kNestedMaxK == QSAEN_MAX_K, "nested_rows.h and qsae_nested.h name the same limit");
static_assert(kMaxLevels == QSAEN_MAX_LEVELS, "unit_levels.h and qsae_nested.h name the same limit");

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

// ---- the checks every entry point shares, in the order the header states ---------------------------------------------------
inline bool nested_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// limits (from the sizes alone), then the host array bounds -> lv
static int nested_limits(const char* who, int B, int k, int H, int D, bool packed, int n_bits, const int* bounds, int n_levels,
                         UnitLevels* lv) {
    if (B < 0 || H < 1) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0 and H >= 1 required", who);
    if (n_levels < 1 || n_levels > kMaxLevels) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_levels <= 8", who);
    if (k < 0 || k > kNestedMaxK) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 0 <= k <= 256", who);
    if (D < 4 || D % 4 != 0 || D > QSAEN_MAX_D) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: D a positive multiple of 4 up to 4096", who);
    if (packed && (n_bits < 1 || n_bits > 8)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_bits <= 8", who);
    if (static_cast<long long>(B) * k >= (1LL << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * k < 2^31", who);
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

static int decode_nested(const char* who, const int32_t* idx, const float* val, int B, int k, NestedDict d, int H,
                         const float* bias, const int* bounds, int n_levels, float* recon, qsae_stream_t stream) {
    const bool packed = d.table == nullptr && d.n != 0;
    UnitLevels lv;
    if (const int rc = nested_limits(who, B, k, H, d.D, packed, d.n, bounds, n_levels, &lv); rc != QSAE_OK) return rc;
    if (B == 0) return QSAE_OK;
    if (!recon || (k > 0 && (!idx || !val)) || (!d.packed && !d.table))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (nested_misaligned(idx, 4) || nested_misaligned(val, 4) || nested_misaligned(bias, 4) || nested_misaligned(recon, 16) ||
        nested_misaligned(d.packed, 4) || nested_misaligned(d.table, 16))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: a pointer is not aligned as the header asks", who);
    hipStream_t s = as_stream(stream);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(B) + kNestedWaves - 1) / kNestedWaves)), block(64 * kNestedWaves);
    switch (packed ? field_width(d.n) : 0) {
        case 0: hipLaunchKernelGGL(nested_decode_kernel<0>, grid, block, 0, s, idx, val, B, k, H, d, bias, lv, recon); break;
        case 1: hipLaunchKernelGGL(nested_decode_kernel<1>, grid, block, 0, s, idx, val, B, k, H, d, bias, lv, recon); break;
        case 2: hipLaunchKernelGGL(nested_decode_kernel<2>, grid, block, 0, s, idx, val, B, k, H, d, bias, lv, recon); break;
        case 4: hipLaunchKernelGGL(nested_decode_kernel<4>, grid, block, 0, s, idx, val, B, k, H, d, bias, lv, recon); break;
        default: hipLaunchKernelGGL(nested_decode_kernel<8>, grid, block, 0, s, idx, val, B, k, H, d, bias, lv, recon); break;
    }
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaen_decode_nested_binary(const int32_t* idx, const float* val, int B, int k, const uint8_t* packed, int H, int D,
                                          int n_bits, float step, const float* dec_bias, const int* bounds, int n_levels,
                                          float* recon, qsae_stream_t stream) {
    const bool bits_ok = n_bits >= 1 && n_bits <= 8;
    // n == 0 marks the table form, so a refused n_bits travels as -1
    const NestedDict d{reinterpret_cast<const uint32_t*>(packed), nullptr,
                       (bits_ok && D > 0 && D <= QSAEN_MAX_D) ? (D * field_width(n_bits) + 31) / 32 : 0,    // qsae_binary_row_bytes / 4
                       bits_ok ? n_bits : -1, D, step};
    return decode_nested(__func__, idx, val, B, k, d, H, dec_bias, bounds, n_levels, recon, stream);
}

extern "C" int qsaen_decode_nested_table(const int32_t* idx, const float* val, int B, int k, const float* table, int H, int D,
                                         float scale, const float* dec_bias, const int* bounds, int n_levels, float* recon,
                                         qsae_stream_t stream) {
    const NestedDict d{nullptr, table, 0, 0, D, scale};
    return decode_nested(__func__, idx, val, B, k, d, H, dec_bias, bounds, n_levels, recon, stream);
}

extern "C" int qsaen_row_grad_nested(const int32_t* idx, int B, int k, const float* table, int H, int D, float step,
                                     const float* const* g_levels, const int* bounds, int n_levels, const float* g_latent,
                                     int64_t g_latent_ld, const float* W_enc, float* G, float* gv, float* dx,
                                     qsae_stream_t stream) {
    UnitLevels lv;
    if (const int rc = nested_limits(__func__, B, k, H, D, false, 0, bounds, n_levels, &lv); rc != QSAE_OK) return rc;
    QSAE_CHECK_ARG(g_levels != nullptr, "g_levels is null");
    LevelGrads gl;
    for (int l = 0; l < kMaxLevels; ++l) gl.p[l] = l < n_levels ? g_levels[l] : nullptr;
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(table && G && (k == 0 || (idx && gv)), "null pointer");
    QSAE_CHECK_ARG(!dx || W_enc, "dx needs W_enc");
    bool g_ok = true;
    for (int l = 0; l < kMaxLevels; ++l) g_ok = g_ok && aligned16(gl.p[l]);
    QSAE_CHECK_ARG(g_ok && aligned16(table) && aligned16(G) && (!dx || (aligned16(dx) && aligned16(W_enc))),
                   "table, g_levels, G, W_enc and dx must be 16-byte aligned");
    QSAE_CHECK_ARG(!nested_misaligned(idx, 4) && !nested_misaligned(gv, 4) && !nested_misaligned(g_latent, 4),
                   "idx, gv and g_latent must be 4-byte aligned");
    QSAE_CHECK_ARG(!g_latent || g_latent_ld >= 0, "g_latent_ld >= 0 required");
    hipLaunchKernelGGL(nested_row_kernel, dim3((B + kNestedWaves - 1) / kNestedWaves), dim3(64 * kNestedWaves), 0,
                       as_stream(stream), idx, B, k, H, D, table, step, gl, lv, g_latent, static_cast<long long>(g_latent_ld),
                       W_enc, G, gv, dx);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsaen_train_unit_grad_nested_workspace_bytes(int B, int k, int H, int D) {
    if (k > kNestedMaxK || static_cast<long long>(B) * k >= (1LL << 31)) return 0;
    return qsae_train_unit_grad_workspace_bytes(B, k, H, D);
}

extern "C" size_t qsaen_train_table_unit_grad_nested_workspace_bytes(int B, int k, int H, int D) {
    return qsae_train_table_unit_grad_workspace_bytes(B, k, H, D);
}

extern "C" int qsaen_train_unit_grad_nested(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv,
                                            int B, int k, const float* x, const float* G, const int* bounds, int n_levels,
                                            const float* logits, int H, int D, int n_bits, float step, const float* g_polarize,
                                            float* dW_enc, float* db_enc, float* dlogits, void* workspace,
                                            size_t workspace_bytes, qsae_stream_t stream) {
    UnitLevels lv;
    if (const int rc = nested_limits(__func__, B, k, H, D, true, n_bits, bounds, n_levels, &lv); rc != QSAE_OK) return rc;
    const long long Bk = static_cast<long long>(B) * k;
    QSAE_CHECK_ARG(offsets != nullptr, "null pointer");
    QSAE_CHECK_ARG(Bk == 0 || (entries && val && gv && x), "null pointer");
    QSAE_CHECK_ARG(!dlogits || logits, "dlogits needs logits");
    QSAE_CHECK_ARG((!x || aligned16(x)) && aligned16(G) && (!dW_enc || aligned16(dW_enc)) &&
                   (!dlogits || (aligned16(dlogits) && aligned16(logits))),
                   "x, G, logits, dW_enc and dlogits must be 16-byte aligned");
    if (!workspace || workspace_bytes < qsaen_train_unit_grad_nested_workspace_bytes(B, k, H, D))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing or smaller than the sizer's bytes", __func__);
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
    if (const int rc = nested_limits(__func__, B, k, H, D, false, 0, bounds, n_levels, &lv); rc != QSAE_OK) return rc;
    const long long Bk = static_cast<long long>(B) * k;
    QSAE_CHECK_ARG(offsets != nullptr, "null pointer");
    QSAE_CHECK_ARG(Bk == 0 || (entries && val && gv && x), "null pointer");
    QSAE_CHECK_ARG(!dW_dec || dW_dec_ld >= H, "dW_dec_ld >= H required");
    QSAE_CHECK_ARG((!x || aligned16(x)) && aligned16(G) && (!dW_enc || aligned16(dW_enc)),
                   "x, G and dW_enc must be 16-byte aligned");
    if (!workspace || workspace_bytes < qsaen_train_table_unit_grad_nested_workspace_bytes(B, k, H, D))
        return fail(QSAE_ERR_WORKSPACE, "%s: workspace missing or smaller than the sizer's bytes", __func__);
    QSAE_HIP(train_table_unit_grad_levels(offsets, entries, val, gv, B, k, x, G, lv, H, D, dW_enc, db_enc, dW_dec,
                                          static_cast<long long>(dW_dec_ld), workspace, as_stream(stream)));
    return QSAE_OK;
}
