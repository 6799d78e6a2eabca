// level_entry.h -- the host side of the level/point entry points (nested.hip, nested_ragged.hip, multi_topk.hip): the checks
// that stand before a launch, in the order the three headers state, and the launches that differ only in a kernel.  Nothing
// here is device code; the extern "C" functions stay in their files and hand over __func__ as `who`, so every refusal keeps
// its status and its text.
#pragma once

#include "nested_rows.h"

namespace qsae {

constexpr int kLevelMaxD = 4096;          // widest activation row (QSAEN_MAX_D, QSAEM_MAX_D, QSAEK_MAX_D)

inline bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

template <class... A>
inline int refuse(int code, const char* fmt, const char* who, A... a) {
    snprintf(last_error_buf(), 512, fmt, who, a...);
    return code;
}

#define QSAE_LEVEL_ARG(cond, ...)                                                          \
    do {                                                                                   \
        if (!(cond)) return refuse(QSAE_ERR_INVALID_ARG, "%s: invalid argument: " __VA_ARGS__); \
    } while (0)

// The dictionary operand of the decoders.  n == 0 marks the table form, so a refused n_bits travels as -1.
inline NestedDict packed_dict(const uint8_t* packed, int D, int n_bits, float step) {
    const bool bits_ok = n_bits >= 1 && n_bits <= 8;
    return NestedDict{reinterpret_cast<const uint32_t*>(packed), nullptr,
                      (bits_ok && D > 0 && D <= kLevelMaxD) ? (D * field_width(n_bits) + 31) / 32 : 0,   // qsae_binary_row_bytes / 4
                      bits_ok ? n_bits : -1, D, step};
}
inline NestedDict table_dict(const float* table, int D, float scale) { return NestedDict{nullptr, table, 0, 0, D, scale}; }
inline bool is_packed(const NestedDict& d) { return d.table == nullptr && d.n != 0; }

// ---- limits (from the sizes alone), then the host array -> lv ---------------------------------------------------------------
enum class SizeCheck {
    kFirst,          // B >= 0 and H >= 1 before the limits (qsae_nested.h)
    kAfterLimits,    // after them (qsae_multik.h)
    kFirstWithK      // B, K and H together, then K <= 256 (qsae_nested_batch.h)
};

struct LevelRules {
    SizeCheck sizes;
    int k_min;               // smallest list length
    bool ends_at_k;          // the array ends at the list length (rank prefixes), not at H (unit bounds)
    bool rows_check_Bk;      // B * k < 2^31 is asked of the row-wise calls too, not of the unit sums alone
    const char* k;           // what the messages call the list length,
    const char* k_range;     // its limits,
    const char* array;       // the host array
    const char* count;       // and its length
};
constexpr LevelRules kNestedRules{SizeCheck::kFirst, 0, false, true, "k", "0 <= k <= 256", "bounds", "n_levels"};
constexpr LevelRules kNestedRaggedRules{SizeCheck::kFirstWithK, 1, false, true, "K", "K <= 256", "bounds", "n_levels"};
constexpr LevelRules kMultikRules{SizeCheck::kAfterLimits, 1, true, false, "K", "1 <= K <= 256", "ks", "n_ks"};

// unit_call: the call runs the unit sums of train.hip, which index the B * k list entries with an int
inline int level_limits(const char* who, const LevelRules& r, bool unit_call, int B, int k, int H, int D, bool packed,
                        int n_bits, const int* a, int n, UnitLevels* lv) {
    const bool k_ok = k >= r.k_min && k <= kNestedMaxK;
    if (r.sizes == SizeCheck::kFirst) QSAE_LEVEL_ARG(B >= 0 && H >= 1, "B >= 0 and H >= 1 required", who);
    if (r.sizes == SizeCheck::kFirstWithK) {
        QSAE_LEVEL_ARG(B >= 0 && k >= 1 && H >= 1, "B >= 0, K >= 1 and H >= 1 required", who);
        if (!k_ok) return refuse(QSAE_ERR_UNSUPPORTED, "%s: unsupported: %s", who, r.k_range);
    }
    if (n < 1 || n > kMaxLevels) return refuse(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= %s <= 8", who, r.count);
    if (!k_ok) return refuse(QSAE_ERR_UNSUPPORTED, "%s: unsupported: %s", who, r.k_range);
    if (D < 4 || D % 4 != 0 || D > kLevelMaxD)
        return refuse(QSAE_ERR_UNSUPPORTED, "%s: unsupported: D a positive multiple of 4 up to 4096", who);
    if (packed && (n_bits < 1 || n_bits > 8)) return refuse(QSAE_ERR_UNSUPPORTED, "%s: unsupported: 1 <= n_bits <= 8", who);
    if ((unit_call || r.rows_check_Bk) && static_cast<long long>(B) * k >= (1LL << 31))
        return refuse(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * %s < 2^31", who, r.k);
    if (r.sizes == SizeCheck::kAfterLimits) QSAE_LEVEL_ARG(B >= 0 && H >= 1, "B >= 0 and H >= 1 required", who);
    QSAE_LEVEL_ARG(a != nullptr, "%s is null", who, r.array);
    lv->stride = static_cast<long long>(B) * D;
    lv->n = n;
    for (int i = 0; i < kMaxLevels; ++i) lv->bounds[i] = i < n ? a[i] : 0;
    bool ascending = true;
    for (int i = 0; i < n; ++i) ascending = ascending && a[i] > (i > 0 ? a[i - 1] : 0);
    QSAE_LEVEL_ARG(ascending && a[n - 1] == (r.ends_at_k ? k : H), "0 < %s[0] < ... < %s[%s - 1] == %s required", who, r.array,
                   r.array, r.count, r.ends_at_k ? "K" : "H");
    return QSAE_OK;
}

// ---- one launch per field width ---------------------------------------------------------------------------------------------
template <int M> struct FieldMode { static constexpr int value = M; };

// f(FieldMode<MODE>) with MODE 0 for the fp32 table and the field width 1, 2, 4 or 8 of a packed dictionary
template <class F>
inline void for_dict_mode(const NestedDict& d, F&& f) {
    switch (is_packed(d) ? field_width(d.n) : 0) {
        case 0: f(FieldMode<0>{}); break;
        case 1: f(FieldMode<1>{}); break;
        case 2: f(FieldMode<2>{}); break;
        case 4: f(FieldMode<4>{}); break;
        default: f(FieldMode<8>{}); break;
    }
}

// ---- the row gradient: G, gv and dx of nested_row_body ----------------------------------------------------------------------
// `launch(gl, lv)` starts the kernel of the family.  counts: nullptr where every row walks its whole list (ragged == false).
// empty_first: B == 0 returns before g is looked at (qsae_nested_batch.h) and not after (the other two).
template <class Launch>
inline int row_grad_levels(const char* who, const LevelRules& r, bool ragged, bool empty_first, const char* g_name,
                           const int32_t* idx, const int32_t* counts, int B, int k, const float* table, int H, int D,
                           const float* const* g, const int* a, int n, const float* g_latent, int64_t g_latent_ld,
                           const float* W_enc, float* G, float* gv, float* dx, Launch&& launch) {
    UnitLevels lv;
    if (const int rc = level_limits(who, r, false, B, k, H, D, false, 0, a, n, &lv); rc != QSAE_OK) return rc;
    if (empty_first && B == 0) return QSAE_OK;
    QSAE_LEVEL_ARG(g != nullptr, "%s is null", who, g_name);
    LevelGrads gl;
    for (int l = 0; l < kMaxLevels; ++l) gl.p[l] = l < n ? g[l] : nullptr;
    if (B == 0) return QSAE_OK;
    QSAE_LEVEL_ARG(table && G && (k == 0 || (idx && gv)) && (!ragged || counts), "null pointer", who);
    QSAE_LEVEL_ARG(!dx || W_enc, "dx needs W_enc", who);
    bool g_ok = true;
    for (int l = 0; l < kMaxLevels; ++l) g_ok = g_ok && aligned16(gl.p[l]);
    QSAE_LEVEL_ARG(g_ok && aligned16(table) && aligned16(G) && (!dx || (aligned16(dx) && aligned16(W_enc))),
                   "table, %s, G, W_enc and dx must be 16-byte aligned", who, g_name);
    QSAE_LEVEL_ARG(!misaligned(idx, 4) && !misaligned(counts, 4) && !misaligned(gv, 4) && !misaligned(g_latent, 4),
                   "idx, %sgv and g_latent must be 4-byte aligned", who, ragged ? "counts, " : "");
    QSAE_LEVEL_ARG(!g_latent || g_latent_ld >= 0, "g_latent_ld >= 0 required", who);
    launch(gl, lv);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
        snprintf(last_error_buf(), 512, "%s: hipGetLastError() failed: %s", who, hipGetErrorString(e));
        return QSAE_ERR_HIP;
    }
    return QSAE_OK;
}

// ---- the unit gradients: the checks of qsae_train_unit_grad / qsae_train_table_unit_grad before the sums of train.hip ------
inline size_t unit_grad_levels_bytes(const LevelRules& r, int B, int k, int H, int D) {
    if (k < r.k_min || k > kNestedMaxK || static_cast<long long>(B) * k >= (1LL << 31)) return 0;
    return qsae_train_unit_grad_workspace_bytes(B, k, H, D);
}
inline size_t table_unit_grad_levels_bytes(const LevelRules& r, int B, int k, int H, int D) {
    if (k < r.k_min) return 0;
    return qsae_train_table_unit_grad_workspace_bytes(B, k, H, D);
}

// Everything before the sums: the caller then runs train_unit_grad_levels or train_unit_grad_ranks (unit_levels.h) on lv
inline int unit_grad_levels_checks(const char* who, const LevelRules& r, const int32_t* offsets, const int32_t* entries,
                                   const float* val, const float* gv, int B, int k, const float* x, const float* G, const int* a,
                                   int n, const float* logits, int H, int D, int n_bits, const float* dW_enc,
                                   const float* dlogits, const void* workspace, size_t workspace_bytes, UnitLevels* lv) {
    if (const int rc = level_limits(who, r, true, B, k, H, D, true, n_bits, a, n, lv); rc != QSAE_OK) return rc;
    QSAE_LEVEL_ARG(offsets != nullptr, "null pointer", who);
    QSAE_LEVEL_ARG(static_cast<long long>(B) * k == 0 || (entries && val && gv && x), "null pointer", who);
    QSAE_LEVEL_ARG(!dlogits || logits, "dlogits needs logits", who);
    QSAE_LEVEL_ARG((!x || aligned16(x)) && aligned16(G) && (!dW_enc || aligned16(dW_enc)) &&
                   (!dlogits || (aligned16(dlogits) && aligned16(logits))),
                   "x, G, logits, dW_enc and dlogits must be 16-byte aligned", who);
    if (!workspace || workspace_bytes < unit_grad_levels_bytes(r, B, k, H, D))
        return refuse(QSAE_ERR_WORKSPACE, "%s: workspace missing or smaller than the sizer's bytes", who);
    return QSAE_OK;
}

// The same before train_table_unit_grad_levels or train_table_unit_grad_ranks
inline int table_unit_grad_levels_checks(const char* who, const LevelRules& r, const int32_t* offsets, const int32_t* entries,
                                         const float* val, const float* gv, int B, int k, const float* x, const float* G,
                                         const int* a, int n, int H, int D, const float* dW_enc, const float* dW_dec,
                                         int64_t dW_dec_ld, const void* workspace, size_t workspace_bytes, UnitLevels* lv) {
    if (const int rc = level_limits(who, r, true, B, k, H, D, false, 0, a, n, lv); rc != QSAE_OK) return rc;
    QSAE_LEVEL_ARG(offsets != nullptr, "null pointer", who);
    QSAE_LEVEL_ARG(static_cast<long long>(B) * k == 0 || (entries && val && gv && x), "null pointer", who);
    QSAE_LEVEL_ARG(!dW_dec || dW_dec_ld >= H, "dW_dec_ld >= H required", who);
    QSAE_LEVEL_ARG((!x || aligned16(x)) && aligned16(G) && (!dW_enc || aligned16(dW_enc)),
                   "x, G and dW_enc must be 16-byte aligned", who);
    if (!workspace || workspace_bytes < table_unit_grad_levels_bytes(r, B, k, H, D))
        return refuse(QSAE_ERR_WORKSPACE, "%s: workspace missing or smaller than the sizer's bytes", who);
    return QSAE_OK;
}

}  // namespace qsae
