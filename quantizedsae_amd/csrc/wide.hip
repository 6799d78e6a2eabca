// wide.hip -- per-row top-k over dictionaries wider than one selection kernel takes (include/qsae_wide.h, DESIGN.md section
// 4.40): qsaew_slab_plan cuts the hidden range into balanced slabs, qsaew_encode_topk / qsaew_encode_topk_prefilter run the
// existing selection forms of qsae.h on every slab's row range of W (views: nothing is copied) and qsaew_merge_topk joins the S
// lists of a row -- the S-way form of merge_topk_halves_kernel (encode_topk.hip).  No float atomics, no LDS, no scratch; every
// output element has exactly one writer.
#include "common.h"
#include "../../include/qsae_wide.h"

namespace qsae {

// the first unit of every slab and, behind the last one, H: by value in the kernel arguments, read with a workgroup-uniform index
struct WideStarts {
    int h[QSAEW_MAX_SLABS + 1];
};

// One thread per entry (s, r, j) of the part lists [S][B][k]; blockIdx.y = s.  rank = j + the entries of the row's other lists
// that go first: key >= own in the slabs below (lower units win a tie), key > own in the slabs above.  Both counts are prefixes
// of a list sorted by key descending, found by binary search.  A rank below k is the entry's place in the row's top-k; an entry
// that lost gives up its element of the dense latent, which its slab's call had written.
__global__ void __launch_bounds__(256)
merge_topk_parts_kernel(const int32_t* __restrict__ pidx, const float* __restrict__ pval, int S, int B, int k, WideStarts st,
                        int32_t* __restrict__ idx, float* __restrict__ val, float* __restrict__ dense, int64_t dense_ld) {
    const long long nk = static_cast<long long>(B) * k;
    const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int s = static_cast<int>(blockIdx.y);
    if (e >= nk) return;
    const int r = static_cast<int>(e / k), j = static_cast<int>(e % k);
    const float v = pval[s * nk + e];
    const uint32_t key = mono_key(v);
    int rank = j;
    for (int t = 0; t < S && rank < k; ++t) {
        if (t == s) continue;
        const float* other = pval + t * nk + static_cast<long long>(r) * k;
        int lo = 0, hi = k - rank;                        // a count of k - rank or more loses either way
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const uint32_t km = mono_key(other[mid]);
            if (t < s ? km >= key : km > key) lo = mid + 1; else hi = mid;
        }
        rank += lo;
    }
    const int h0 = st.h[s], width = st.h[s + 1] - h0;
    const int u = pidx[s * nk + e];
    if (rank < k) {
        idx[static_cast<long long>(r) * k + rank] = u + h0;
        val[static_cast<long long>(r) * k + rank] = v;
    } else if (dense != nullptr && u >= 0 && u < width) {
        dense[static_cast<long long>(r) * dense_ld + h0 + u] = 0.0f;
    }
}

// The plan of qsaew_slab_plan for operands already known to be positive: -> S, or 0 with *why set.
static int slab_plan(int H, int k, int slab, int* starts, const char** why) {
    *why = nullptr;
    if (H > QSAEW_MAX_H) { *why = "hidden_dim above 2^20"; return 0; }
    if (k > 256) { *why = "k above 256"; return 0; }
    if (H % 4 != 0) { *why = "hidden_dim must be a multiple of 4"; return 0; }
    if (slab > QSAEW_MAX_SLAB || slab % 256 != 0) { *why = "slab must be a multiple of 256 up to 32768"; return 0; }
    const int S = (H + slab - 1) / slab;
    if (S > QSAEW_MAX_SLABS) { *why = "more than 32 slabs"; return 0; }
    int h0 = 0;
    for (int s = 0; s < S; ++s) {
        const int rem = H - h0, parts = S - s;
        const int w = parts == 1 ? rem : ((rem + parts - 1) / parts + 255) / 256 * 256;
        if (w < k || w > rem) { *why = "a slab narrower than k"; return 0; }
        if (starts) starts[s] = h0;
        h0 += w;
    }
    if (starts) starts[S] = H;
    return S;
}

// Shape and argument checks shared by the encode entry points and their workspace functions (B apart): QSAE_OK with S and
// starts filled, or the code with the error text set.
static int wide_checks(const char* who, int D, int H, int k, int slab, int* starts, int* S) {
    const char* why = nullptr;
    if (H > 0 && k > 0 && slab > 0) *S = slab_plan(H, k <= H ? k : 1, slab, starts, &why);
    if (why) {
        snprintf(last_error_buf(), 512, "%s: unsupported: %s", who, why);
        return QSAE_ERR_UNSUPPORTED;
    }
    if (D > 0 && D % 4 != 0) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: input_dim must be a multiple of 4", who);
    if (!(D > 0 && H > 0 && k >= 1 && k <= H && slab > 0))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: D > 0, H > 0, 1 <= k <= H, slab > 0 required", who);
    return QSAE_OK;
}

struct WideLayout {
    size_t pidx, pval, slab_ws, total;
};

static size_t slab_ws_bytes(int B, int D, int w, int k, bool prefilter) {
    const size_t pre = prefilter ? qsae_encode_topk_prefilter_workspace_bytes(B, D, w, k) : 0;
    return pre ? pre : qsae_encode_topk_workspace_bytes(B, D, w, k);
}

// -> false where some slab has no form that takes it
static bool wide_layout(int B, int D, int k, int S, const int* starts, bool prefilter, WideLayout* L) {
    const size_t part = (static_cast<size_t>(S) * B * k * 4 + 255) / 256 * 256;
    size_t ws = 0;
    for (int s = 0; s < S; ++s) {
        const size_t need = slab_ws_bytes(B, D, starts[s + 1] - starts[s], k, prefilter);
        if (need == 0) return false;
        ws = need > ws ? need : ws;
    }
    L->pidx = 0;
    L->pval = part;
    L->slab_ws = 2 * part;
    L->total = 2 * part + ws;
    return true;
}

static size_t wide_workspace_bytes(int B, int D, int H, int k, int slab, bool prefilter) {
    int starts[QSAEW_MAX_SLABS + 1], S = 0;
    if (B <= 0 || wide_checks("qsaew", D, H, k, slab, starts, &S) != QSAE_OK) return 0;
    if (static_cast<long long>(B) * k >= (1ll << 31)) return 0;
    WideLayout L;
    return wide_layout(B, D, k, S, starts, prefilter, &L) ? L.total : 0;
}

static int wide_encode(const char* who, const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                       bool prefilter, int B, int D, int H, int k, int slab, int32_t* idx, float* val, float* dense,
                       int64_t dense_ld, void* workspace, size_t workspace_bytes, int spec_rows, int* flagged_rows,
                       qsae_stream_t stream) {
    int starts[QSAEW_MAX_SLABS + 1], S = 0;
    int rc = wide_checks(who, D, H, k, slab, starts, &S);
    if (rc != QSAE_OK) return rc;
    if (B < 0) return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: B >= 0 required", who);
    if (flagged_rows) *flagged_rows = 0;
    if (B == 0) return QSAE_OK;
    if (static_cast<long long>(B) * k >= (1ll << 31)) return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: B * k must be below 2^31", who);
    if (!(x && W && idx && val && workspace && (!prefilter || (Wq && meta))))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: null pointer", who);
    if (!(aligned16(x) && aligned16(W) && aligned16(workspace) && (!prefilter || aligned16(Wq))))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: 16-byte alignment", who);
    if (dense && !(dense_ld >= H && dense_ld % 4 == 0 && aligned16(dense)))
        return fail(QSAE_ERR_INVALID_ARG, "%s: invalid argument: dense latent alignment / ld", who);
    WideLayout L;
    if (!wide_layout(B, D, k, S, starts, prefilter, &L))
        return fail(QSAE_ERR_UNSUPPORTED, "%s: unsupported: no selection form takes a slab of this shape", who);
    if (workspace_bytes < L.total) return fail(QSAE_ERR_WORKSPACE, "%s: workspace too small", who);
    char* ws = static_cast<char*>(workspace);
    int32_t* pidx = reinterpret_cast<int32_t*>(ws + L.pidx);
    float* pval = reinterpret_cast<float*>(ws + L.pval);
    const size_t slab_bytes = workspace_bytes - L.slab_ws;
    const size_t nk = static_cast<size_t>(B) * k;
    int flagged = 0;
    // every slab's call uses the same scratch behind the part lists: the calls follow one another on `stream`
    for (int s = 0; s < S; ++s) {
        const int h0 = starts[s], w = starts[s + 1] - h0;
        const float* Ws = W + static_cast<size_t>(h0) * D;
        const float* bs = bias ? bias + h0 : nullptr;
        float* ds = dense ? dense + h0 : nullptr;
        if (prefilter && qsae_encode_topk_prefilter_workspace_bytes(B, D, w, k) > 0) {
            int f = 0;
            rc = qsae_encode_topk_prefilter(x, Ws, bs, static_cast<const char*>(Wq) + static_cast<size_t>(h0) * D * 2, meta, B, D, w, k,
                                            pidx + s * nk, pval + s * nk, ds, dense_ld, ws + L.slab_ws, slab_bytes, spec_rows, &f,
                                            stream);
            flagged += f;
        } else if (ds) {
            rc = qsae_encode_topk_latent(x, Ws, bs, B, D, w, k, pidx + s * nk, pval + s * nk, ds, dense_ld, /*kperm=*/0,
                                         ws + L.slab_ws, slab_bytes, stream);
        } else {
            rc = qsae_encode_topk(x, Ws, bs, B, D, w, k, pidx + s * nk, pval + s * nk, ws + L.slab_ws, slab_bytes, stream);
        }
        if (rc != QSAE_OK) return rc;
    }
    if (flagged_rows) *flagged_rows = flagged;
    return qsaew_merge_topk(pidx, pval, S, B, k, starts, idx, val, dense, dense_ld, stream);
}

}  // namespace qsae

using namespace qsae;

extern "C" int qsaew_slab_plan(int H, int k, int slab, int* starts) {
    const char* why = nullptr;
    int S = 0;
    if (H > 0 && k > 0 && slab > 0) S = slab_plan(H, k <= H ? k : 1, slab, starts, &why);
    if (why) {
        snprintf(last_error_buf(), 512, "%s: unsupported: %s", __func__, why);
        return QSAE_ERR_UNSUPPORTED;
    }
    QSAE_CHECK_ARG(H > 0 && k >= 1 && k <= H && slab > 0, "H > 0, 1 <= k <= H, slab > 0 required");
    return S;
}

extern "C" int qsaew_merge_topk(const int32_t* pidx, const float* pval, int S, int B, int k, const int* starts, int32_t* idx,
                                float* val, float* dense, int64_t dense_ld, qsae_stream_t stream) {
    QSAE_CHECK_SUPPORTED(S <= QSAEW_MAX_SLABS, "at most 32 slabs");
    QSAE_CHECK_SUPPORTED(B <= 0 || k <= 0 || static_cast<long long>(B) * k < (1ll << 31), "B * k must be below 2^31");
    QSAE_CHECK_ARG(S >= 1 && B >= 0 && k >= 1 && starts, "S >= 1, B >= 0, k >= 1, starts non-null required");
    WideStarts st{};
    QSAE_CHECK_ARG(starts[0] >= 0, "starts[0] >= 0 required");
    for (int s = 0; s < S; ++s) {
        QSAE_CHECK_ARG(static_cast<long long>(starts[s + 1]) - starts[s] >= k, "every slab must be at least k wide");
        st.h[s] = starts[s];
    }
    st.h[S] = starts[S];
    if (B == 0) return QSAE_OK;
    QSAE_CHECK_ARG(pidx && pval && idx && val, "null pointer");
    QSAE_CHECK_ARG(((reinterpret_cast<uintptr_t>(pidx) | reinterpret_cast<uintptr_t>(pval) | reinterpret_cast<uintptr_t>(idx) |
                     reinterpret_cast<uintptr_t>(val) | reinterpret_cast<uintptr_t>(dense)) & 3u) == 0, "4-byte alignment");
    QSAE_CHECK_ARG(!dense || dense_ld >= starts[S], "dense_ld below the last unit");
    const long long nk = static_cast<long long>(B) * k;
    hipLaunchKernelGGL(merge_topk_parts_kernel, dim3(static_cast<unsigned>((nk + 255) / 256), static_cast<unsigned>(S)), dim3(256), 0,
                       as_stream(stream), pidx, pval, S, B, k, st, idx, val, dense, dense_ld);
    QSAE_LAUNCH_CHECK();
    return QSAE_OK;
}

extern "C" size_t qsaew_encode_topk_workspace_bytes(int B, int D, int H, int k, int slab) {
    return wide_workspace_bytes(B, D, H, k, slab, false);
}

extern "C" size_t qsaew_encode_topk_prefilter_workspace_bytes(int B, int D, int H, int k, int slab) {
    return wide_workspace_bytes(B, D, H, k, slab, true);
}

extern "C" int qsaew_encode_topk(const float* x, const float* W, const float* bias, int B, int D, int H, int k, int slab,
                                 int32_t* idx, float* val, float* dense, int64_t dense_ld, void* workspace,
                                 size_t workspace_bytes, qsae_stream_t stream) {
    return wide_encode(__func__, x, W, bias, nullptr, nullptr, false, B, D, H, k, slab, idx, val, dense, dense_ld, workspace,
                       workspace_bytes, 0, nullptr, stream);
}

extern "C" int qsaew_encode_topk_prefilter(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                           int B, int D, int H, int k, int slab, int32_t* idx, float* val, float* dense,
                                           int64_t dense_ld, void* workspace, size_t workspace_bytes, int spec_rows,
                                           int* flagged_rows, qsae_stream_t stream) {
    return wide_encode(__func__, x, W, bias, Wq, meta, true, B, D, H, k, slab, idx, val, dense, dense_ld, workspace, workspace_bytes,
                       spec_rows, flagged_rows, stream);
}
