// The qsaew_* entry points (csrc/wide.hip) on the host stand-in runtime: the merge kernel's own source over part lists read from
// a file, and the whole slab selection with host stand-ins for the per-slab selection forms of qsae.h (they are other units'
// kernels; here each is a plain loop that honours the same contract: the slab's columns of the dense latent zeroed, the k
// survivors written, lists by key descending then unit ascending).  Guards of 0x5A lie around every buffer and read-only
// operands must keep their bytes.
#include "wide.hip"   // the kernel source (see tests/test_wide_emu_host.py)
#include "emu_driver.h"
#include <algorithm>

// ---- host stand-ins for the per-slab forms ------------------------------------------------------------------------------
static int g_slab_calls[3];                                  // prefilter, latent, compact
static uint32_t host_mono(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    if (v != v) return 0xFFFFFFFFu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// z = bias + sum_d x W, an fmaf chain in ascending d (the test's operands are small integers: every order gives these bits)
static int slab_select(const float* x, const float* W, const float* bias, int B, int D, int H, int k, int32_t* idx, float* val,
                       float* dense, int64_t ld) {
    std::vector<float> z(H);
    std::vector<int> order(H);
    for (int r = 0; r < B; ++r) {
        for (int h = 0; h < H; ++h) {
            float a = bias ? bias[h] : 0.0f;
            for (int d = 0; d < D; ++d) a = fmaf(x[(size_t)r * D + d], W[(size_t)h * D + d], a);
            z[h] = a;
            order[h] = h;
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return host_mono(z[a]) > host_mono(z[b]); });
        if (dense) for (int h = 0; h < H; ++h) dense[(size_t)r * ld + h] = 0.0f;
        for (int j = 0; j < k; ++j) {
            idx[(size_t)r * k + j] = order[j];
            val[(size_t)r * k + j] = z[order[j]];
            if (dense) dense[(size_t)r * ld + order[j]] = z[order[j]];
        }
    }
    return QSAE_OK;
}
// the prefilter "takes" slabs of at least 1024 units at batches of at least 4 rows here, so that a plan can mix both forms
extern "C" size_t qsae_encode_topk_prefilter_workspace_bytes(int B, int D, int H, int k) { return (B >= 4 && H >= 1024) ? 512 : 0; }
extern "C" size_t qsae_encode_topk_workspace_bytes(int B, int D, int H, int k) { return (B > 0 && H % 4 == 0 && k <= H) ? 256 : 0; }
extern "C" int qsae_encode_topk_prefilter(const float* x, const float* W, const float* bias, const void* Wq, const float* meta, int B,
                                          int D, int H, int k, int32_t* idx, float* val, float* dense, int64_t dense_ld, void* workspace,
                                          size_t workspace_bytes, int spec_rows, int* flagged_rows, qsae_stream_t) {
    if (workspace_bytes < 512 || !Wq || !meta) return QSAE_ERR_WORKSPACE;
    // the 16-bit copy must be the slab's own rows: the test stores unit h's first weight (a small integer >= 0) as a 16-bit
    // integer in the first element of row h
    const uint16_t* wq = static_cast<const uint16_t*>(Wq);
    for (int h = 0; h < H; ++h)
        if (wq[(size_t)h * D] != (uint16_t)(int)W[(size_t)h * D]) return QSAE_ERR_INVALID_ARG;
    memset(workspace, 0xA5, 512);
    ++g_slab_calls[0];
    *flagged_rows = 1;                                        // one flagged row per prefiltered slab: the sum is checked
    return slab_select(x, W, bias, B, D, H, k, idx, val, dense, dense_ld);
}
extern "C" int qsae_encode_topk_latent(const float* x, const float* W, const float* bias, int B, int D, int H, int k, int32_t* idx,
                                       float* val, float* dense, int64_t dense_ld, int kperm, void* workspace, size_t workspace_bytes,
                                       qsae_stream_t) {
    if (workspace_bytes < 256 || !dense || kperm) return QSAE_ERR_WORKSPACE;
    memset(workspace, 0xA5, 256);
    ++g_slab_calls[1];
    return slab_select(x, W, bias, B, D, H, k, idx, val, dense, dense_ld);
}
extern "C" int qsae_encode_topk(const float* x, const float* W, const float* bias, int B, int D, int H, int k, int32_t* idx, float* val,
                                void* workspace, size_t workspace_bytes, qsae_stream_t) {
    if (workspace_bytes < 256) return QSAE_ERR_WORKSPACE;
    memset(workspace, 0xA5, 256);
    ++g_slab_calls[2];
    return slab_select(x, W, bias, B, D, H, k, idx, val, nullptr, 0);
}

// usage: emu merge S B k with_dense ld starts in.bin out.bin    (starts "0,5,11": S + 1 ints; in: pidx pval [S][B][k], dense
//                                                               [B][ld] when with_dense; out: idx val [B][k], dense)
//        emu encode B D H k slab with_dense prefilter ld in.bin out.bin
//                                                              (in: x [B][D], W [H][D], bias [H], Wq [H][D] fp16 when prefilter;
//                                                               out: idx val [B][k], dense [B][ld] when with_dense, then four
//                                                               ints: flagged rows and the calls of the three slab forms)
int main(int argc, char** argv) {
    if (argc < 9) return 2;
    FILE* in = fopen(argv[argc - 2], "rb");
    if (!in) return 2;
    FILE* out = fopen(argv[argc - 1], "wb");
    if (argv[1][0] == 'm') {
        const int S = atoi(argv[2]), B = atoi(argv[3]), k = atoi(argv[4]), with_dense = atoi(argv[5]);
        const long long ld = atoll(argv[6]);
        int starts[QSAEW_MAX_SLABS + 1];
        if (parse_ints(argv[7], starts, QSAEW_MAX_SLABS + 1) != S + 1) return 2;
        const size_t part = (size_t)S * B * k * 4, lists = (size_t)B * k * 4;
        Guarded pidx(part), pval(part), idx(lists), val(lists), dense(with_dense ? (size_t)B * ld * 4 : 0);
        pidx.fill(in); pval.fill(in); dense.fill(in);
        int rc = qsaew_merge_topk(pidx.as<int32_t>(), pval.f(), S, B, k, starts, idx.as<int32_t>(), val.f(),
                                  with_dense ? dense.f() : nullptr, ld, nullptr);
        FAIL_RC(rc);
        if (!all_intact(pidx, pval, idx, val, dense) || !pidx.unchanged() || !pval.unchanged()) { printf("merge_topk: write outside\n"); return 1; }
        idx.dump(out); val.dump(out); dense.dump(out);
    } else {
        if (argc < 12) return 2;
        const int B = atoi(argv[2]), D = atoi(argv[3]), H = atoi(argv[4]), k = atoi(argv[5]), slab = atoi(argv[6]),
                  with_dense = atoi(argv[7]), prefilter = atoi(argv[8]);
        const long long ld = atoll(argv[9]);
        const size_t wb = prefilter ? qsaew_encode_topk_prefilter_workspace_bytes(B, D, H, k, slab)
                                    : qsaew_encode_topk_workspace_bytes(B, D, H, k, slab);
        if (wb == 0) { printf("workspace_bytes 0\n"); return 1; }
        const size_t lists = (size_t)B * k * 4;
        Guarded x((size_t)B * D * 4), W((size_t)H * D * 4), bias((size_t)H * 4), Wq(prefilter ? (size_t)H * D * 2 : 0), meta(16), ws(wb),
            idx(lists), val(lists), dense(with_dense ? (size_t)B * ld * 4 : 0);
        x.fill(in); W.fill(in); bias.fill(in); Wq.fill(in);
        memset(meta.data(), 0, 16);
        meta.before.assign(meta.data(), meta.data() + 16);
        int flagged = -1;
        int rc = prefilter ? qsaew_encode_topk_prefilter(x.f(), W.f(), bias.f(), Wq.data(), meta.f(), B, D, H, k, slab, idx.as<int32_t>(),
                                                         val.f(), with_dense ? dense.f() : nullptr, ld, ws.data(), wb, 0, &flagged, nullptr)
                           : qsaew_encode_topk(x.f(), W.f(), bias.f(), B, D, H, k, slab, idx.as<int32_t>(), val.f(),
                                               with_dense ? dense.f() : nullptr, ld, ws.data(), wb, nullptr);
        FAIL_RC(rc);
        if (!all_intact(x, W, bias, Wq, meta, ws, idx, val, dense) || !x.unchanged() || !W.unchanged() || !bias.unchanged() ||
            !Wq.unchanged() || !meta.unchanged()) { printf("encode_topk: write outside\n"); return 1; }
        idx.dump(out); val.dump(out); dense.dump(out);
        const int words[4] = {flagged, g_slab_calls[0], g_slab_calls[1], g_slab_calls[2]};
        fwrite(words, 4, 4, out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
