/*
 * qsae_multik.h -- the Multi-TopK objective of the top-k SAEs (Gao et al. 2024, L(k) + L(4k) / 8): entry points of
 * libqsae_hip.so that are not yet part of qsae.h.
 *
 * One more extension header in the spirit of qsae_curve.h and qsae_nested.h: qsae.h, the binding table _lib.SIGNATURES and their
 * ledgers are pinned to each other and are opened together.  The functions below are exported as qsaek_* from the same library
 * (csrc/multi_topk.hip; the unit sums run the kernels of csrc/train.hip), share its error text (qsae_last_error()), its
 * conventions (qsae.h, "Conventions") and its return codes, are bound from _lib.MULTIK_SIGNATURES, and have a ledger of their
 * own in tests/test_multi_topk_host.py (every function declared here is bound, exported by the product and the debug library,
 * and is either a *_bytes sizer or guarded in tests/test_multi_topk_gpu.py).  They join qsae.h as qsae_* when the ledger is next
 * opened; QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_MULTIK_H
#define QSAE_MULTIK_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEK_MAX_POINTS 8     /* most rank prefixes of one call */
#define QSAEK_MAX_K 256        /* longest top-K list */
#define QSAEK_MAX_D 4096       /* widest activation row */

/* -- One reconstruction per rank prefix ------------------------------------------------------------------------------------ */
/* ks is a HOST array of n_ks ints, read before the call returns: 0 < ks[0] < ... < ks[n_ks - 1] == K, where K is the width of
 * the lists idx / val [B][K].  A top-K list is ordered by rank with distinct keys (qsae_curve.h), so list position is rank and
 * the selection at ks[p] is the first ks[p] entries.  point(j) is the smallest p with j < ks[p]: the entry of rank j takes part
 * in the points p >= point(j) and in no other.
 *
 * Operands (device unless stated; the host reads none of the device operands):
 *   idx      int32 [B][K], val fp32 [B][K]: as qsae_encode_topk* writes them; the ids of a row are distinct
 *   packed, H, D, n_bits, step    the n-bit dictionary of qsae_pack_binary (4-byte aligned), or
 *   table, H, D, scale            fp32 [H][D], 16-byte aligned: the baseline decoder or BinarySAE's soft table
 *   dec_bias fp32 [D] or NULL
 *   recon    fp32 [n_ks][B][D], contiguous, 16-byte aligned
 *
 * Forward.  recon[p][r] is bit for bit what qsae_decode_binary_sparse / qsae_decode_table_sparse return for
 * idx[r][:ks[p]], val[r][:ks[p]]: the fmaf chain from +0 over those entries in ascending unit index; then fl32(step * chain)
 * (packed; always) or fl32(scale * chain) (table; skipped when scale == 1); then fl32(. + bias[d]), or fl32(. + (+0)) without a
 * bias -- the wording of qsae_curve.h, so it also equals recon_out of qsaec_prefix_errors_* bit for bit.  An entry of rank
 * >= ks[p] takes no part in point p at all -- it is not multiplied by zero -- so an inf or NaN dictionary entry behind a point
 * cannot show in it.  An id outside [0, H) causes no read and joins no chain.  A row's dictionary rows are gathered once for up
 * to four points; a call of more than four points makes one trip per four, the widest first.
 *
 * Limits, checked before any launch and before any pointer is looked at: 1 <= n_ks <= 8, 1 <= K <= 256, D a positive multiple
 * of 4 up to 4096, 1 <= n_bits <= 8 (QSAE_ERR_UNSUPPORTED otherwise); B >= 0, H >= 1 (QSAE_ERR_INVALID_ARG).  Then ks (host) is
 * read: QSAE_ERR_INVALID_ARG unless it is as above.  B == 0: QSAE_OK with nothing launched and no device pointer looked at.
 * Then null or misaligned pointers (QSAE_ERR_INVALID_ARG).  With n_ks == 1 (ks = [K]) the call is the plain sparse decode. */
int qsaek_decode_multik_binary(const int32_t* idx, const float* val, int B, int K, const uint8_t* packed, int H, int D,
                               int n_bits, float step, const float* dec_bias, const int* ks, int n_ks, float* recon,
                               qsae_stream_t stream);
int qsaek_decode_multik_table(const int32_t* idx, const float* val, int B, int K, const float* table, int H, int D, float scale,
                              const float* dec_bias, const int* ks, int n_ks, float* recon, qsae_stream_t stream);

/* -- The gradient of a loss over the points ---------------------------------------------------------------------------------
 * g_points is a HOST array of n_ks device pointers, read before the call returns: g_points[p] is the gradient arriving at
 * recon[p], fp32 [B][D], contiguous, 16-byte aligned, or NULL for a point the loss does not read (skipped, not added as zero).
 *
 * Suffix sums, fp32, written to G [n_ks][B][D] (16-byte aligned): with P the last point that has a gradient,
 *   G[P] = g[P];   G[p] = fl32(g[p] + G[p + 1]) for p < P with a gradient, G[p] = G[p + 1] for p < P without one;
 *   G[p] = +0 for p > P (and for every p when no point has a gradient).
 * G[point(j)] is the gradient that reaches the dictionary row of the entry of rank j; G[0] is the gradient of the decoder bias'
 * rows (qsae_train_col_sum(G[0]) is the decoder-bias gradient).
 *
 * qsaek_row_grad_multik: per entry (r, j) with unit h = idx[r][j] (clamped into [0, H) as qsae_train_row_grad does),
 *   gv[r][j] = g_latent[r][h] + step * <G[point(j)][r], table[h]>
 * in the operation order of qsae_train_row_grad with g_recon = G[point(j)], and dx (nullable) from gv exactly as there.
 *
 * qsaek_train_unit_grad_multik / qsaek_train_table_unit_grad_multik: what qsae_train_unit_grad / qsae_train_table_unit_grad
 * compute over the lists of qsae_train_csr(idx [B][K]), with g_recon[r] replaced, per entry e (the flat index r K + j the lists
 * hold), by G[point(e % K)][r] (G as qsaek_row_grad_multik wrote it, or NULL: no reconstruction gradient); same operands, same
 * workspace layout, same chunking of lists over 256 entries, same order of every sum.  No float atomics anywhere: the same
 * bits on every run.
 *
 * Limits and their order as above (the unit calls also refuse B * K >= 2^31, QSAE_ERR_UNSUPPORTED); B == 0: QSAE_OK with
 * nothing launched for qsaek_row_grad_multik; the unit calls then write their outputs as the calls they extend do (zeros).
 * Then null or misaligned pointers (QSAE_ERR_INVALID_ARG), then the workspace (QSAE_ERR_WORKSPACE when missing or smaller
 * than the sizer says).  With n_ks == 1 every call is bit for bit the plain call it extends. */
int qsaek_row_grad_multik(const int32_t* idx, int B, int K, const float* table, int H, int D, float step,
                          const float* const* g_points, const int* ks, int n_ks, const float* g_latent, int64_t g_latent_ld,
                          const float* W_enc, float* G, float* gv, float* dx, qsae_stream_t stream);
size_t qsaek_train_unit_grad_multik_workspace_bytes(int B, int K, int H, int D);
int qsaek_train_unit_grad_multik(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int K,
                                 const float* x, const float* G, const int* ks, int n_ks, const float* logits, int H, int D,
                                 int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc, float* dlogits,
                                 void* workspace, size_t workspace_bytes, qsae_stream_t stream);
size_t qsaek_train_table_unit_grad_multik_workspace_bytes(int B, int K, int H, int D);
int qsaek_train_table_unit_grad_multik(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                                       int K, const float* x, const float* G, const int* ks, int n_ks, int H, int D,
                                       float* dW_enc, float* db_enc, float* dW_dec, int64_t dW_dec_ld, void* workspace,
                                       size_t workspace_bytes, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_MULTIK_H */
