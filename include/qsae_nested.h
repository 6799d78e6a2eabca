/*
 * qsae_nested.h -- the nested-dictionary (Matryoshka) objective of the top-k SAEs: entry points of libqsae_hip.so that are not
 * yet part of qsae.h.
 *
 * A third extension header in the spirit of qsae_ext.h and qsae_curve.h: qsae.h, the binding table _lib.SIGNATURES and their
 * ledgers are pinned to each other and are opened together.  The functions below are exported as qsaen_* from the same library
 * (csrc/nested.hip; the unit sums run the kernels of csrc/train.hip), share its error text (qsae_last_error()), its conventions
 * (qsae.h, "Conventions") and its return codes, are bound from _lib.NESTED_SIGNATURES, and have a ledger of their own in
 * tests/test_nested_host.py (every function declared here is bound, exported by the product and the debug library, and is
 * either a *_bytes sizer or guarded in tests/test_nested_gpu.py).  They join qsae.h as qsae_* when the ledger is next opened;
 * QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_NESTED_H
#define QSAE_NESTED_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEN_MAX_LEVELS 8     /* most dictionary prefixes of one call */
#define QSAEN_MAX_K 256        /* longest top-k list */
#define QSAEN_MAX_D 4096       /* widest activation row */

/* -- One reconstruction per dictionary prefix (Bussmann et al., Matryoshka SAEs) ------------------------------------------ */
/* bounds is a HOST array of n_levels ints, read before the call returns: 0 < bounds[0] < ... < bounds[n_levels - 1] == H.
 * Level l is the dictionary prefix of the units below bounds[l]; level(h) is the smallest l with h < bounds[l].
 *
 * The sparse decoders sum a row's entries as one fmaf chain in ascending unit index, so the reconstruction from the units
 * below a bound is a prefix of that chain: one walk over a row's sorted list gives every level, and the last level is bit for
 * bit what qsae_decode_binary_sparse / qsae_decode_table_sparse return.
 *
 * Operands (device unless stated; the host reads none of the device operands):
 *   idx      int32 [B][k], val fp32 [B][k]: as qsae_encode_topk* writes them; the ids of a row are distinct
 *   packed, H, D, n_bits, step    the n-bit dictionary of qsae_pack_binary (4-byte aligned), or
 *   table, H, D, scale            fp32 [H][D], 16-byte aligned: the baseline decoder or BinarySAE's soft table
 *   dec_bias fp32 [D] or NULL
 *   recon    fp32 [n_levels][B][D], contiguous, 16-byte aligned
 *
 * Forward.  For row r, level l and column d, recon[l][r][d] is exactly what the sparse decoders return for the row's list with
 * the entries of units >= bounds[l] removed: the fmaf chain from +0 over the remaining entries in ascending unit index; then
 * fl32(step * chain) (packed; always) or fl32(scale * chain) (table; skipped when scale == 1); then fl32(. + bias[d]), or
 * fl32(. + (+0)) without a bias.  A removed entry takes no part at all -- it is not multiplied by zero -- so an inf or NaN
 * dictionary entry behind a bound, or a -0 accumulator, cannot show.  A level with no entry goes through the same two
 * roundings from a chain of +0 (the bias).  An id outside [0, H) contributes to no level and causes no read.
 *
 * Limits, checked before any launch and before any pointer is looked at: 1 <= n_levels <= 8, 0 <= k <= 256, D a positive
 * multiple of 4 up to 4096, 1 <= n_bits <= 8 (QSAE_ERR_UNSUPPORTED otherwise); B >= 0, H >= 1 (QSAE_ERR_INVALID_ARG).  Then
 * bounds (host) is read: QSAE_ERR_INVALID_ARG unless it is as above.  B == 0: QSAE_OK with nothing launched and no device
 * pointer looked at.  Then null or misaligned pointers (QSAE_ERR_INVALID_ARG).  k == 0: idx and val may be NULL, and every
 * level is written as a level with no entry. */
int qsaen_decode_nested_binary(const int32_t* idx, const float* val, int B, int k, const uint8_t* packed, int H, int D,
                               int n_bits, float step, const float* dec_bias, const int* bounds, int n_levels, float* recon,
                               qsae_stream_t stream);
int qsaen_decode_nested_table(const int32_t* idx, const float* val, int B, int k, const float* table, int H, int D, float scale,
                              const float* dec_bias, const int* bounds, int n_levels, float* recon, qsae_stream_t stream);

/* -- The gradient of a loss over the levels ----------------------------------------------------------------------------------
 * g_levels is a HOST array of n_levels device pointers, read before the call returns: g_levels[l] is the gradient arriving at
 * recon[l], fp32 [B][D], contiguous, 16-byte aligned, or NULL for a level the loss does not read (skipped, not added as zero).
 *
 * Suffix sums, fp32, written to G [n_levels][B][D] (16-byte aligned): with P the last level that has a gradient,
 *   G[P] = g[P];   G[l] = fl32(g[l] + G[l + 1]) for l < P with a gradient, G[l] = G[l + 1] for l < P without one;
 *   G[l] = +0 for l > P (and for every l when no level has a gradient).
 * G[level(h)] is the gradient that reaches the dictionary row of unit h; G[0] is the gradient of the decoder bias' rows
 * (qsae_train_col_sum(G[0]) is the decoder-bias gradient).
 *
 * qsaen_row_grad_nested: per selected entry (r, j) with unit h = idx[r][j] (clamped into [0, H) as qsae_train_row_grad does),
 *   gv[r][j] = g_latent[r][h] + step * <G[level(h)][r], table[h]>
 * in the operation order of qsae_train_row_grad with g_recon = G[level(h)], and dx (nullable) from gv exactly as there.
 * It writes G, gv and dx; k == 0: G is written, dx is zeros, gv is empty.
 *
 * qsaen_train_unit_grad_nested / qsaen_train_table_unit_grad_nested: per unit h what qsae_train_unit_grad /
 * qsae_train_table_unit_grad compute with g_recon replaced by G[level(h)] (G as qsaen_row_grad_nested wrote it, or NULL: no
 * reconstruction gradient); same operands, same workspace layout, same order of every sum.  No float atomics anywhere: the
 * same bits on every run.
 *
 * Limits and their order as above (the unit calls also refuse B * k >= 2^31, QSAE_ERR_UNSUPPORTED); B == 0: QSAE_OK with
 * nothing launched for qsaen_row_grad_nested; the unit calls then write their outputs as the calls they extend do (zeros).
 * Then null or misaligned pointers (QSAE_ERR_INVALID_ARG), then the workspace (QSAE_ERR_WORKSPACE when missing or smaller
 * than the sizer says). */
int qsaen_row_grad_nested(const int32_t* idx, int B, int k, const float* table, int H, int D, float step,
                          const float* const* g_levels, const int* bounds, int n_levels, const float* g_latent,
                          int64_t g_latent_ld, const float* W_enc, float* G, float* gv, float* dx, qsae_stream_t stream);
size_t qsaen_train_unit_grad_nested_workspace_bytes(int B, int k, int H, int D);
int qsaen_train_unit_grad_nested(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                                 const float* x, const float* G, const int* bounds, int n_levels, const float* logits, int H,
                                 int D, int n_bits, float step, const float* g_polarize, float* dW_enc, float* db_enc,
                                 float* dlogits, void* workspace, size_t workspace_bytes, qsae_stream_t stream);
size_t qsaen_train_table_unit_grad_nested_workspace_bytes(int B, int k, int H, int D);
int qsaen_train_table_unit_grad_nested(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                                       int k, const float* x, const float* G, const int* bounds, int n_levels, int H, int D,
                                       float* dW_enc, float* db_enc, float* dW_dec, int64_t dW_dec_ld, void* workspace,
                                       size_t workspace_bytes, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_NESTED_H */
