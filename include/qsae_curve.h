/*
 * qsae_curve.h -- the sparsity-fidelity curve: entry points of libqsae_hip.so that are not yet part of qsae.h.
 *
 * A second extension header in the spirit of qsae_ext.h: qsae.h, qsae_ext.h, the binding tables _lib.SIGNATURES and
 * _lib.EXT_SIGNATURES and their ledgers are pinned to each other and are opened together.  The functions below are exported
 * as qsaec_* from the same library (csrc/sparsity_curve.hip), share its error text (qsae_last_error()), its conventions
 * (qsae.h, "Conventions") and its return codes, are bound from _lib.CURVE_SIGNATURES, and have a ledger of their own in
 * tests/test_sparsity_curve_host.py (every function declared here is bound, exported by the product and the debug library,
 * and is either a *_bytes sizer or guarded in tests/test_sparsity_curve_gpu.py).  They join qsae.h as qsae_* when the ledger
 * is next opened; QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_CURVE_H
#define QSAE_CURVE_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEC_MAX_K 256        /* longest top-K list */
#define QSAEC_MAX_POINTS 16    /* most points k' of one call */
#define QSAEC_MAX_D 4096       /* widest activation row */

/* -- Reconstruction error at many k' from one top-K list (the test-time k sweep of Gao et al. 2024) ------------------- */
/* The top-k list of a row is ordered by (value descending, unit ascending) with distinct keys, so the selection at k' <= K
 * is the first k' entries of the top-K list; the sparse decoders sum a row's entries as one fmaf chain in ascending unit
 * index.  From ONE list per row these calls give the squared reconstruction error at every listed k', each point bit for bit
 * what the model gives when it is rebuilt with top_k = k', without a [B][D] reconstruction per point and without another
 * encoder pass: a row's dictionary rows are gathered once per four points and the chains of those points run side by side.
 *
 * Operands (device unless stated; the host reads none of the device operands):
 *   x        fp32 [B][D], contiguous, 4-byte aligned (every access is one element)
 *   idx      int32 [B][K], val fp32 [B][K]: as qsae_encode_topk* writes them.  List position is rank; the ids of a row are
 *            distinct; the values need not be ordered (the call never compares them)
 *   packed, H, D, n_bits, step    the n-bit dictionary of qsae_pack_binary (4-byte aligned), or
 *   table, H, D, scale            fp32 [H][D], 16-byte aligned: the baseline decoder or BinarySAE's soft table
 *   dec_bias fp32 [D] or NULL
 *   ks       HOST array of n_ks ints, read before the call returns
 *   sums     fp64 [n_ks], counts int64 [2] {rows kept, rows skipped}: running state, zeroed by the caller before the first
 *            call, 8-byte aligned
 *   recon_out  fp32 [n_ks][B][D] (4-byte aligned) or NULL
 *
 * Reconstruction.  For row r and point i, recon_i[r][.] is exactly what qsae_decode_binary_sparse / qsae_decode_table_sparse
 * return for the truncated lists idx[r][:ks[i]], val[r][:ks[i]]: per column the fmaf chain from +0 over those entries in
 * ascending unit index; then fl32(step * chain) (packed; always) or fl32(scale * chain) (table; skipped when scale == 1);
 * then fl32(. + bias[d]), or fl32(. + (+0)) without a bias.  An entry of rank >= ks[i] takes no part in chain i at all -- it
 * is not multiplied by zero -- so an inf or NaN dictionary entry behind it, or a -0 accumulator, cannot show.  ks[i] == 0
 * gives the bias, or +0 without one.
 * Ids outside [0, H): such an entry causes no read out of range and contributes to no chain.
 *
 * Error terms.  t = fl32(e * e) with e = fl32(recon_i[r][d] - x[r][d]): the terms of qsae_sq_err_sum and of
 * qsae_dataset_moments_add.  Each term is widened to fp64 (exact) and summed in fp64.
 *
 * Row groups.  The rows of a call are cut into groups of group_rows from its first row (the last may be short).  A group
 * holding a NaN in x adds nothing to sums and its rows go to counts[1]; the rows of the other groups go to counts[0]: the
 * rule of qsae_dataset_moments_add, so the curve and the moments count the same rows.
 *
 * Order of the sums -- a function of (B, D, group_rows, n_ks) alone, never of the grid, the CU count or the dictionary's
 * format; no float atomic; the same bits on every run:
 *   row r, point i:  the columns are taken in octets o = d / 8 (the last octet holds 4 columns when D % 8 == 4).  Slot
 *       s = o % 64 (64 slots) adds to 0.0 the terms of its octets in ascending column order (slots without a column keep
 *       0.0); the 64 slot sums are joined by a butterfly, v[s] += v[s ^ m] for m = 32, 16, 8, 4, 2, 1 (both partners of a
 *       step use the values from before the step); the row sum is v[0];
 *   group g, point i:  the row sums of its rows are added to 0.0 in ascending row order;
 *   sums[i] = (((sums[i] + group sum g0) + group sum g1) + ...) over the unflagged groups in ascending order.
 * Hence the same bits whether the rows arrive in one call or in several calls cut at multiples of group_rows.
 *
 * recon_out, when given, receives all n_ks reconstructions of every row, the rows of flagged groups included.
 *
 * Limits, checked before any launch and before any pointer is looked at: 1 <= n_ks <= 16, K <= 256, D a positive multiple
 * of 4 up to 4096, 1 <= n_bits <= 8 (QSAE_ERR_UNSUPPORTED otherwise); B >= 0, H >= 1, group_rows >= 1
 * (QSAE_ERR_INVALID_ARG).  Then ks (host) is read: 0 <= ks[0] < ... < ks[n_ks - 1] <= K, else QSAE_ERR_INVALID_ARG.
 * B == 0: QSAE_OK with nothing launched and no device pointer looked at.  Then null or misaligned pointers
 * (QSAE_ERR_INVALID_ARG) and the workspace (QSAE_ERR_WORKSPACE when missing, smaller than the sizer says or not 8-byte
 * aligned).
 * workspace: qsaec_prefix_errors_*_workspace_bytes(B, n_ks, group_rows) bytes (a sum per row and point, a flag per row,
 * a sum per group and point, a flag per group; 0 for B < 1 or a refused n_ks or group_rows).  It need not be zeroed, and
 * nothing in it is read by a later call. */
size_t qsaec_prefix_errors_binary_workspace_bytes(int B, int n_ks, int group_rows);
int qsaec_prefix_errors_binary(const float* x, const int32_t* idx, const float* val, int B, int K, const uint8_t* packed, int H,
                               int D, int n_bits, float step, const float* dec_bias, const int* ks, int n_ks, int group_rows,
                               double* sums, int64_t* counts, float* recon_out, void* workspace, size_t workspace_bytes,
                               qsae_stream_t stream);
size_t qsaec_prefix_errors_table_workspace_bytes(int B, int n_ks, int group_rows);
int qsaec_prefix_errors_table(const float* x, const int32_t* idx, const float* val, int B, int K, const float* table, int H,
                              int D, float scale, const float* dec_bias, const int* ks, int n_ks, int group_rows, double* sums,
                              int64_t* counts, float* recon_out, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_CURVE_H */
