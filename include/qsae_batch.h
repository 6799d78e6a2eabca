/*
 * qsae_batch.h -- BatchTopK for the top-k SAEs (Bussmann et al.): a batch-wide exact selection over the rows' top-K lists, the
 * threshold selection of inference, and the row-side operations on ragged rows.  Entry points of libqsae_hip.so that are not
 * yet part of qsae.h.
 *
 * A fourth extension header in the spirit of qsae_ext.h, qsae_curve.h and qsae_nested.h: qsae.h, the binding table
 * _lib.SIGNATURES and their ledgers are pinned to each other and are opened together.  The functions below are exported as
 * qsaeb_* from the same library (csrc/batch_topk.hip, csrc/batch_topk_decode.hip), share its error text (qsae_last_error()),
 * its conventions (qsae.h, "Conventions") and its return codes, are bound from _lib.BATCH_SIGNATURES, and have a ledger of
 * their own in tests/test_batch_topk_host.py (every function declared here is bound, exported by the product and the debug
 * library, and is either a *_bytes sizer or guarded in tests/test_batch_topk_gpu.py).  They join qsae.h as qsae_* when the
 * ledger is next opened; QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_BATCH_H
#define QSAE_BATCH_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEB_MAX_K 256        /* widest list (the cap per row) */
#define QSAEB_MAX_D 4096       /* widest activation row */

/* -- Lists and their order ----------------------------------------------------------------------------------------------------
 * idx int32 [B][K] and val fp32 [B][K] are the lists qsae_encode_topk* writes at width K (the CAP, 1 <= K <= 256): rank
 * ordered, value descending, then unit ascending.  The key of an entry is mono_key(val) descending (csrc/common.h: NaN first,
 * then +inf, ..., -0 == +0, ..., -inf), then row ascending, then list position ascending.  Precondition of the prefix
 * property: every row is non-increasing in mono_key.  Rows that are not are still handled safely and exactly by the key order
 * (sum(counts) == n_select, val_sel holds exactly the selected entries), but a row's selected entries are then no prefix.
 *
 * -- Batch selection ---------------------------------------------------------------------------------------------------------
 * The n_select first entries in key order are selected (0 <= n_select <= B * K; the front end passes B * k).
 *   counts   int32 [B]: the selected entries of row r -- under the precondition a prefix of its list
 *   val_sel  fp32 [B][K] or NULL: val where selected, +0 elsewhere ("0 = inactive", what every consumer of (idx, val) reads)
 *   report   int64 [4] or NULL: {selected, rows with counts == K (saturated), rows with counts == 0 (empty), the bits of the
 *            smallest selected value -- the value of the LAST selected entry in key order -- in the low 32 bits (0 when
 *            nothing is selected)}
 * This is BatchTopK capped at K per row; it equals BatchTopK over the dense [B][H] pre-activations whenever report[1] == 0 (a
 * unit outside a row's top-K can beat the threshold only if the row's K-th entry does too).
 *
 * Threshold state (theta fp32 [1] and batches int64 [1], device, both or neither): with m the smallest selected value, if
 * anything is selected and m > 0:  theta <- m when batches == 0, else theta <- fl32(theta + fl32(lr * fl32(m - theta)));
 * batches += 1.  Otherwise neither is written.  The update is part of the same kernel chain; the host reads nothing.
 *
 * The k-th key is found exactly by three radix passes (11 + 11 + 10 bits) with per-workgroup LDS histograms and integer
 * atomics; ties at the boundary key go to the lowest (row, position) through per-row tie counts and an exclusive prefix over
 * the rows.  No float atomics, no sort: the same bits on every run, whatever the grid.
 *
 * Limits, checked before any launch and before any pointer is looked at: K <= 256 and B * K < 2^31 (QSAE_ERR_UNSUPPORTED);
 * B >= 0, K >= 1, 0 <= n_select <= B * K (QSAE_ERR_INVALID_ARG).  B == 0: QSAE_OK with nothing launched.  Then null or
 * misaligned pointers (QSAE_ERR_INVALID_ARG), then the workspace (QSAE_ERR_WORKSPACE when missing or smaller than the sizer
 * says; 256-byte aligned; it need not be zeroed).  The sizers return 0 for shapes the calls refuse. */
size_t qsaeb_batch_select_workspace_bytes(int B, int K);
int qsaeb_batch_select(const float* val, int B, int K, int64_t n_select, int32_t* counts, float* val_sel, int64_t* report,
                       float* theta, int64_t* batches, float lr, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- Threshold selection -----------------------------------------------------------------------------------------------------
 * counts[r] = the length of the longest prefix of row r with val >= theta (a float compare: NaN, in the list or as theta,
 * ends the prefix; -0 >= +0).  theta is read from theta_dev (device, fp32 [1]) or, when that is NULL, is theta_host.  val_sel
 * and report as above (the selected entries are the prefixes).  Limits and their order as above. */
size_t qsaeb_threshold_select_workspace_bytes(int B, int K);
int qsaeb_threshold_select(const float* val, int B, int K, const float* theta_dev, float theta_host, int32_t* counts,
                           float* val_sel, int64_t* report, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- Ragged rows -------------------------------------------------------------------------------------------------------------
 * Every call below reads only the first c(r) = min(max(counts[r], 0), K) entries of row r.  An entry behind the prefix takes
 * no part at all: it is not multiplied by zero, its dictionary row is not read.
 *
 * qsaeb_decode_ragged_binary / _table: recon[r] (fp32 [B][D], the table form 16-byte aligned) is bit for bit what
 * qsae_decode_binary_sparse / qsae_decode_table_sparse return for the list truncated to c(r) entries (ids clamped into
 * [0, H) as there); c(r) == 0 gives the bias, or +0 without one.
 *
 * qsaeb_row_grad_ragged: gv[r][j] for j < c(r) and dx[r] (nullable) are bit for bit qsae_train_row_grad on the truncated
 * list; gv[r][j] for j >= c(r) is written as +0.
 *
 * qsaeb_csr_ragged: offsets int32 [H + 1] and entries int32 (room for B * K) as qsae_train_csr writes them, over the entries
 * (r, j) with j < c(r) and 0 <= idx[r][j] < H (other ids are dropped): entry r * K + j, grouped by unit, ordered by row within
 * a unit; the lists fill the first offsets[H] places of `entries`, the rest is written as -1.  With every c(r) == K and every id in
 * range this is qsae_train_csr bit for bit.  The result feeds qsae_train_unit_grad / qsae_train_table_unit_grad with k = K
 * (they address entries as r * k + j) together with val_sel and gv.
 *
 * Limits, in this order: B >= 0, K >= 1, H >= 1 (QSAE_ERR_INVALID_ARG); K <= 256, D a positive multiple of 4 up to 4096,
 * 1 <= n_bits <= 8, B * K < 2^31 (QSAE_ERR_UNSUPPORTED).  B == 0: QSAE_OK with nothing launched (qsaeb_csr_ragged then still
 * writes offsets as zeros).  Then null or misaligned pointers (QSAE_ERR_INVALID_ARG), then the workspace. */
int qsaeb_decode_ragged_binary(const int32_t* idx, const float* val, const int32_t* counts, int B, int K, const uint8_t* packed,
                               int H, int D, int n_bits, float step, const float* dec_bias, float* recon, qsae_stream_t stream);
int qsaeb_decode_ragged_table(const int32_t* idx, const float* val, const int32_t* counts, int B, int K, const float* table,
                              int H, int D, float scale, const float* dec_bias, float* recon, qsae_stream_t stream);
int qsaeb_row_grad_ragged(const int32_t* idx, const int32_t* counts, int B, int K, const float* table, int H, int D, float step,
                          const float* g_recon, const float* g_latent, int64_t g_latent_ld, const float* W_enc, float* gv,
                          float* dx, qsae_stream_t stream);
size_t qsaeb_csr_ragged_workspace_bytes(int B, int K, int H);
int qsaeb_csr_ragged(const int32_t* idx, const int32_t* counts, int B, int K, int H, int32_t* offsets, int32_t* entries,
                     void* workspace, size_t workspace_bytes, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_BATCH_H */
