/*
 * qsae_nested_batch.h -- the nested-dictionary (Matryoshka) objective over the ragged rows of BatchTopK: one reconstruction per
 * dictionary prefix from the first counts[r] entries of every row's top-K list, and the row side of the gradient of a loss that
 * sums over the prefixes.  Entry points of libqsae_hip.so that are not yet part of qsae.h.
 *
 * A fifth extension header in the spirit of qsae_ext.h, qsae_curve.h, qsae_nested.h and qsae_batch.h: qsae.h, the binding table
 * _lib.SIGNATURES and their ledgers are pinned to each other and are opened together.  The functions below are exported as
 * qsaem_* from the same library (csrc/nested_ragged.hip; the kernel bodies are those of csrc/nested.hip, csrc/nested_rows.h),
 * share its error text (qsae_last_error()), its conventions (qsae.h, "Conventions") and its return codes, are bound from
 * _lib.NESTED_BATCH_SIGNATURES, and have a ledger of their own in tests/test_nested_ragged_host.py (every function declared
 * here is bound, exported by the product and the debug library, and guarded in tests/test_nested_ragged_gpu.py).  They
 * join qsae.h as qsae_* when the ledger is next opened; QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_NESTED_BATCH_H
#define QSAE_NESTED_BATCH_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEM_MAX_LEVELS 8     /* most dictionary prefixes of one call */
#define QSAEM_MAX_K 256        /* widest list (the cap per row) */
#define QSAEM_MAX_D 4096       /* widest activation row */

/* -- Lists, prefixes and levels -----------------------------------------------------------------------------------------------
 * idx int32 [B][K], val fp32 [B][K] and counts int32 [B] are what qsae_encode_topk* and qsaeb_batch_select /
 * qsaeb_threshold_select write (qsae_batch.h): row r keeps the first c(r) = min(max(counts[r], 0), K) entries of its rank
 * ordered list.  Only these entries are ever read.  An entry behind the prefix takes no part at all: it is not multiplied by
 * zero, its dictionary row is not read -- so an inf or NaN dictionary row or value behind a prefix, or a -0 accumulator, cannot
 * show.
 *
 * bounds is a HOST array of n_levels ints, read before the call returns: 0 < bounds[0] < ... < bounds[n_levels - 1] == H
 * (qsae_nested.h).  Level l is the dictionary prefix of the units below bounds[l]; level(h) is the smallest l with
 * h < bounds[l].
 *
 * -- One reconstruction per dictionary prefix -------------------------------------------------------------------------------
 * Operands (device unless stated; the host reads none of the device operands):
 *   packed, H, D, n_bits, step    the n-bit dictionary of qsae_pack_binary (4-byte aligned), or
 *   table, H, D, scale            fp32 [H][D], 16-byte aligned: the baseline decoder or BinarySAE's soft table
 *   dec_bias      fp32 [D] or NULL
 *   recon         fp32 [n_levels][B][D], contiguous, 16-byte aligned
 *   counts_below  int32 [n_levels][B] or NULL: the kept entries (in the prefix, id in [0, H)) of row r below bounds[l]
 *
 * recon[l][r] is bit for bit what qsaen_decode_nested_binary / _table return for the row's list truncated to c(r) entries: the
 * fmaf chain from +0 over the kept entries of units below bounds[l] in ascending unit id; then fl32(step * chain) (packed;
 * always) or fl32(scale * chain) (table; skipped when scale == 1); then fl32(. + bias[d]), or fl32(. + (+0)) without a bias.
 * An id outside [0, H) is dropped, as there: it contributes to no level and causes no read (a clamped id would have no
 * meaningful level).  A level with no entry, and a row with c(r) == 0, go through the same two roundings from a chain of +0.
 * With n_levels == 1 and every prefix id in range, recon[0] is qsaeb_decode_ragged_* bit for bit; with every c(r) == K the
 * result is qsaen_decode_nested_* at k = K.  One walk over a row's sorted prefix gives every level; counts_below are the
 * wave-uniform numbers that steer the walk, stored by one lane.  No atomics.
 *
 * -- The row side of the gradient ---------------------------------------------------------------------------------------------
 * g_levels is a HOST array of n_levels device pointers, read before the call returns: g_levels[l] is the gradient arriving at
 * recon[l], fp32 [B][D], contiguous, 16-byte aligned, or NULL for a level the loss does not read (skipped, not added as zero).
 *
 * qsaem_row_grad_nested_ragged writes
 *   G   fp32 [n_levels][B][D] (16-byte aligned): the suffix sums of qsaen_row_grad_nested, for every row, whatever counts is;
 *   gv  fp32 [B][K]: for j < c(r) the value of qsaen_row_grad_nested (unit h = idx[r][j] clamped into [0, H),
 *       gv = g_latent[r][h] + step * <G[level(h)][r], table[h]>); for j >= c(r) it is written as +0;
 *   dx  fp32 [B][D] or NULL: the fmaf chain of gv[r][j] * W_enc[h] over the first c(r) entries in list order (ids clamped).
 * With every c(r) == K this is qsaen_row_grad_nested bit for bit; with n_levels == 1 it is qsaeb_row_grad_ragged with
 * g_recon = g_levels[0].
 *
 * The unit sums need no call of their own: qsaeb_csr_ragged (k = K) lists exactly the kept entries as r * K + j, and
 * qsaen_train_unit_grad_nested / qsaen_train_table_unit_grad_nested address entries through those lists, so with val_sel, gv
 * and G from above they never reach an entry behind a prefix.  No float atomics anywhere: the same bits on every run.
 *
 * Limits, checked in this order before any launch and before any pointer is looked at: B >= 0, K >= 1, H >= 1
 * (QSAE_ERR_INVALID_ARG); K <= 256, 1 <= n_levels <= 8, D a positive multiple of 4 up to 4096, 1 <= n_bits <= 8,
 * B * K < 2^31 (QSAE_ERR_UNSUPPORTED).  Then bounds (host) is read: QSAE_ERR_INVALID_ARG unless it is as above.  B == 0:
 * QSAE_OK with nothing launched and no other pointer looked at.  Then null (g_levels itself included) or misaligned pointers
 * (QSAE_ERR_INVALID_ARG). */
int qsaem_decode_nested_ragged_binary(const int32_t* idx, const float* val, const int32_t* counts, int B, int K,
                                      const uint8_t* packed, int H, int D, int n_bits, float step, const float* dec_bias,
                                      const int* bounds, int n_levels, float* recon, int32_t* counts_below, qsae_stream_t stream);
int qsaem_decode_nested_ragged_table(const int32_t* idx, const float* val, const int32_t* counts, int B, int K, const float* table,
                                     int H, int D, float scale, const float* dec_bias, const int* bounds, int n_levels,
                                     float* recon, int32_t* counts_below, qsae_stream_t stream);
int qsaem_row_grad_nested_ragged(const int32_t* idx, const int32_t* counts, int B, int K, const float* table, int H, int D,
                                 float step, const float* const* g_levels, const int* bounds, int n_levels, const float* g_latent,
                                 int64_t g_latent_ld, const float* W_enc, float* G, float* gv, float* dx, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_NESTED_BATCH_H */
