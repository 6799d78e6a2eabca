/*
 * qsae_jump_dense.h -- the dense (uncapped) JumpReLU encoder of the top-k SAEs: the encoder's exact-fp32 contraction with the
 * per-unit thresholds of qsae_jump.h applied in its epilogue, so that a row's firing units are found among all H
 * pre-activations and not among a top-K list.  Entry points of libqsae_hip.so that are not yet part of qsae.h.
 *
 * A further extension header in the spirit of qsae_jump.h: qsae.h, the binding table _lib.SIGNATURES and their ledgers are
 * pinned to each other and are opened together.  The functions below are exported as qsaed_* from the same library
 * (csrc/jump_dense.hip), share its error text (qsae_last_error()), its conventions (qsae.h, "Conventions") and its return
 * codes, are bound from _lib.JUMP_DENSE_SIGNATURES, and have a ledger of their own in tests/test_jump_dense_host.py (every
 * function declared here is bound, exported by the product and the debug library, and is either a *_bytes sizer or guarded in
 * tests/test_jump_dense_gpu.py).  They join qsae.h as qsae_* when the ledger is next opened; QSAE_ABI_VERSION does not move
 * until then.
 */
#ifndef QSAE_JUMP_DENSE_H
#define QSAE_JUMP_DENSE_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAED_MAX_K 256        /* widest list per row */
#define QSAED_REPORT_WORDS 6

/* -- qsaed_encode_jump ---------------------------------------------------------------------------------------------------------
 * x fp32 [B][ldx], W fp32 [H][ldw] (the encoder's weight, one row per unit), bias fp32 [H] or NULL, theta fp32 [H], all on the
 * device.  theta is read as given (the front end takes the exponential of its log-parameter).  eps is the bandwidth, half_eps
 * = fl32(0.5f * eps) as the host computed it.
 *
 * Pre-activation.  z[r][h] is the encoder pre-activation of DESIGN.md section 2: the fp32 fmaf chain over k = 0 .. D - 1 in
 * ascending order, seeded with bias[h] (+0 without a bias) -- the bits qsae_encode_dense writes and oracle.encode computes.
 *
 * Predicates, exactly those of qsae_jump.h, over every unit h of [0, H):
 *   selected     iff  z > theta[h]                         (a float compare: NaN on either side is not selected, z == theta
 *                                                           is not selected, -0 > +0 is false)
 *   in the band  iff  fabsf(z - theta[h]) < half_eps       (ONE fp32 subtraction, a strict compare; NaN is not in the band; a
 *                                                           unit is in the band whether it is selected or not)
 *
 * Rank order.  The library's: value descending (-0 and +0 are one value), then unit ascending.
 *
 *   idx_sel int32 [B][K], val_sel fp32 [B][K], counts int32 [B]: the selected units of row r in rank order, the first K of them
 *            when more than K fire; counts[r] = min(n_sel(r), K), n_sel(r) the number of selected units of the row.  val_sel
 *            holds the bits of z.  Behind the prefix idx_sel = -1 and val_sel = +0 (the convention of qsaex_encode_topk_units
 *            for short lists).  (idx_sel, val_sel, counts) reads like any ragged selection (qsae_batch.h, "Ragged rows").
 *   idx_band int32 [B][K], counts_band int32 [B], both or neither: the same for the units in the band, -1 behind the prefix.
 *   l0       fp32 [1] or NULL: fl32((double)(sum over r of n_sel(r)) / B) -- the UNCAPPED counts.
 *   report   int64 [6] or NULL: {sum of counts, sum of min(n_band, K) (computed with or without the band lists), rows with
 *            n_sel > K (truncated), rows with counts == 0 (empty), rows with n_band > K, sum of n_sel uncapped}.
 *
 * Exact for every row: there is no certificate.  A row with more than K firing units gets the K largest in rank order, however
 * many such rows there are.  The chain: the contraction on the fp32 matrix cores (128 x 128 tiles, the rows of W split over at
 * most 8 workgroups per panel of 128 rows of x) appends every unit that is selected or in the band to a region of the workspace
 * that belongs to one (split, row); one wave per row joins the regions and ranks them.  A row one of whose regions overflowed,
 * or with more than 512 such units, is recomputed by a third kernel from the fmaf chain itself (the same bits) and its lists
 * are taken by a radix search over the 64-bit rank keys.  Which path a row takes is a function of the operands alone.  Integer
 * atomics hand out places inside a region and sum the report; no output depends on their arrival order (every list is ranked by
 * keys that are distinct within a row).  No float atomics: the same bits on every run, whatever the grid.
 *
 * Limits, checked before any launch and before any pointer is looked at, in this order: B >= 0, K >= 1, H >= 1, eps > 0 and
 * finite (QSAE_ERR_INVALID_ARG); K <= 256, K <= H, D a positive multiple of 4, B * K < 2^31, H <= 2^30 (QSAE_ERR_UNSUPPORTED).
 * B == 0: QSAE_OK with nothing launched.  Then ldx and ldw (>= D and multiples of 4), null or misaligned pointers (x and W
 * 16-byte aligned; the others 4-byte, report 8; QSAE_ERR_INVALID_ARG), then the workspace (QSAE_ERR_WORKSPACE when missing or
 * smaller than the sizer says; 256-byte aligned; it need not be zeroed).  The sizer returns 0 for shapes the call refuses.
 * The outputs must not overlap the operands. */
size_t qsaed_encode_jump_workspace_bytes(int B, int D, int H, int K);
int qsaed_encode_jump(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, const float* theta, int B,
                      int D, int H, int K, float eps, float half_eps, int32_t* idx_sel, float* val_sel, int32_t* counts,
                      int32_t* idx_band, int32_t* counts_band, float* l0, int64_t* report, void* workspace,
                      size_t workspace_bytes, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_JUMP_DENSE_H */
