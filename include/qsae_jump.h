/*
 * qsae_jump.h -- JumpReLU for the top-k SAEs (Rajamanoharan et al. 2024, "Jumping Ahead"): one threshold per dictionary unit,
 * applied to the rows' top-K lists as a stable partition, and the thresholds' straight-through pseudo-gradient with the
 * rectangle kernel.  Entry points of libqsae_hip.so that are not yet part of qsae.h.
 *
 * A further extension header in the spirit of qsae_batch.h: qsae.h, the binding table _lib.SIGNATURES and their ledgers are
 * pinned to each other and are opened together.  The functions below are exported as qsaej_* from the same library
 * (csrc/jumprelu.hip), share its error text (qsae_last_error()), its conventions (qsae.h, "Conventions") and its return codes,
 * are bound from _lib.JUMP_SIGNATURES, and have a ledger of their own in tests/test_jumprelu_host.py (every function declared
 * here is bound, exported by the product and the debug library, and is either a *_bytes sizer or guarded in
 * tests/test_jumprelu_gpu.py).  They join qsae.h as qsae_* when the ledger is next opened; QSAE_ABI_VERSION does not move until
 * then.
 */
#ifndef QSAE_JUMP_H
#define QSAE_JUMP_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEJ_MAX_K 256        /* widest list (the cap per row) */
#define QSAEJ_REPORT_WORDS 6

/* -- Lists and thresholds -----------------------------------------------------------------------------------------------------
 * idx int32 [B][K] and val fp32 [B][K] are the lists qsae_encode_topk* writes at width K (the CAP, 1 <= K <= 256).  theta fp32
 * [H] lies on the device and is read as given: the front end takes the exponential of its log-parameter, no expf stands between
 * a restatement and the kernel.  eps is the bandwidth, half_eps = fl32(0.5f * eps) as the host computed it.
 *
 * -- qsaej_jump_select ---------------------------------------------------------------------------------------------------------
 * For the entry (r, j) with h = idx[r][j], v = val[r][j] and 0 <= h < H:
 *   selected     iff  v > theta[h]                         (a float compare: NaN on either side is not selected, v == theta
 *                                                           is not selected, -0 > +0 is false)
 *   in the band  iff  fabsf(v - theta[h]) < half_eps       (ONE fp32 subtraction, a strict compare; NaN is not in the band; an
 *                                                           entry is in the band whether it is selected or not)
 * An entry whose id lies outside [0, H) is neither.
 *
 *   idx_sel int32 [B][K], val_sel fp32 [B][K], counts int32 [B]: the STABLE PARTITION of row r by "selected" -- the selected
 *            entries first, in list order, then the others, in list order.  counts[r] = the selected entries; val_sel holds
 *            their values and +0 behind them; idx_sel is a permutation of the row's ids (ids outside [0, H) included, as
 *            given).  (idx_sel, val_sel) reads like any compact selection ("0 = inactive"), (idx_sel, val_sel, counts) like
 *            any ragged one (qsae_batch.h, "Ragged rows").  The selection is a subset of the list, not a prefix: thresholds
 *            differ by unit, so an entry ranked behind a rejected one may pass.
 *   idx_band int32 [B][K], counts_band int32 [B], both or neither: the same stable partition by "in the band".
 *   l0       fp32 [1] or NULL: fl32((double)selected / B), written by the same kernel chain.
 *   report   int64 [6] or NULL: {selected entries, band entries, rows with counts == K (saturated), rows with counts == 0
 *            (empty), uncertified rows, the bits of theta_min in the low 32 bits}.
 * theta_min is the smallest theta[h] under a float <, NaN skipped (of -0 and +0 the -0; the quiet NaN 0x7FC00000 when every
 * threshold is NaN); it is computed in the same chain and kept in the workspace.
 *
 * Row r is UNCERTIFIED iff K < H and not val[r][K - 1] < fl32(theta_min - half_eps).  Guarantee: for a certified row whose list
 * is what qsae_encode_topk* writes (the K largest pre-activations of the row, non-increasing), the selected set and the band
 * set equal those over the row's dense [H] pre-activations (DESIGN.md section 4.36 has the proof: a unit outside the list has a
 * value <= val[r][K - 1], and rounding is monotone).
 *
 * One wave per row, four entries per lane at K = 256, the places of the partition from 64-bit ballots and popcount prefixes; the
 * report is summed with 64-bit integer atomics only.  No float atomics, no sort: the same bits on every run, whatever the grid.
 * idx_sel, val_sel and idx_band must not overlap idx or val.
 *
 * Limits, checked before any launch and before any pointer is looked at, in this order: B >= 0, K >= 1, H >= 1, eps > 0 and
 * finite (QSAE_ERR_INVALID_ARG); K <= 256 and B * K < 2^31 (QSAE_ERR_UNSUPPORTED).  B == 0: QSAE_OK with nothing launched.
 * Then null or misaligned pointers (QSAE_ERR_INVALID_ARG; 4-byte alignment, report 8), then the workspace (QSAE_ERR_WORKSPACE
 * when missing or smaller than the sizer says; 256-byte aligned; it need not be zeroed).  The sizer returns 0 for shapes the
 * call refuses. */
size_t qsaej_jump_select_workspace_bytes(int B, int K, int H);
int qsaej_jump_select(const int32_t* idx, const float* val, int B, int K, const float* theta, int H, float eps, float half_eps,
                      int32_t* idx_sel, float* val_sel, int32_t* counts, int32_t* idx_band, int32_t* counts_band, float* l0,
                      int64_t* report, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- qsaej_threshold_grad ------------------------------------------------------------------------------------------------------
 * The pseudo-derivative of the paper with the rectangle kernel, for the JumpReLU and for the Heaviside step of the L0 term at
 * once.  offsets int32 [H + 1] and entries int32 are what qsaeb_csr_ragged writes over (idx_band, counts_band); gv_band fp32
 * [B][K] (nullable) is what qsaeb_row_grad_ragged writes over the same lists with dx = NULL, so that
 *   gv[e] = g_latent[r, h] + step * <g_recon[r], table[h]>     is exactly dL/dz of the entry e = r K + j.
 * For unit h with its n = offsets[h + 1] - offsets[h] entries in CSR order (ascending row):
 *   S         = sum of (double)gv_band[e], accumulated sequentially in fp64 from +0     (gv_band == NULL: S = +0)
 *   dtheta[h] = fl32( -( (double)theta[h] * S + (double)g_l0 * n / B ) / (double)eps )
 * evaluated left to right in fp64 -- the product, the product g_l0 * n, its quotient by B, the sum, the negation, the quotient
 * by eps -- with one rounding to fp32 at the end.  g_l0 is fp32 [1] on the device (the gradient that reached l0), or NULL, which
 * puts +0 in the term's place.  A unit without entries gets +0.  Offsets are clamped into [0, B K] and an entry outside
 * [0, B K) adds nothing: that is memory safety, not a contract.
 *
 * Limits and their order as above (no workspace).  B == 0: dtheta is written as zeros, nothing else is looked at. */
int qsaej_threshold_grad(const int32_t* offsets, const int32_t* entries, const float* gv_band, const float* theta,
                         const float* g_l0, int B, int K, int H, float eps, float* dtheta, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_JUMP_H */
