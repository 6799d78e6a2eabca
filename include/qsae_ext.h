/*
 * qsae_ext.h -- entry points of libqsae_hip.so that are not yet part of qsae.h.
 *
 * qsae.h, the binding table _lib.SIGNATURES and the ledgers of tests/test_host.py, tests/test_analysis_guards_host.py and
 * tests/test_train_guards_host.py are pinned to each other; they are opened together.  What is added between two such
 * openings lives here: the functions below are exported as qsaex_* from the same library (csrc/auxk.hip), share its error
 * text (qsae_last_error()), its conventions (qsae.h, "Conventions") and its return codes, are bound from
 * _lib.EXT_SIGNATURES, and have a ledger of their own in tests/test_auxk_host.py (every function declared here is bound
 * and is either a *_bytes sizer or guarded in tests/test_auxk_gpu.py).  They join qsae.h as qsae_* when the ledger is next
 * opened; QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_EXT_H
#define QSAE_EXT_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- AuxK (Gao et al. 2024, "Scaling and evaluating sparse autoencoders", the auxiliary loss of the top-k SAE) -------- */
/* Encoder plus top-k over a LIST of units: what qsae_encode_topk computes on the rows units[] of W, without the gathered
 * copy of those rows and without a [B][n_units] tensor.  x [B][ldx], W [H][ldw] fp32, bias [H] fp32 or NULL (+0),
 * units [n_units] int32, all on the device; the host reads none of them.
 * Arithmetic (the encoder contract of qsae.h): for row r and list position p with u = units[p],
 *   v(r, p) = the fp32 fmaf chain over d ascending, the accumulator seeded with bias[u]
 * -- the bits qsae_encode_dense gives at [r][u].  Row r outputs its k largest by (value descending, unit ascending) in that
 * order: idx[r][j] (int32 [B][k]) = the unit id u, val[r][j] (fp32 [B][k]) = v.  The order is that of the library's 64-bit
 * keys (order-preserving bits of v, -0 as +0) << 32 | ~u: NaN ranks above +inf, -0.0 and +0.0 tie and go to the lower unit.
 * val is decoded from the key, so a selected -0.0 comes back as +0.0 and a selected NaN as the NaN 0x7FFFFFFF; every other
 * value keeps its bits.  Keys of a row are distinct, so the result does not depend on tiling, grid or candidate split.
 * units: ascending and distinct.  An entry outside [0, H) is never a candidate and causes no read out of range; when
 * fewer than k entries of the list are inside, the slots past them hold idx = -1, val = +0.
 * Limits: 1 <= k <= 64, k <= n_units, D a positive multiple of 4, H >= 1, otherwise QSAE_ERR_UNSUPPORTED before any
 * launch; any n_units >= 1 and any B.  ldx, ldw >= D and multiples of 4, x and W 16-byte aligned.  Floats of a row at or
 * past D are not read.  B == 0 or n_units == 0: QSAE_OK with nothing launched, no pointer is looked at.
 * QSAE_ERR_WORKSPACE when the workspace is missing or too small.
 * workspace: 16-byte aligned, qsaex_encode_topk_units_workspace_bytes(B, D, n_units, k) bytes (the list's unit ids and
 * biases padded to the tile, the keys, and the partial lists of a candidate split; 0 for a shape the call refuses or
 * launches nothing for; monotone in B, n_units and k).  The call leaves nothing in it that a later call reads and does
 * not need it zeroed. */
size_t qsaex_encode_topk_units_workspace_bytes(int B, int D, int n_units, int k);
int qsaex_encode_topk_units(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, int B, int D, int H,
                            const int32_t* units, int n_units, int k, int32_t* idx, float* val, void* workspace,
                            size_t workspace_bytes, qsae_stream_t stream);

/* The normalised auxiliary loss and its gradient.  x, recon, aux, grad: fp32 [B][D], contiguous, on the device; 4-byte
 * alignment is all they need (every access is one element).  With every fp32 step rounded separately:
 *   e[r][d] = fl32(x - recon)                      the residual the dead units are asked to explain; a constant of the loss
 *   m[d]    = (sum_r e[r][d]) / B                  in fp64; a constant of the loss as well
 *   Dn      = sum_{r,d} (e - m[d])^2               in fp64 (e widened exactly)
 *   q[r][d] = fl32(aux - e);  N = sum_{r,d} q^2    the square and the sum in fp64
 *   loss[0] (fp32, device) = fp32((coef * N) / Dn)
 *   grad[r][d] = fl32(s * q[r][d]),  s = fp32((2 * coef) / Dn)          -- d loss / d aux; nothing else has a gradient
 *   Dn == 0:  loss[0] = 0 and grad = 0 everywhere.
 * sums (fp64 [2], device) receives (N, Dn) unless NULL.  Nothing is read back to the host and no float atomic is used:
 * the same input gives the same bits on every run.  Order of the sums, a function of (B, D) alone:
 *   rows are taken in groups of 32 consecutive rows (the last group may be short), columns in blocks of 256;
 *   m:  thread d adds the rows of a group to 0.0 in ascending order; the group sums of a column are then added to 0.0 in
 *       ascending group order, and the total is divided by B;
 *   N, Dn:  workgroup (group g, column block c) -- number g * ceil(D / 256) + c -- has thread t add column 256 c + t of the
 *       rows of group g to 0.0 in ascending order (a thread past D keeps 0.0); the 64 lane sums of a wave are joined by a
 *       butterfly (xor 32, 16, ..., 1), the 4 wave sums added in ascending order; then thread t of ONE workgroup adds the
 *       workgroup sums t, t + 256, ... to 0.0 in ascending order and the 256 thread sums are joined the same way.
 * Three streaming passes over [B][D]: x and recon are read twice (m; then N, Dn and q, which is parked in grad), aux once,
 * grad is written twice and read once (the scaling by s).
 * B == 0: QSAE_OK without a launch, nothing written.  Errors: QSAE_ERR_INVALID_ARG (B < 0, D < 1, a null or misaligned
 * pointer), QSAE_ERR_UNSUPPORTED (ceil(B / 32) * ceil(D / 256) above 2^31 - 1), QSAE_ERR_WORKSPACE.
 * workspace: 8-byte aligned, qsaex_auxk_loss_workspace_bytes(B, D) bytes (the group sums of the columns, m, two partial
 * sums per workgroup and s; 0 for B < 1 or D < 1).  It need not be zeroed. */
size_t qsaex_auxk_loss_workspace_bytes(int B, int D);
int qsaex_auxk_loss(const float* x, const float* recon, const float* aux, int B, int D, double coef, float* loss,
                    float* grad, double* sums, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_EXT_H */
