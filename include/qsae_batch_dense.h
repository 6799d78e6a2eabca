/*
 * qsae_batch_dense.h -- the dense BatchTopK encoder of the top-k SAEs: the encoder's exact-fp32 contraction with a scalar
 * floor in its epilogue, the batch-wide selection of qsae_batch.h over the candidates above the floor, and a device-side
 * certificate that repeats the chain without a floor when the floor was too high.  Entry points of libqsae_hip.so that are not
 * yet part of qsae.h.
 *
 * A further extension header in the spirit of qsae_jump_dense.h: qsae.h, the binding table _lib.SIGNATURES and their ledgers
 * are pinned to each other and are opened together.  The functions below are exported as qsaebd_* from the same library
 * (csrc/batch_dense.hip), share its error text (qsae_last_error()), its conventions (qsae.h, "Conventions") and its return
 * codes, are bound from _lib.BATCH_DENSE_SIGNATURES, and have a ledger of their own in tests/test_batch_dense_host.py (every
 * function declared here is bound, exported by the product and the debug library, and is either a *_bytes sizer or guarded in
 * tests/test_batch_dense_gpu.py).  They join qsae.h as qsae_* when the ledger is next opened; QSAE_ABI_VERSION does not move
 * until then.
 */
#ifndef QSAE_BATCH_DENSE_H
#define QSAE_BATCH_DENSE_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEBD_MAX_K 256        /* widest list per row (the cap) */
#define QSAEBD_REPORT_WORDS 8

/* -- qsaebd_encode_batch_topk --------------------------------------------------------------------------------------------------
 * x fp32 [B][ldx], W fp32 [H][ldw] (the encoder's weight, one row per unit), bias fp32 [H] or NULL, all on the device.
 *
 * Pre-activation.  z[r][h] is the encoder pre-activation of DESIGN.md section 2: the fp32 fmaf chain over k = 0 .. D - 1 in
 * ascending order, seeded with bias[h] (+0 without a bias) -- the bits qsae_encode_dense writes and oracle.encode computes.
 *
 * The capped reference list.  L(r) is row r's top-K list in the library's rank order (value descending with -0 and +0 as one
 * value, then unit ascending): what qsae_encode_topk* writes at width K.
 *
 * The outputs are what qsaeb_batch_select(val = L, n_select) returns on those lists (qsae_batch.h, "Batch selection"):
 *   counts   int32 [B]: identical.
 *   val_sel  fp32 [B][K]: the selected values (the bits of z), +0 behind the prefix.
 *   idx_sel  int32 [B][K]: idx_sel[r][j] == L(r).idx[j] for j < counts[r], -1 behind it (the convention of qsaed_encode_jump;
 *            the ragged consumers of qsae_batch.h read by counts).
 *   report   int64 [8] or NULL: [0..3] as qsaeb_batch_select, the same bits: {selected, rows with counts == K (saturated), rows
 *            with counts == 0 (empty), the bits of the smallest selected value m}.  [4] the candidates of attempt one, a row
 *            counting at most K; [5] 1 if the second attempt ran; [6] the rows of attempt one with more than K pre-activations
 *            above the floor; [7] the bits of the floor that was used.
 *   theta fp32 [1], batches int64 [1] (both or neither), lr: the threshold state of qsaeb_batch_select, under the same rule.
 * Ties at the boundary key go to the lowest (row, list position), as there.  As there, this equals BatchTopK over all [B][H]
 * pre-activations whenever report[1] == 0.
 *
 * The floor.  It is read from floor_dev (device, fp32 [1]) when that is non-NULL, otherwise it is floor_host.  The candidates
 * of row r are the entries of L(r) with z > floor (a float compare): the list is rank ordered, so they are a prefix of it.
 * Call their union over the rows C.  If |C| >= n_select (the CERTIFICATE, an integer the chain counts), the n_select first
 * entries in key order of all lists are the n_select first of C, because every entry left out is <= floor and so behind every
 * candidate.  Otherwise the chain runs again and admits every pre-activation that is not a NaN: then C = L.  Both attempts are
 * launched every time; the workgroups of the second read the certificate word and leave at once when it holds.  Nothing is read
 * back, and which path ran is a function of the operands alone.  The result is the same bits for EVERY floor; the floor changes
 * the time only.  A NaN floor admits no candidate, so the second attempt runs (unless n_select == 0, which any floor
 * certifies); so does a floor of +inf.
 *
 * With floor_dev, the chain ends by writing floor_dev[0] = fl32(floor_ratio * m) when something was selected and m > 0 (the
 * condition of the threshold state), so the next step's floor comes from this step without a host read; otherwise it is left
 * as it was.  floor_ratio is not looked at beyond its range check when floor_dev is NULL.
 *
 * NaN pre-activations.  A NaN z is never a candidate, in either attempt, while the capped path ranks NaN first: equality with
 * the capped path is claimed for batches without NaN pre-activations only.  With NaN present the call stays inside its
 * buffers and gives the same bits on every run: L(r) is then the top-K list of the row's non-NaN pre-activations (shorter
 * than K when fewer than K are left), and when the second attempt holds fewer than n_select candidates all of them are
 * selected.
 *
 * The chain.  The contraction on the fp32 matrix cores (128 x 128 tiles, the rows of W split over at most 8 workgroups per
 * panel of 128 rows of x) appends every unit above the floor to a region of the workspace that belongs to one (split, row);
 * one wave per row joins the regions and ranks them; a row one of whose regions overflowed, or with more than 512 such units,
 * is recomputed from the fmaf chain itself (the same bits) and its list is taken by a radix search over the 64-bit rank keys.
 * The selection is that of qsaeb_batch_select (three radix passes over mono_key, per-row tie counts, an exclusive prefix over
 * the rows) with every row read up to its candidate count.  Integer atomics hand out places and add integers; no output
 * depends on their arrival order.  No float atomics: the same bits on every run, whatever the grid.
 *
 * Limits, checked before any launch and before any pointer is looked at, in this order: B >= 0, K >= 1, H >= 1, floor_ratio
 * finite and in (0, 1] (QSAE_ERR_INVALID_ARG); K <= 256, K <= H, D a positive multiple of 4, B * K < 2^31, H <= 2^30
 * (QSAE_ERR_UNSUPPORTED); 0 <= n_select <= B * K (QSAE_ERR_INVALID_ARG).  B == 0: QSAE_OK with nothing launched.  Then ldx and
 * ldw (>= D and multiples of 4), null or misaligned pointers (x and W 16-byte aligned; the others 4-byte, report and batches
 * 8; theta and batches both or neither; QSAE_ERR_INVALID_ARG), then the workspace (QSAE_ERR_WORKSPACE when missing or smaller
 * than the sizer says; 256-byte aligned; it need not be zeroed).  The sizer returns 0 for shapes the call refuses.  The
 * outputs must not overlap the operands. */
size_t qsaebd_encode_batch_topk_workspace_bytes(int B, int D, int H, int K);
int qsaebd_encode_batch_topk(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, int B, int D, int H,
                             int K, int64_t n_select, float* floor_dev, float floor_host, float floor_ratio, int32_t* idx_sel,
                             float* val_sel, int32_t* counts, int64_t* report, float* theta, int64_t* batches, float lr,
                             void* workspace, size_t workspace_bytes, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_BATCH_DENSE_H */
