/*
 * qsae_recycle.h -- the forward-in-one-call prefilter entry points of qsae.h on a RECYCLED dense latent.  Entry points of
 * libqsae_hip.so that are not yet part of qsae.h.
 *
 * The contract.  Each function below is its qsae_* namesake with two more arguments at the end, stale_idx and stale_k.
 * stale_idx points to device memory, int32 [B][stale_k], and is a promise about the buffer passed as `dense`:
 *   `dense` is +0.0 in all B x H positions except possibly at dense[r][stale_idx[r][j]]  (0 <= r < B, 0 <= j < stale_k).
 * That is what a dense latent written by this library looks like once its caller has dropped it: zeros, and per row the k
 * entries listed in that call's idx -- also for rows with NaN or infinite inputs and rows that took the exact fallback,
 * which write nothing but their k listed entries into the zeros.  Given the promise, the call does not write B x H zeros
 * again (8.6 GB at 65536 x 32768): it stores +0.0 at the at most B * stale_k listed positions, ordered on `stream` behind
 * everything queued before the call and ahead of the call's first write to `dense`, and otherwise runs as its namesake
 * does.  idx, val, dense and recon are bit-identical to the namesake's.  A
 * promise that does not hold gives a dense latent with whatever the unlisted positions held; idx, val and recon are right
 * even then.
 * An entry of stale_idx below 0 or at or past H is skipped and causes no access; stale_idx is read before anything of this
 * call is written, so it may be the idx buffer of the call that wrote `dense` -- but not this call's own idx.  The columns of
 * a row at or past H (dense_ld > H) are not touched.
 * The list is used by the plans that write the zeros of `dense` during the candidate pass (D in {128, 256, 512}, H a
 * multiple of 256, see qsae.h at qsae_encode_topk_prefilter); every other plan writes all of `dense` itself, and there --
 * and with stale_idx == NULL or dense == NULL -- the call is exactly its namesake.  With D = 512 the erase runs where the
 * namesake's fill kernel does: beside the candidate pass on the calling thread's side stream, forked from and joined back
 * into `stream` inside the call.
 * Limits and errors: those of the namesake, checked first and in the same order; then, with stale_idx != NULL,
 * 1 <= stale_k <= 1024 and stale_idx 4-byte aligned, otherwise QSAE_ERR_INVALID_ARG before any launch.  B == 0: QSAE_OK,
 * nothing launched, no pointer looked at.
 * The two submit forms are finished by qsae_prefilter_finish / qsae_prefilter_finish_table of qsae.h, with the arguments
 * they share: a finish never looks at the list.
 *
 * A further extension header in the spirit of qsae_ext.h: qsae.h, the binding table _lib.SIGNATURES and their ledgers are
 * pinned to each other and are opened together.  The functions below are exported as qsaer_* from the same library
 * (csrc/prefilter_topk.hip; the erase kernel is in csrc/misc.hip), share its error text (qsae_last_error()), its conventions
 * (qsae.h, "Conventions") and its return codes, are bound from _lib.RECYCLE_SIGNATURES, and have a ledger of their own in
 * tests/test_latent_recycle_host.py (every function declared here is bound and exported by the product and the debug
 * library; tests/test_latent_recycle_gpu.py drives them).  They join qsae.h as qsae_* when the ledger is next opened;
 * QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_RECYCLE_H
#define QSAE_RECYCLE_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAER_MAX_STALE_K 1024

/* qsae_binary_forward_prefilter on a recycled latent. */
int qsaer_binary_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                   const float* meta, int B, int D, int H, int k, const uint8_t* packed, int n_bits,
                                   float step, const float* dec_bias, int32_t* idx, float* val, float* dense,
                                   int64_t dense_ld, float* recon, void* workspace, size_t workspace_bytes,
                                   int spec_rows, int* flagged_rows, qsae_stream_t stream, const int32_t* stale_idx,
                                   int stale_k);

/* qsae_table_forward_prefilter on a recycled latent. */
int qsaer_table_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                  int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                  int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon, void* workspace,
                                  size_t workspace_bytes, int spec_rows, int* flagged_rows, qsae_stream_t stream,
                                  const int32_t* stale_idx, int stale_k);

/* qsae_prefilter_submit on a recycled latent; finished by qsae_prefilter_finish. */
int qsaer_prefilter_submit(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                           int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step,
                           const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                           float* recon, void* workspace, size_t workspace_bytes, int* flagged_host,
                           qsae_stream_t stream, const int32_t* stale_idx, int stale_k);

/* qsae_prefilter_submit_table on a recycled latent; finished by qsae_prefilter_finish_table. */
int qsaer_prefilter_submit_table(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                 int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                 int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon, void* workspace,
                                 size_t workspace_bytes, int* flagged_host, qsae_stream_t stream,
                                 const int32_t* stale_idx, int stale_k);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_RECYCLE_H */
