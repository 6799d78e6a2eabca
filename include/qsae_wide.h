/*
 * qsae_wide.h -- per-row top-k over dictionaries wider than one selection kernel takes: the hidden range is cut into
 * contiguous slabs, every slab is selected by the existing forms of qsae.h on offset pointers, and the S lists of a row are
 * merged into the row's top-k on the device.  Entry points of libqsae_hip.so that are not yet part of qsae.h.
 *
 * Why slab lists suffice: a pre-activation is an fmaf chain over one unit's own weights, so its bits do not depend on which
 * other units are computed beside it; and an entry of a row's top-k is in the top-k of whichever slab holds it.  The top-k of
 * the union of the S slab lists is therefore the row's top-k, values and order included.
 *
 * Common to all entry points: arguments are checked before any launch, in the order each function states; no float atomics;
 * every output element is written by exactly one thread, so every run gives the same bits; element indices are 64-bit.
 *
 * qsaew_slab_plan(H, k, slab, starts)                                                                              (host only)
 *   S = ceil(H / slab) slabs; slab s covers the units starts[s] .. starts[s + 1] - 1, starts[0] = 0, starts[S] = H.  Starts
 *   are ascending multiples of 256.  Widths are balanced: walking s upwards, slab s takes the remaining units divided by the
 *   remaining slabs, rounded up to a multiple of 256, and the last slab the rest -- no width exceeds `slab`, and no two widths
 *   differ by 256 S or more (no short tail).  Returns S (>= 1), or a negative QSAE_ERR_* code with the error text set.
 *   starts: QSAEW_MAX_SLABS + 1 ints, or NULL to ask for S alone.
 *   Checks, in order: H <= QSAEW_MAX_H, k <= 256, H a multiple of 4, slab <= QSAEW_MAX_SLAB and a multiple of 256, S <=
 *   QSAEW_MAX_SLABS, every width >= k (all QSAE_ERR_UNSUPPORTED; a check whose operands are not positive is left to the next
 *   group); then H > 0, 1 <= k <= H, slab > 0 (QSAE_ERR_INVALID_ARG).
 *
 * qsaew_merge_topk(pidx, pval, S, B, k, starts, idx, val, dense, dense_ld, stream)
 *   pidx int32 / pval fp32 [S][B][k] (device): list (s, r) is the top-k of row r within slab s in the order of qsae_topk_rows --
 *   value descending by mono_key (NaN above +inf, -0 equal to +0), unit ascending among equal keys -- with unit ids relative to
 *   starts[s].  starts: S + 1 host ints as qsaew_slab_plan gives them (any ascending starts with widths >= k are taken).
 *   idx / val [B][k] (device): the k best of the row's S k entries in the same order, unit ids global (pidx + starts[s]),
 *   values with the bits they came with.  The rank of entry j of list s is j, plus for every slab t < s the entries of list
 *   (t, r) whose key is >= its own, plus for every slab t > s those whose key is > its own: the order of the one-piece kernels,
 *   where a tie goes to the lower unit.  One thread per entry; the counts are binary searches over the sorted lists.
 *   dense (nullable, device, row stride dense_ld >= starts[S]): the kernel stores +0.0f at dense[r][starts[s] + pidx] for each
 *   of the S k - k entries of a row that lost.  The winners' elements and every other element are not touched.
 *   Checks, in order: S <= QSAEW_MAX_SLABS, B * k < 2^31 (QSAE_ERR_UNSUPPORTED); S >= 1, B >= 0, k >= 1, starts non-null,
 *   starts[0] >= 0, every width >= k; B == 0 -> QSAE_OK; pidx, pval, idx, val non-null and 4-byte aligned; with dense:
 *   4-byte aligned and dense_ld >= starts[S].
 *
 * qsaew_encode_topk(x, W, bias, B, D, H, k, slab, idx, val, dense, dense_ld, workspace, workspace_bytes, stream)
 * qsaew_encode_topk_prefilter(x, W, bias, Wq, meta, B, D, H, k, slab, idx, val, dense, dense_ld, workspace, workspace_bytes,
 *                             spec_rows, flagged_rows, stream)
 *   The whole selection: for each slab of qsaew_slab_plan(H, k, slab) the existing implementation on W + h0 D, (Wq + h0 D,)
 *   bias + h0 and dense + h0 with dense_ld unchanged, into the slab's part lists in the workspace, then qsaew_merge_topk.
 *   Results are those of qsae_encode_topk_latent on the whole matrix wherever that runs, bit for bit, dense latent included.
 *   qsaew_encode_topk: every slab takes qsae_encode_topk_latent (dense given) or qsae_encode_topk, i.e. the fused form or the
 *   chunked one as its own shape selects.  qsaew_encode_topk_prefilter: a slab whose shape the prefilter takes
 *   (qsae_encode_topk_prefilter_workspace_bytes(B, D, width, k) > 0) goes through qsae_encode_topk_prefilter, any other
 *   through the exact forms above.  (Wq, meta) are those of qsae_prefilter_pack_w of the WHOLE matrix: meta holds maxima over
 *   all rows, which bound every row range.  *flagged_rows (nullable) = the sum of the slabs' flagged rows; each slab's count
 *   is read back by its own call (S host round trips at the most).  dense is nullable; the zeros of a slab's columns are
 *   written by the slab's call as today, the losers of the merge are erased by the merge; no [B, H] memset is added.
 *   Checks, in order: those of qsaew_slab_plan except its last group, D a multiple of 4 (QSAE_ERR_UNSUPPORTED); B >= 0, D > 0,
 *   H > 0, 1 <= k <= H, slab > 0; B == 0 -> QSAE_OK (*flagged_rows = 0); x, W, idx, val, workspace (Wq, meta) non-null; x, W,
 *   workspace (Wq) 16-byte aligned; with dense: 16-byte aligned, dense_ld >= H and a multiple of 4; workspace_bytes
 *   (QSAE_ERR_WORKSPACE).
 * qsaew_encode_topk_workspace_bytes / qsaew_encode_topk_prefilter_workspace_bytes(B, D, H, k, slab): the bytes the call needs
 *   (the part lists plus the largest slab's own workspace); 0 where the call would refuse the shape or B <= 0.
 *
 * A further extension header in the spirit of qsae_ext.h: qsae.h, the binding table _lib.SIGNATURES and their ledgers are
 * pinned to each other and are opened together.  The functions below are exported as qsaew_* from the same library
 * (csrc/wide.hip), share its error text (qsae_last_error()), its conventions (qsae.h, "Conventions") and its return codes, are
 * bound from _lib.WIDE_SIGNATURES, and have a ledger of their own in tests/test_wide_host.py.  They join qsae.h as qsae_* when
 * the ledger is next opened; QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_WIDE_H
#define QSAE_WIDE_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEW_MAX_SLABS 32
#define QSAEW_MAX_H (1 << 20)
#define QSAEW_MAX_SLAB 32768
#define QSAEW_DEFAULT_SLAB 32768

int qsaew_slab_plan(int H, int k, int slab, int* starts);

int qsaew_merge_topk(const int32_t* pidx, const float* pval, int S, int B, int k, const int* starts, int32_t* idx, float* val,
                     float* dense, int64_t dense_ld, qsae_stream_t stream);

size_t qsaew_encode_topk_workspace_bytes(int B, int D, int H, int k, int slab);

int qsaew_encode_topk(const float* x, const float* W, const float* bias, int B, int D, int H, int k, int slab, int32_t* idx,
                      float* val, float* dense, int64_t dense_ld, void* workspace, size_t workspace_bytes,
                      qsae_stream_t stream);

size_t qsaew_encode_topk_prefilter_workspace_bytes(int B, int D, int H, int k, int slab);

int qsaew_encode_topk_prefilter(const float* x, const float* W, const float* bias, const void* Wq, const float* meta, int B,
                                int D, int H, int k, int slab, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                                void* workspace, size_t workspace_bytes, int spec_rows, int* flagged_rows,
                                qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_WIDE_H */
