/*
 * qsae_optim.h -- what the top-k SAE papers put around the Adam step, in the passes that already touch the data: the joint
 * gradient norm and its clip coefficient as one device word, the Adam step that multiplies the gradient by that word and
 * carries an exponential moving average of the weights as one more stream, and the projection that removes from the decoder
 * gradient its component parallel to each atom.  Entry points of libqsae_hip.so that are not yet part of qsae.h.
 *
 * Common to all entry points: arguments are checked before any launch, in the order each function states; a size of zero
 * returns QSAE_OK with nothing launched; no float atomics -- every sum runs in a fixed order that depends on the sizes only,
 * never on the grid, so every run gives the same bits; element indices are 64-bit.  Every operation named below is one IEEE
 * operation of the stated width (the build passes -ffp-contract=off; divisions and square roots are the correctly rounded
 * ones, subnormals are kept).  NaN and inf go where the operations take them.
 *
 * qsaeo_project_columns(W, G, D, H, ld, stream)
 *   W: decoder.weight, fp32 [D][ld], read only.  G: its gradient, same layout, updated in place.  For every column h < H
 *       dot_h = sum_d G[d][h] * W[d][h]        and then        G[d][h] = fmaf(-dot_h, W[d][h], G[d][h])   for every d.
 *   Order of dot_h: QSAEO_PROJECT_GROUPS = 16 chains per column.  Chain r starts from +0.0f and takes the rows
 *   d = r, r + 16, r + 32, ... in ascending order, one c = fmaf(G[d][h], W[d][h], c) each (a chain without rows stays +0.0f).
 *   dot_h = (((c_0 + c_1) + c_2) + ... + c_15), fp32 additions in ascending r.
 *   A column whose dot_h compares equal to zero is not rewritten: its bits stay, signed zeros included.  A NaN or inf in
 *   column h stays in column h; its neighbours keep their bits.  Columns at or past H, up to ld, are neither read nor written.
 *   Checks, in order: D >= 0 and H >= 0; D == 0 or H == 0 -> QSAE_OK; H a multiple of 4 (QSAE_ERR_UNSUPPORTED, the limit of
 *   qsae_normalize_columns_table); ld >= H and ld a multiple of 4; W and G non-null; W and G 16-byte aligned; W != G.
 *
 * qsaeo_grad_norm(ptrs, counts, T, max_norm, coef, report, workspace, workspace_bytes, stream)
 *   The joint L2 norm of T fp32 tensors (host arrays of device pointers and element counts, the form of
 *   qsae_tensor_stats; tensors 4-byte aligned -- one that starts off a 16-byte boundary is read element by element, the
 *   same elements in the same order, hence the same bits).  Order of the fp64 sums: a tensor is cut into chunks of 8192
 *   elements, a chunk into 8 slabs of 1024; thread j of 256 takes the elements 4 j .. 4 j + 3 of every slab and adds
 *   double(x) * double(x) (one fp64 multiplication, one addition) in ascending (slab, element) order from 0.0; the 64 lane
 *   sums of a wave are joined by a butterfly (xor 32, 16, ..., 1), the 4 wave sums added in ascending order: a chunk's
 *   partial.  Per tensor, thread j adds the chunk partials j, j + 256, ... in ascending order from 0.0 and the 256 threads
 *   are joined the same way; the tensors' sums are added in ascending order from 0.0.
 *   report (device, 8-byte words, 4 + T of them): word 0 the total sum of squares (fp64), word 1 norm = sqrt(total), word 2
 *   the coefficient as fp64 (the fp32 value widened), word 3 int64: 0 where the coefficient is exactly 1, else 1, words
 *   4 .. 4 + T - 1 the tensors' sums of squares.
 *   *coef (device fp32): torch.nn.utils.clip_grad_norm_'s formula in fp64, c = max_norm / (norm + 1e-6); c >= 1 gives 1.0f,
 *   a NaN c gives NaN, otherwise c rounded to fp32 once.  An infinite gradient therefore gives 0, a NaN gradient NaN.
 *   Nothing is read back.
 *   Checks, in order: T >= 0; T <= 65536 (QSAE_ERR_UNSUPPORTED); T == 0 -> QSAE_OK; ptrs and counts non-null; per tensor
 *   count >= 0, a non-null pointer where the count is not zero, 4-byte alignment; at most 2^40 elements per tensor and 2^30
 *   chunks per call (QSAE_ERR_UNSUPPORTED); max_norm >= 0 (a NaN is refused); coef non-null and 4-byte aligned, report
 *   non-null and 8-byte aligned; workspace non-null, 8-byte aligned and at least qsaeo_grad_norm_workspace_bytes(counts, T)
 *   (QSAE_ERR_WORKSPACE).  Tensors without elements are fine (sum 0); with T > 0 the report is always written.
 * qsaeo_grad_norm_workspace_bytes(counts, T): the bytes qsaeo_grad_norm needs; 0 where it would refuse T or counts.
 *
 * qsaeo_adam_step(p, g, m, v, n, one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, step_size, coef, ema, one_minus_decay, stream)
 *   qsae_adam_step with two optional streams.  coef: a nullable device fp32 word; when non-null the gradient enters the
 *   element's step as g * (*coef), one fp32 multiplication (1.0f leaves every finite g as it is); g is not written.
 *   ema: nullable, fp32 [n]; after the element's step  t = p' - e;  te = t * one_minus_decay;  e' = e + te.
 *   With both null the result is qsae_adam_step's bit for bit.  Load widths (16 bytes where p, g, m, v -- and ema when
 *   given -- are all 16-byte aligned, 4 otherwise), the tail rule and the grid cap are qsae_adam_step's.
 *   Checks, in order: n >= 0; n == 0 -> QSAE_OK; p, g, m, v non-null; coef 4-byte aligned.
 *
 * qsaeo_adam_step_prefilter(W, gW, mW, vW, bias, gb, mb, vb, H, D, <six scalars>, coef, emaW, emab, one_minus_decay, Wq,
 *                           meta, stream)
 *   qsae_adam_step_prefilter with the same two streams for the encoder pair; (Wq, meta) are bit-identical to
 *   qsae_prefilter_pack_w of the new W and bias.  Lane assignment, chain order and tree are qsae_adam_step_prefilter's.
 *   Checks, in order: those of qsae_adam_step_prefilter; coef 4-byte aligned; emab non-null exactly where emaW and bias
 *   both are (emaW null: emab null).
 *
 * A further extension header in the spirit of qsae_ext.h: qsae.h, the binding table _lib.SIGNATURES and their ledgers are
 * pinned to each other and are opened together.  The functions below are exported as qsaeo_* from the same library
 * (csrc/optim_recipe.hip), share its error text (qsae_last_error()), its conventions (qsae.h, "Conventions") and its return
 * codes, are bound from _lib.OPTIM_SIGNATURES, and have a ledger of their own in tests/test_optim_recipe_host.py.  They
 * join qsae.h as qsae_* when the ledger is next opened; QSAE_ABI_VERSION does not move until then.
 */
#ifndef QSAE_OPTIM_H
#define QSAE_OPTIM_H

#include "qsae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSAEO_PROJECT_GROUPS 16
#define QSAEO_NORM_HEAD 4

int qsaeo_project_columns(const float* W, float* G, int D, int H, int64_t ld, qsae_stream_t stream);

size_t qsaeo_grad_norm_workspace_bytes(const int64_t* counts, int T);

int qsaeo_grad_norm(const void* const* ptrs, const int64_t* counts, int T, double max_norm, float* coef, void* report,
                    void* workspace, size_t workspace_bytes, qsae_stream_t stream);

int qsaeo_adam_step(float* p, const float* g, float* m, float* v, long long n, float one_minus_b1, float b2,
                    float one_minus_b2, float bc2_sqrt, float eps, float step_size, const float* coef, float* ema,
                    float one_minus_decay, qsae_stream_t stream);

int qsaeo_adam_step_prefilter(float* W, const float* gW, float* mW, float* vW, float* bias, const float* gb, float* mb,
                              float* vb, int H, int D, float one_minus_b1, float b2, float one_minus_b2, float bc2_sqrt,
                              float eps, float step_size, const float* coef, float* emaW, float* emab,
                              float one_minus_decay, void* Wq, float* meta, qsae_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QSAE_OPTIM_H */
