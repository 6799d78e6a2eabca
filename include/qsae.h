/*
 * qsae.h -- C ABI of the MI355X (gfx950) quantized-SAE forward backend.
 *
 * Drop-in boundary for the forward hot path of ASSERT-KTH/QuantizedSAE.  The reference
 * is pure Python/PyTorch and has no FFI of its own; each entry
 * point below replaces the ATen call sequence cited next to it (paths relative to the
 * reference root).  Everything here is stateless: plain device pointers and sizes, no
 * torch types, work is enqueued on the given HIP stream and the call returns without
 * synchronising (exceptions are marked "one host round trip").  No call leaves anything
 * behind that a later call reads: what the library keeps is per device ("this kernel's LDS limit
 * is raised on device d") or owned by one host thread for one device (a side stream, three
 * events, one pinned word -- created on first use).  Calls may therefore be made from several
 * host threads and on several devices of one process; the caller makes the device of its
 * pointers current, as for any HIP library, and gives every concurrently running call its own
 * workspace.  (Several host threads: tested on hardware.  Several devices in ONE process: by
 * construction only -- no box with two visible devices has run it yet; one process per GPU is the
 * tested deployment.)  The Python host side in quantizedsae_amd/ binds these with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - all tensors row-major, contiguous, device memory unless stated;
 *   - B rows of activations, D = input_dim, H = hidden_dim, k = top-k;
 *   - return value: QSAE_OK or a negative QSAE_ERR_* code; qsae_last_error() gives text;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - B == 0 is a valid no-op everywhere.
 *
 * Numerical contract (bit-exact against oracle/qsae_oracle.c):
 *   encoder latent = fp32 fmaf chain over k ascending seeded with bias (what
 *   v_mfma_f32_32x32x2_f32 computes when K is walked in order); top-k = k largest by
 *   (value desc, index asc), NaN above +inf; sparse decode = ascending-index fmaf chain,
 *   then separately rounded *step and +bias.
 */
#ifndef QSAE_H
#define QSAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSAE_ABI_VERSION 4

#define QSAE_OK 0
#define QSAE_ERR_INVALID_ARG (-1)  /* null pointer, non-positive dim, misaligned pointer      */
#define QSAE_ERR_UNSUPPORTED (-2)  /* shape outside what the kernels implement                 */
#define QSAE_ERR_HIP (-3)          /* a HIP runtime call failed (text in qsae_last_error())    */
#define QSAE_ERR_WORKSPACE (-4)    /* workspace too small; see the *_workspace_bytes() helpers */

/* activation applied by qsae_encode_dense */
#define QSAE_ACT_NONE 0    /* BinarySAE / Baseline: sae/binary.py:82-84, sae/baseline.py:8-10 */
#define QSAE_ACT_RELU 1    /* Ternary: sae/ternary.py:95-98                                    */
#define QSAE_ACT_SIGMOID 2 /* Matryoshka: sae/quantized_matryoshka.py:206-209                  */

typedef void* qsae_stream_t;

/* -- library ---------------------------------------------------------------------------- */
int qsae_abi_version(void);
/* Thread-local text of the last failing call ("" if none). */
const char* qsae_last_error(void);
/* Properties of the current device: compute units, name of the gfx target (e.g. "gfx950"). */
int qsae_device_info(int* cu_count, char* arch, int arch_len);

/* -- profiling ---------------------------------------------------------------------------- */
/* One-shot, per host thread: the NEXT fused / prefilter / bits-prefilter call of the calling thread records
 * ev_begin (hipEvent_t) on its stream right before its candidate-sweep launch and ev_end right after it (after the
 * co-resident fill kernel has joined, where there is one), then forgets them.  NULL, NULL clears a pending pair.
 * This is how bench.py times the dominant kernel live on the launch stream. */
int qsae_profile_sweep_events(void* ev_begin, void* ev_end);
/* The events for the call above, created / read / destroyed through the HIP runtime this library is linked against
 * (timing enabled).  elapsed: QSAE_ERR_HIP while either event has not completed. */
int qsae_profile_event_create(void** ev);
int qsae_profile_event_destroy(void* ev);
int qsae_profile_event_elapsed_ms(void* ev_begin, void* ev_end, float* ms);
/* Fraction of the encoder's 2 B D H FLOPs that the profiled launch covers for hidden width H (1.0 when the sweep
 * derives its thresholds itself, else (H - pilot block) / H). */
double qsae_profile_sweep_flop_fraction(int H);

/* -- encoder ---------------------------------------------------------------------------- */
/* K-interleaved operand layout.  dst[r][8g + j/2 + 4*(j&1)] = src[r][8g + j]: every 8 consecutive
 * k of a row stored as [k0 k2 k4 k6 k1 k3 k5 k7] -- the order the fp32 MFMA consumes them from LDS,
 * so that staged 16-byte chunks need no register shuffle.  Purely a storage permutation: the
 * contraction still runs in ascending k and gives bit-identical results.  W_enc is permuted once
 * per checkpoint, x once per batch (a 2 x B x D x 4-byte copy).  K % 8 == 0. */
int qsae_kperm_rows(const float* src, int rows, int K, float* dst, qsae_stream_t stream);

/* out[b][h] = act(bias[h] + sum_k x[b][k] * W[h][k])           (fp32 MFMA, exact fmaf chain)
 * Replaces nn.Linear (+ReLU / +Sigmoid) in SparseAutoencoder.encode, sae/base.py:16-19.
 * x [B][D], W [H][D], bias [H] or NULL, out [B][out_ld] with out_ld >= H.
 * Requires D % 4 == 0 and 16-byte aligned x, W. */
int qsae_encode_dense(const float* x, const float* W, const float* bias, int B, int D, int H,
                      int act, float* out, int64_t out_ld, qsae_stream_t stream);
/* Same with x and W already K-interleaved (qsae_kperm_rows); D % 32 == 0. */
int qsae_encode_dense_kperm(const float* xp, const float* Wp, const float* bias, int B, int D, int H,
                            int act, float* out, int64_t out_ld, qsae_stream_t stream);

/* The same contraction at fp32 ACCURACY, not fp32 bit-exactness, on the fp16 matrix pipe (opt-in; nothing that ranks or
 * thresholds latents uses it): both operands are split into two fp16 terms under power-of-two scales (x per row, W global),
 * the three partial contractions x1.w1 + x1.w2 + x2.w1 (every product exact in fp32) run as one fp16 GEMM over a concatenated
 * K of 3 D with fp32 accumulation.  The result differs from qsae_encode_dense by accumulation-order noise (~1e-6 of a latent's
 * standard deviation -- the size of the reference's own sgemm-vs-chain difference).  Rows or weights that are not finite give
 * NaN outputs for the whole row / everything.  D % 64 == 0.
 *   qsae_emu_pack_w: once per checkpoint, W [H][D] -> Wc (qsae_emu_w_bytes() = 6 H D bytes, opaque), meta2 = 2 device floats;
 *   qsae_encode_dense_emu: workspace from qsae_encode_dense_emu_workspace_bytes(B, D) (the split copy of the batch). */
size_t qsae_emu_w_bytes(int H, int D);
int qsae_emu_pack_w(const float* W, int H, int D, void* Wc, float* meta2, qsae_stream_t stream);
size_t qsae_encode_dense_emu_workspace_bytes(int B, int D);
int qsae_encode_dense_emu(const float* x, const void* Wc, const float* meta2, const float* bias, int B, int D, int H, int act,
                          float* out, int64_t out_ld, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* zbits[b][w] bit j = (sigmoid(pre[b][32w+j]) > 0.5) == (pre >= 0x33C00001), pre as above.
 * Replaces encoder(x) followed by `latent > 0.5`, sae/quantized_matryoshka.py:97-99,206-209
 * (also scripts/analysis/dynamic_analysis.py:51).  zbits [B][words_ld] uint32, words_ld >=
 * ceil(H/32); bits beyond H are zero. */
int qsae_encode_bits(const float* x, const float* W, const float* bias, int B, int D, int H,
                     uint32_t* zbits, int64_t words_ld, qsae_stream_t stream);

/* Per-row top-k of a dense latent [B][ld]: idx/val [B][k] ordered by (value desc, index asc).
 * If zero_rest != 0 every non-selected entry of `latent` is overwritten with +0 in place, which
 * yields `latent * mask` of sae/binary.py:94-99 and the scatter of sae/baseline.py:34-40.
 * Replaces torch.topk + zeros_like + scatter_.  1 <= k <= min(H, 256), H <= 32768. */
int qsae_topk_rows(float* latent, int64_t ld, int B, int H, int k, int32_t* idx, float* val,
                   int zero_rest, qsae_stream_t stream);

/* Fused encoder + top-k without materialising the dense latent: same results as
 * qsae_encode_dense(act=NONE) followed by qsae_topk_rows.  Workspace from
 * qsae_encode_topk_workspace_bytes(), which is 0 exactly for the shapes refused with QSAE_ERR_UNSUPPORTED before any
 * launch: D % 4 == 0, H % 4 == 0, k <= 256 and H <= 32768 -- or H <= 65536 for B >= 2048, H >= 8192 (fused form). */
size_t qsae_encode_topk_workspace_bytes(int B, int D, int H, int k);
int qsae_encode_topk(const float* x, const float* W, const float* bias, int B, int D, int H, int k,
                     int32_t* idx, float* val, void* workspace, size_t workspace_bytes,
                     qsae_stream_t stream);
/* Same with x and W already K-interleaved (qsae_kperm_rows); D % 32 == 0. */
int qsae_encode_topk_kperm(const float* xp, const float* Wp, const float* bias, int B, int D, int H, int k,
                           int32_t* idx, float* val, void* workspace, size_t workspace_bytes,
                           qsae_stream_t stream);

/* qsae_encode_topk plus the reference's dense return value: dense[b][h] = latent if h is one of row
 * b's top-k else +0 (`latent * mask`, sae/binary.py:96-99; `zeros_like + scatter_`,
 * sae/baseline.py:38-40).  In the fused form the sweep zero-fills the dense tensor tile by tile
 * underneath its own MFMAs and the k survivors are scattered in at the end -- no separate memset
 * pass, no dense latent read back.  kperm != 0: x and W are K-interleaved.  Same workspace. */
int qsae_encode_topk_latent(const float* x, const float* W, const float* bias, int B, int D, int H, int k,
                            int32_t* idx, float* val, float* dense, int64_t dense_ld, int kperm,
                            void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* Order-preserving fp16 prefilter for the same operation.  A fp16 MFMA pass (per-row power-of-two
 * scaling, fp32 accumulation) with a rigorous per-row error bound eps_b only decides which hidden units
 * CAN belong to a row's top-k (everything with approximate value >= approximate k-th - 2 eps_b, ~90 of
 * 32768); those survivors are re-evaluated with the exact fp32 fmaf chain and ranked exactly, so idx,
 * val and dense are bit-identical to qsae_encode_topk_latent.  Rows the bound cannot serve (non-finite
 * inputs, overflowing lists) go through the exact kernels.  Wq/meta come from qsae_prefilter_pack_w
 * (once per checkpoint: Wq = H*D fp16, meta = 4 device floats -- weight scale, largest row norm, largest |bias|, largest
 * distance between a row and its fp16 copy; opaque to the caller).  D % 64 == 0, D <= 2048; other shapes
 * return QSAE_ERR_UNSUPPORTED (use qsae_encode_topk_latent).  dense may be NULL.  For D in {128, 256, 512} the
 * candidate pass is one launch (activation rows stationary in registers, fp16 weights streamed once per workgroup)
 * that also derives the row thresholds and writes the zeros of `dense`; the survivors are written by the refinement.
 * With D = 512 and a dense output the zeros are written by a second kernel that runs beside the candidate pass on a
 * side stream owned by the calling thread (one per device), forked from and joined back into `stream` inside the call
 * (the call stays ordered on `stream`).
 * One host round trip per call: the number of rows sent through the exact kernels (normally 0-5 of 65536), which also
 * comes back in *flagged_rows (host int, may be NULL).  spec_rows > 0 lets the device recompute the first spec_rows
 * flagged rows while the host waits for that count (worth it only when the previous batch had flagged rows; <= 1024).
 * qsae_prefilter_submit / _finish below are the same call without the round trip inside. */
size_t qsae_prefilter_w_bytes(int H, int D);
int qsae_prefilter_pack_w(const float* W, const float* bias, int H, int D, void* Wq, float* meta,
                          qsae_stream_t stream);
size_t qsae_encode_topk_prefilter_workspace_bytes(int B, int D, int H, int k);
int qsae_encode_topk_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                               const float* meta, int B, int D, int H, int k, int32_t* idx, float* val,
                               float* dense, int64_t dense_ld, void* workspace, size_t workspace_bytes,
                               int spec_rows, int* flagged_rows, qsae_stream_t stream);

/* BinarySAE.forward in one call (sae/binary.py:91-103 with binary_decoder.forward, :24-47, on the k kept entries):
 * qsae_encode_topk_prefilter followed by qsae_decode_binary_sparse, with the decode of a row done by the refinement
 * kernel as soon as it has ranked the row (its dictionary gathers and integer converts fill issue slots that the
 * refinement's own gathers leave idle; rows that take the exact fallback are decoded afterwards).  Outputs are
 * bit-identical to the two separate calls.  packed from qsae_pack_binary; same workspace and shape limits as
 * qsae_encode_topk_prefilter; dense may be NULL (compact outputs only). */
int qsae_binary_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq,
                                  const float* meta, int B, int D, int H, int k, const uint8_t* packed, int n_bits,
                                  float step, const float* dec_bias, int32_t* idx, float* val, float* dense,
                                  int64_t dense_ld, float* recon, void* workspace, size_t workspace_bytes,
                                  int spec_rows, int* flagged_rows, qsae_stream_t stream);

/* The same pipeline in two calls, so that the host never waits inside the library and can queue the next batch behind
 * this one (the blocking forms above are submit + wait + finish):
 *   submit : everything up to the refinement; every row that did not need the exact fallback is final afterwards.  The
 *            number of rows that do need it is copied asynchronously, in stream order, into *flagged_host (a host int,
 *            page-locked if the copy is to be asynchronous); the caller learns when it has landed from an event it
 *            records behind the call (or any later synchronisation of `stream`).
 *   finish : given that number, enqueues the exact fallback for those rows (their idx / val / dense entries and, with a
 *            dictionary, their reconstruction) and, on the paths whose sweep does not write the zeros, the dense latent.
 *            Outputs may be consumed once finish has been enqueued.  Same arguments as submit; workspace untouched in
 *            between (a second batch in flight needs a second workspace).
 * packed == NULL: no reconstruction (qsae_encode_topk_prefilter), n_bits / step / dec_bias / recon ignored. */
int qsae_prefilter_submit(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                          int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step,
                          const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                          float* recon, void* workspace, size_t workspace_bytes, int* flagged_host,
                          qsae_stream_t stream);
int qsae_prefilter_finish(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                          int B, int D, int H, int k, const uint8_t* packed, int n_bits, float step,
                          const float* dec_bias, int32_t* idx, float* val, float* dense, int64_t dense_ld,
                          float* recon, void* workspace, size_t workspace_bytes, int flagged,
                          qsae_stream_t stream);

/* The three calls above with an fp32 dictionary [H][D] (row h = the decoder's weights of hidden unit h) in place of the
 * packed n-bit one: recon = scale * sum_j val_j table[idx_j] + dec_bias, the arithmetic of qsae_decode_table_sparse, done
 * by the refinement kernel for every row it ranks.  Two users: BaselineSparseAutoencoder.forward (sae/baseline.py:17-31;
 * table = decoder.weight transposed, scale = 1) and BinarySAE.forward on a checkpoint whose decoder logits are not
 * polarised (sae/binary.py:24-47 with the soft integers of :26-35; table = qsae_binary_soft_table, scale =
 * quantization step).  table and recon 16-byte aligned; otherwise as above. */
int qsae_table_forward_prefilter(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                 int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                 int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon, void* workspace,
                                 size_t workspace_bytes, int spec_rows, int* flagged_rows, qsae_stream_t stream);
int qsae_prefilter_submit_table(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon, void* workspace,
                                size_t workspace_bytes, int* flagged_host, qsae_stream_t stream);
int qsae_prefilter_finish_table(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                int B, int D, int H, int k, const float* table, float scale, const float* dec_bias,
                                int32_t* idx, float* val, float* dense, int64_t dense_ld, float* recon, void* workspace,
                                size_t workspace_bytes, int flagged, qsae_stream_t stream);

/* dense[b][h] = val if (b,h) selected else +0; dense [B][ld].  Replaces zeros_like+scatter_. */
int qsae_densify(const int32_t* idx, const float* val, int B, int k, int H, float* dense, int64_t ld,
                 qsae_stream_t stream);

/* -- BinarySAE decoder (sae/binary.py:10-69) ---------------------------------------------- */
/* Bytes per packed dictionary row: D fields of width fw = 1,2,4,8 (smallest power of two >=
 * n_bits), rounded up to a multiple of 4 bytes. */
int qsae_binary_row_bytes(int D, int n_bits);
/* Hard two's-complement packer == binary_decoder.quantized_int_weights(), sae/binary.py:49-58:
 * bit = sigmoid(logit) > 0.5; logits [H][D*n_bits] (column d*n+b = bit b of output d, LSB first,
 * MSB negative) -> packed [H][row_bytes], fields little-endian.  If polarize_sum != NULL the
 * device double receives sum(p(1-p)2^b) (sae/binary.py:42-43; caller divides by H*D*n).
 * If soft_gap != NULL the device float receives max over (h, d) of |soft - hard| with
 * soft = sum_b sigmoid(logit_b) bw_b -- the integer the reference's forward actually multiplies
 * with (sae/binary.py:26-35) -- and hard the packed integer: the distance, in integer steps,
 * between the reference forward and a hard-bit decode of this checkpoint (~1e-12 at +-30
 * logits, ~0.5 for an untrained decoder; +inf for NaN logits).  The host side uses it to pick
 * qsae_decode_binary_sparse (hard) or qsae_decode_table_sparse over qsae_binary_soft_table. */
int qsae_pack_binary(const float* logits, int H, int D, int n_bits, uint8_t* packed,
                     double* polarize_sum, float* soft_gap, qsae_stream_t stream);
/* int_weights[h][d] as fp32 (for decoder_dictionary(), inference/framework.py:114-124). */
int qsae_unpack_binary(const uint8_t* packed, int H, int D, int n_bits, float* int_weights,
                       qsae_stream_t stream);
/* recon[b][d] = step * sum_j val[b][j] * w[idx[b][j]][d] + bias[d]  -- the reference's dense
 * `latent.matmul(int_weights)` (sae/binary.py:38) evaluated on the k non-zeros only. */
int qsae_decode_binary_sparse(const int32_t* idx, const float* val, int B, int k,
                              const uint8_t* packed, int H, int D, int n_bits, float step,
                              const float* bias, float* recon, qsae_stream_t stream);
/* Same with an fp32 table [H][D]: Baseline decoder nn.Linear(H, D) (sae/baseline.py:12,29; the
 * table is decoder.weight transposed) and BinarySAE's "soft" int_weights for unpolarised
 * checkpoints (sae/binary.py:26-38).  scale == 1 skips the multiply. */
int qsae_decode_table_sparse(const int32_t* idx, const float* val, int B, int k, const float* table,
                             int H, int D, float scale, const float* bias, float* recon,
                             qsae_stream_t stream);
/* Soft int_weights table of sae/binary.py:26-35: table[h][d] = sum_b sigmoid(logit)*bw[b]. */
int qsae_binary_soft_table(const float* logits, int H, int D, int n_bits, float* table,
                           qsae_stream_t stream);

/* -- Ternary decoder (sae/ternary.py:41-52) ---------------------------------------------- */
/* codes2 [D][ceil(H/16)] uint32: 2-bit fields, 0 -> 0, 1 -> +1, 3 -> -1 (two's complement),
 * hard = sign(w) * (|w| >= 0.5); w is decoder.weight [D][H]. */
int qsae_pack_ternary(const float* w, int D, int H, uint32_t* codes2, qsae_stream_t stream);
/* recon[b][d] = sum_h h[b][h] * hard[d][h]   (no bias), h [B][ld]. */
int qsae_decode_ternary_dense(const float* h, int64_t ld, int B, int H, const uint32_t* codes2, int D,
                              float* recon, qsae_stream_t stream);

/* -- Matryoshka decoder (sae/quantized_matryoshka.py:10-143) ------------------------------ */
/* level sizes of :25-38; sizes[n_bits]. Host-side helper. */
int qsae_matryoshka_sizes(int H, int n_bits, int32_t* sizes);
/* codes2t [D][ceil(H/16)] uint32 2-bit two's-complement fields of S/2 in {-1,0,+1} where
 * S = sgn(sig(w)>=.5)+sgn(sig(wm)>=.5) (:67-80), transposed so that H is contiguous;
 * scale[j] = reciprocal(||S_j||+1e-8) * 2^(n-i-2) * abs_range/2^(n-1) for j in level i (:82-90).
 * level_sizes: HOST array of n_bits level sizes summing to H, or NULL for qsae_matryoshka_sizes(H)
 * (a caller that pads levels to multiples of 32 passes the padded sizes). */
int qsae_pack_matryoshka(const float* w, const float* wm, int H, int D, int n_bits, float abs_range,
                         const int32_t* level_sizes, uint32_t* codes2t, float* scale,
                         qsae_stream_t stream);
/* levels[i][b][d] cumulative reconstructions (:121-129), l0_counts[i] = number of set z bits in
 * level i over the whole batch (latent_group[i] = l0_counts[i] / B, :128).
 * zbits as produced by qsae_encode_bits.  Level boundaries (and H) must be multiples of 32. */
int qsae_decode_matryoshka(const uint32_t* zbits, int64_t words_ld, int B, int H, int D, int n_bits,
                           const int32_t* level_sizes, const uint32_t* codes2t, const float* scale,
                           const float* bias, int allow_bias, float* levels,
                           unsigned long long* l0_counts, qsae_stream_t stream);
/* The same z bits as qsae_encode_bits (z = sigmoid(x W^T + b) > 0.5, sae/quantized_matryoshka.py:97-99,217-220)
 * without computing every latent in fp32: the fp16 candidate sweep of the prefilter (tau = the fp32 cutoff of
 * sigmoid > 0.5, Wq/meta from qsae_prefilter_pack_w) lists the latents within 2 eps_b of the cutoff or above it;
 * latents above cutoff + eps_b get bit 1 directly, the few inside the band are re-evaluated with the exact fp32
 * chain.  Bit-identical to qsae_encode_bits.  Rows with more than 2048 listed latents (dense activations) and
 * rows with non-finite inputs are recomputed by the exact dense kernel; *flagged_rows (host int, may be NULL)
 * receives their count so that a caller can route a dense-regime model to qsae_encode_bits.  D in {128,256,512},
 * H % 64 == 0, else QSAE_ERR_UNSUPPORTED.  One host round trip per call (that count). */
size_t qsae_encode_bits_prefilter_workspace_bytes(int B, int D, int H);
int qsae_encode_bits_prefilter(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                               int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                               size_t workspace_bytes, int* flagged_rows, qsae_stream_t stream);
/* The same in two calls (see qsae_prefilter_submit / _finish): submit enqueues everything up to the bit resolution and the
 * asynchronous copy of the flagged-row count into *flagged_host; finish, given that count, enqueues the exact dense kernel
 * for those rows.  Bits of unflagged rows are final after submit; workspace untouched in between. */
int qsae_encode_bits_prefilter_submit(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                      int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                                      size_t workspace_bytes, int* flagged_host, qsae_stream_t stream);
int qsae_encode_bits_prefilter_finish(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                      int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                                      size_t workspace_bytes, int flagged, qsae_stream_t stream);
/* The same bits when the activations are DENSE (an untrained encoder: half of the units fire; the lists of the call above
 * overflow and every row would take the exact fp32 contraction): an fp16 MFMA pass classifies EVERY latent -- bit 1 above
 * cutoff + eps_b, bit 0 below cutoff - eps_b -- and lists only the latents inside the band (~0.7 % of them), which are
 * re-evaluated with the exact fp32 chain.  Bit-identical to qsae_encode_bits.  Rows with more than 1024 band entries or
 * non-finite inputs are recomputed by the exact dense kernel (*flagged_rows).  D % 64 == 0, H % 32 == 0, else
 * QSAE_ERR_UNSUPPORTED.  One host round trip per call. */
size_t qsae_encode_bits_band_workspace_bytes(int B, int D, int H);
int qsae_encode_bits_band(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                          int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                          size_t workspace_bytes, int* flagged_rows, qsae_stream_t stream);
/* ... and in two calls (as qsae_encode_bits_prefilter_submit / _finish). */
int qsae_encode_bits_band_submit(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                 int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                                 size_t workspace_bytes, int* flagged_host, qsae_stream_t stream);
int qsae_encode_bits_band_finish(const float* x, const float* W, const float* bias, const void* Wq, const float* meta,
                                 int B, int D, int H, uint32_t* zbits, int64_t words_ld, void* workspace,
                                 size_t workspace_bytes, int flagged, qsae_stream_t stream);
/* Hidden-major dictionary for the sparse decoder: codes_rows[j][ceil(D/8)] uint32, 4-bit two's-complement
 * fields of S_j/2 (same S as qsae_pack_matryoshka; ABI 4: 2-bit fields, ceil(D/16) words per row, until ABI 3). */
int qsae_pack_matryoshka_rows(const float* w, const float* wm, int H, int D, uint32_t* codes_rows,
                              qsae_stream_t stream);
/* qsae_decode_matryoshka evaluated on the active units only (ascending walk over the row's z bits, one fmaf
 * per active unit and output column): the same chain as the dense kernel, whose z = 0 terms leave the
 * accumulator unchanged -- bit-identical levels and l0_counts.  Pays off below ~5 % active units.
 * D in {64,128,256,512,1024}; H % 32 == 0 (level boundaries need no alignment here). */
int qsae_decode_matryoshka_sparse(const uint32_t* zbits, int64_t words_ld, int B, int H, int D, int n_bits,
                                  const int32_t* level_sizes, const uint32_t* codes_rows, const float* scale,
                                  const float* bias, int allow_bias, float* levels,
                                  unsigned long long* l0_counts, qsae_stream_t stream);
/* zbits[b][w] bit j = dense[b][32w+j] > thr -- the `latent > 0.5` binarisation applied to an
 * already materialised sigmoid latent (sae/quantized_matryoshka.py:97-99 when the decoder is
 * called directly, scripts/analysis/dynamic_analysis.py:51,66). */
int qsae_pack_bits_gt(const float* dense, int64_t ld, int B, int H, float thr, uint32_t* zbits,
                      int64_t words_ld, qsae_stream_t stream);

/* -- the dense decoders on the bf16 matrix pipe ------------------------------------------------------ */
/* qsae_decode_ternary_dense and qsae_decode_matryoshka contract a dictionary of {-1, 0, +1} with fp32 MFMA, at 1/16 of the
 * bf16 rate.  The *_split forms give the same sums from v_mfma_f32_32x32x16_bf16: the fp32 operand (the latent h, resp.
 * z_j * 2 scale_j) is split exactly into three bf16 terms (8 + 8 + 8 mantissa bits), the dictionary entries are exact in
 * bf16, so every product is exact and the three passes add into one fp32 accumulator.  What differs from the fp32 kernels
 * is the order of the fp32 accumulation roundings (results agree to ~1e-6 relative; both are graded at 1e-5 against the
 * fp64-accumulating oracle).  D == 512, H % 64 == 0 (matryoshka: level boundaries % 64 == 0); qsae_split_dec_supported() says
 * whether a shape qualifies.
 *   qsae_expand_codes_bf16: once per checkpoint, codes2 [D][ceil(H/16)] (as produced by qsae_pack_ternary or
 *     qsae_pack_matryoshka) -> the bf16 image the kernels stream (qsae_expand_codes_bf16_bytes() = 2 H D bytes, opaque);
 *   qsae_split_scale_bf16: once per checkpoint, scale [H] (qsae_pack_matryoshka) -> the three bf16 terms of 2 scale,
 *     s3 [3][H] bf16 (6 H bytes). */
int qsae_split_dec_supported(int B, int H, int D);
size_t qsae_expand_codes_bf16_bytes(int D, int H);
int qsae_expand_codes_bf16(const uint32_t* codes2, int D, int H, void* tq, qsae_stream_t stream);
/* recon[b][d] = sum_h h[b][h] * hard[d][h] (sae/ternary.py:41-52), h [B][ld] fp32. */
int qsae_decode_ternary_dense_split(const float* h, int64_t ld, int B, int H, const void* tq, int D, float* recon,
                                    qsae_stream_t stream);
int qsae_split_scale_bf16(const float* scale, int H, void* s3, qsae_stream_t stream);
/* levels / l0_counts as qsae_decode_matryoshka (sae/quantized_matryoshka.py:121-129). */
int qsae_decode_matryoshka_split(const uint32_t* zbits, int64_t words_ld, int B, int H, int D, int n_bits,
                                 const int32_t* level_sizes, const void* tq, const void* s3, const float* bias,
                                 int allow_bias, float* levels, unsigned long long* l0_counts, qsae_stream_t stream);

/* -- small elementwise steps (each operation rounded separately, as in the reference's ATen sequence) -------- */
/* out[i] = (residual[i] - recon[i]) * scale: the residual handed to the next stage of ResidualQuantizedSAE
 * (sae/residual_quantized.py:67, scale = 2).  out may alias residual. */
int qsae_residual_update(const float* residual, const float* recon, size_t n, float scale, float* out,
                         qsae_stream_t stream);
/* out[i] = pre[i] >= cutoff ? 1 : 0: the binary latent of BinaryLatentSAE, sigmoid(pre) >= 0.5 <=> pre >= 0xB43FFFFE
 * (sae/binary_latent.py:21-24). */
int qsae_threshold_ge(const float* pre, size_t n, float cutoff, float* out, qsae_stream_t stream);
/* out[b][d] = scale * acc[b][d] + bias[d] (bias may be NULL): the tail of binary_decoder.forward on an arbitrary dense
 * latent, reconstruction = quantization_step * latent.matmul(int_weights) + bias (sae/binary.py:38). */
int qsae_scale_bias_rows(const float* acc, int B, int D, float scale, const float* bias, float* out,
                         qsae_stream_t stream);

/* -- metric ------------------------------------------------------------------------------ */
/* *sum += sum_i (float)((recon[i]-x[i])^2) accumulated in double (device pointer; the caller
 * zeroes it).  scripts/analysis/dynamic_analysis.py:86-100. */
int qsae_sq_err_sum(const float* recon, const float* x, size_t n, double* sum, qsae_stream_t stream);

/* -- consumers of the sparse latent (scripts/analysis/dynamic_analysis.py:255-311, 314-440) ---------------- */
/* counts[idx[b][j]] += 1 for every entry with val[b][j] > 0 (val == NULL: every entry): mask.sum(dim=0) of the
 * reference's activation mask `latent > 0`, accumulated over calls (the caller zeroes counts[H], uint64). */
int qsae_activation_counts(const int32_t* idx, const float* val, int B, int k, int H, unsigned long long* counts,
                           qsae_stream_t stream);
/* The same for bit-packed masks (`latent > 0.5` of the matryoshka / residual encoders): counts[32 w + j] += bit j
 * of zbits[b][w]; nbits a multiple of 32. */
int qsae_activation_counts_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, unsigned long long* counts,
                                qsae_stream_t stream);
/* coact[a][c] += 1 for every ordered pair of units active in the same row, diagonal included: the reference's
 * mask_int.t() @ mask_int (dynamic_analysis.py:296, 411), accumulated over calls into an int32 [H][ld] matrix. */
int qsae_coactivation_sparse(const int32_t* idx, const float* val, int B, int k, int H, int32_t* coact, int64_t ld,
                             qsae_stream_t stream);

/* The same matrix for bit-packed masks, on the int8 matrix pipe: coact[u(p)][u(q)] += sum_b bit(b, p) & bit(b, q) for
 * every ordered pair of packed positions p, q < nbits (diagonal included), accumulated over calls into the caller's
 * int32 [H][ld] matrix.  zbits uint32 [B][words_ld], bit j of word w = packed position 32 w + j (the layout
 * qsae_activation_counts_bits reads); nbits a positive multiple of 32, words_ld >= nbits / 32, ld >= H.
 * u() = index[nbits] (int32, device): destination unit of a packed position, -1 = inert pad slot -- never written, and
 * its bits are masked, they need not be zero.  index == NULL: identity, requires nbits <= H.  Two positions must not
 * map to the same unit, and values outside [-1, H) are the caller's duty (the kernel drops values >= H, it does not
 * report them).  The only scratch is the bit transpose of the input in `workspace` (16-byte aligned,
 * qsae_coactivation_bits_workspace_bytes(B, nbits) = nbits * ceil(B / 256) * 32 bytes; 0 for an invalid shape): no
 * [B, H] mask of bytes or floats is formed.  QSAE_ERR_INVALID_ARG before any HIP call; QSAE_ERR_WORKSPACE when the
 * workspace is too small. */
size_t qsae_coactivation_bits_workspace_bytes(int B, int nbits);
int qsae_coactivation_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index, int H,
                           int32_t* coact, int64_t ld, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- co-activation partner sets: one bit per pair (scripts/analysis/summarize_stats.py:37-70) -------------------- */
/* average_coactivating_features reads `coactivation > 0` only: for every feature, how many other features ever fired
 * with it.  That is one bit per pair of state, OR-accumulated over calls, instead of an int32 count.
 * partners is uint32 [P][ld_words] on the device, P = the number of packed positions; bit q & 31 of word q >> 5 of row p
 * = positions p and q were active in the same row at least once.  The diagonal is included: bit (p, p) = p was active
 * at all.  ld_words >= P / 32.  The caller zeroes the state; every call ORs into it and clears nothing.  The state
 * stays in packed-position space; a position -> unit map is applied once, by qsae_coactivation_partner_counts.
 *
 * Bits form (threshold models): zbits, words_ld, B, nbits, index and the workspace as in qsae_coactivation_bits (same
 * bit transpose, same int8-MFMA main loop, same qsae_coactivation_bits_workspace_bytes(B, nbits)); P = nbits.  index is
 * used only to mask: positions with index[p] < 0 are inert (their bits are ignored and need not be zero, their rows and
 * columns of partners stay as they are); index == NULL masks nothing.  Rows and words at or past nbits are not
 * written.  QSAE_ERR_INVALID_ARG before any HIP call; QSAE_ERR_WORKSPACE when the workspace is missing or too small;
 * B == 0 does nothing. */
int qsae_coactivation_partners_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index,
                                    uint32_t* partners, int64_t ld_words, void* workspace, size_t workspace_bytes,
                                    qsae_stream_t stream);
/* Compact form (top-k models): positions are units, P = H rounded up to a multiple of 32, ld_words >= ceil(H / 32); bits
 * at columns >= H are never set.  Row r is active in unit idx[r][j] when val[r][j] > 0 (NaN, 0.0 and -0.0 are not; val
 * == NULL: every entry); entries outside [0, H) are dropped; 1 <= k <= 256 (QSAE_ERR_INVALID_ARG otherwise).  Bit c of
 * row a is set for every ordered pair (a, c) of a row's active units.  A unit listed twice in one row sets its bits
 * once, as the mask has one bit -- unlike qsae_coactivation_sparse, which counts such a unit twice.  B == 0 does
 * nothing. */
int qsae_coactivation_partners_sparse(const int32_t* idx, const float* val, int B, int k, int H, uint32_t* partners,
                                      int64_t ld_words, qsae_stream_t stream);
/* counts[u(p)] = popcount(row p of partners over words [0, P / 32)) - bit(p, p): the number of other positions that
 * were ever active together with p, for every p < P whose unit u(p) = index[p] lies in [0, H).  index == NULL: the
 * identity, over rows p < min(P, H).  counts is int32 [H]; the call clears it on the stream first, so units without a
 * position get 0.  P a positive multiple of 32, ld_words >= P / 32; two positions must not map to one unit. */
int qsae_coactivation_partner_counts(const uint32_t* partners, int P, int64_t ld_words, const int32_t* index, int H,
                                     int32_t* counts, qsae_stream_t stream);
/* The same count from co-activation counts that already exist as an int32 matrix (a saved dynamic_stats_*.pt, or the
 * result of qsae_coactivation_bits / _sparse): counts[i] = #{j < H, j != row0 + i : coact[i][j] > 0} for the R rows
 * row0 .. row0 + R - 1 of the [H][H] matrix, given as a slab int32 [R][ld], ld >= H -- so a matrix that lives on the
 * host can be streamed through the device slab by slab.  counts is int32 [R], written, not accumulated.  R == 0 does
 * nothing. */
int qsae_coactivation_partner_counts_dense(const int32_t* coact, int64_t ld, int R, int H, int64_t row0, int32_t* counts,
                                           qsae_stream_t stream);

/* -- tokens per feature as ordered CSR lists (scripts/analysis/dynamic_analysis.py:283-306) -------------------- */
/* tokens_per_feature[f] of the reference holds the token of every row whose mask bit f is set, in ascending row order
 * (the order of mask.nonzero()), batch after batch.  Here it is a CSR pair on the device: offsets int64 [H + 1] with
 * offsets[0] = 0 and tokens int32 [offsets[H]], feature f in tokens[offsets[f] .. offsets[f + 1]).  A batch is built in
 * two calls -- a count that leaves the batch's offsets (so that the caller can size the token buffer from offsets[H])
 * and a unit-major row bitmap in the workspace, then qsae_token_lists_fill from that same, untouched workspace -- and
 * the batches are joined by qsae_token_lists_regroup.  List positions are prefix counts over the bitmap, never an
 * atomic counter: the result does not depend on scheduling.  No [B, H] mask of bytes is formed; the scratch is the
 * bitmap, qsae_token_lists_workspace_bytes(B, H) = align256(H * 2 ceil(B / 64) * 4) + align256(H * 4) bytes (one bit per
 * row and unit; 0 for an invalid shape: B < 0 or H <= 0).  The workspace must be 16-byte aligned.
 * Limits: every index into the bitmap and into tokens is 64-bit, so B * H and the number of entries may exceed 2^31
 * (B = 65536 at H = 32768 is one call); the compact form requires B * k < 2^31 and the bits form nbits <= 134215680,
 * otherwise QSAE_ERR_UNSUPPORTED.  QSAE_ERR_INVALID_ARG before any HIP call; QSAE_ERR_WORKSPACE when the workspace is
 * missing or too small.  B == 0 leaves all-zero offsets and needs no workspace. */
size_t qsae_token_lists_workspace_bytes(int B, int H);
/* Compact form (top-k models): row r is active in unit idx[r][j] when val[r][j] > 0 (NaN, 0.0 and -0.0 are not; val ==
 * NULL: every entry, as in qsae_activation_counts).  Entries outside [0, H) are dropped; a unit listed twice in one row
 * counts once (the mask has one bit). */
int qsae_token_lists_count(const int32_t* idx, const float* val, int B, int k, int H, int64_t* offsets, void* workspace,
                           size_t workspace_bytes, qsae_stream_t stream);
/* Bits form (threshold models): zbits uint32 [B][words_ld], bit j of word w = packed position 32 w + j; nbits a
 * positive multiple of 32, words_ld >= nbits / 32.  index[nbits] (int32, device) follows qsae_coactivation_bits: the
 * destination unit of a packed position, -1 = inert pad slot, whose bits are ignored and need not be zero (values >= H
 * are dropped too); two positions must not map to one unit.  index == NULL: identity, requires nbits <= H.  offsets
 * come out in unit order. */
int qsae_token_lists_count_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index, int H,
                                int64_t* offsets, void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* tokens[offsets[u] + rank] = row_tokens[r] for every active (r, u) of the batch whose count call left `workspace` and
 * `offsets`; rank = active rows of u before r.  row_tokens int32 [B]: the token id of each row, written as it is (no
 * row number that a second pass would gather).  n_entries = the capacity of tokens, normally offsets[H]; nothing is
 * written at or past it.  B == 0 or n_entries == 0: nothing to do. */
int qsae_token_lists_fill(const void* workspace, size_t workspace_bytes, const int64_t* offsets, const int32_t* row_tokens,
                          int B, int H, int32_t* tokens, int64_t n_entries, qsae_stream_t stream);
/* Joins nb batches: batch_offsets int64 [nb][H + 1] (each row as a count call left it) and segments int32
 * [n_entries], the batches' token buffers back to back in batch order -> offsets int64 [H + 1] of the whole dataset and
 * tokens int32 [n_entries] feature-major, the segments of a feature in batch order.  n_entries must be the sum of the
 * batches' totals; reads and writes stay inside [0, n_entries) whatever batch_offsets holds.  nb == 0: all-zero
 * offsets. */
int qsae_token_lists_regroup(const int64_t* batch_offsets, int nb, int H, const int32_t* segments, int64_t n_entries,
                             int64_t* offsets, int32_t* tokens, qsae_stream_t stream);

/* -- token overlap between two SAEs (scripts/analysis/summarize_stats.py:100-156, 320-378) -------------------- */
/* The script scores every pair (a, b) of live features of two SAEs as |A & B| / |A | B| over their top-k token sets and
 * keeps every score.  A score is fixed by (inter, union) with inter <= k and union <= 2k, so the whole result is the
 * table hist[k + 1][2k + 1] (int64, device, accumulated into -- the caller zeroes it):
 *   hist[i][u] += #{(a, b) : asize[a] > 0, bsize[b] > 0, |A_a & B_b| = i, asize[a] + bsize[b] - i = u},
 * pairs with an empty intersection included, at (0, asize + bsize).  The intersections of all pairs are the product of
 * the two 0/1 membership matrices, formed on the int8 matrix pipe from the packed bits; no [Na][Nb] matrix exists.
 * asets uint32 [Na][a_ld]: bit t & 31 of word t >> 5 of row i = token t is in the set of feature i; a_ld >= ceil(V / 32);
 * bits at or past V in the last word are masked, they need not be zero.  asize[i] (int32, device) is the true size of
 * the set -- passed, not popcounted, because the caller may have dropped tokens that cannot be in any intersection --
 * and 0 means no set: that feature takes part in no pair.  bsets / b_ld / bsize / Nb: the same for the other side.
 * A pair that contradicts itself is not counted and touches no memory: a size above k or below 0, or an intersection
 * larger than either size (sizes smaller than the bits say).  Callers see that as sum(hist) falling short of
 * #{asize > 0} * #{bsize > 0}.
 * 1 <= k <= 128, otherwise QSAE_ERR_UNSUPPORTED.  Na == 0 or Nb == 0: nothing to do, no pointer is looked at.
 * workspace: 16-byte aligned, qsae_token_overlap_hist_workspace_bytes(Na, Nb, V) = (Na + Nb) * ceil(V / 256) * 32
 * bytes (both bitsets re-tiled by 256-token chunk; 0 for an invalid shape).  QSAE_ERR_INVALID_ARG before any HIP call;
 * QSAE_ERR_WORKSPACE when the workspace is too small. */
size_t qsae_token_overlap_hist_workspace_bytes(int Na, int Nb, int V);
int qsae_token_overlap_hist(const uint32_t* asets, int64_t a_ld, const int32_t* asize, int Na, const uint32_t* bsets,
                            int64_t b_ld, const int32_t* bsize, int Nb, int V, int k, int64_t* hist, void* workspace,
                            size_t workspace_bytes, qsae_stream_t stream);

/* -- activation quantizer of the binary datasets (src/quantized_sae/data/dataset.py:76-102) ----------------- */
/* bits[b][d*n + j] = bit j (LSB first, as 0.0 / 1.0) of the n-bit code of x[b][d]:
 *   is_signed = 0 (quantize):        int(round(clamp((x * sf) * 2 + 2^(n-1), 0, 2^n - 1)))
 *   is_signed = 1 (quantize_signed): int(round(clamp(x * sf, -2^(n-1), 2^(n-1) - 1))) & (2^n - 1)
 * with sf = scale_factor = 2^(n-1) / (gamma + 1e-5) rounded to fp32, round half to even. */
int qsae_quantize_bits(const float* x, int64_t ld, int B, int D, int n_bits, float scale_factor, int is_signed,
                       float* bits, qsae_stream_t stream);

/* -- decoder dictionary comparison (scripts/analysis/analyze_sae.py:24-91, data/load_baseline.py:102-122) ---- */
/* inv_norm[h] = 1 / max(||atoms[h]||_2, 1e-12), squares summed in fp64 (F.normalize semantics: a zero atom has
 * cosine 0 with everything).  atoms [H][ld] fp32. */
int qsae_atom_inv_norms(const float* atoms, int64_t ld, int H, int D, float* inv_norm, qsae_stream_t stream);
/* Device workspace of qsae_cosine_compare (0 for an invalid shape); in self mode Hb is ignored. */
size_t qsae_cosine_compare_workspace_bytes(int Ha, int Hb, int self_mode);
/* Cosine similarities c(i, j) = (a_i . b_j)_fp32-chain * (inv_a[i] * inv_b[j]) of atoms A [Ha][lda] and B [Hb][ldb]
 * (fp32, 16-byte aligned, D, lda, ldb multiples of 4), reduced without forming the matrix.  Every output is
 * overwritten.  Keys are (order-preserving bits of c) << 32 | ~index, 0 = none (ties go to the lower index):
 *   row_best[i] (u64 [Ha]) best (c, j) of row i;  col_best[j] (u64 [Hb]) best (c, i) of column j;
 *   moments = {sum c, sum c^2} in fp64, summed in a fixed order;  extrema = {key(max), ~key(min)} (32-bit keys);
 *   counts[t] = #pairs with c > thresholds[t] (n_thresholds <= 8, thresholds in host memory);
 *   hist[b] (bins <= 4096, NULL when 0): #pairs with clamp(floor((c + 1) * (bins / 2)), 0, bins - 1) == b (fp32);
 *   out (nullable): c stored into [Ha][out_ld].
 * self_mode != 0: B is A (B, ldb, Hb, col_best ignored); only pairs i < j count, a pair updates row_best[i] with
 * (c, j) and row_best[j] with (c, i); `out` then receives the tiles on and above the diagonal only (c(j, i) == c(i, j)
 * bit for bit, the caller mirrors). */
int qsae_cosine_compare(const float* A, int64_t lda, int Ha, const float* B, int64_t ldb, int Hb, int D, int self_mode,
                        const float* thresholds, int n_thresholds, int bins, unsigned long long* row_best,
                        unsigned long long* col_best, double* moments, unsigned long long* extrema,
                        unsigned long long* counts, unsigned long long* hist, float* out, int64_t out_ld,
                        void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- nearest atoms of an integer dictionary (src/quantized_sae/utils/inspector.py:47-67, 110-121) ------------- */
/* The k nearest atoms (cosine) of every atom of A among the atoms of B, for int8 dictionaries (ternary, n-bit two's
 * complement), without the [Na][Nb] matrix.  a [Na][a_ld], b [Nb][b_ld] int8 on the device; b == NULL is self mode
 * (B = A; b_ld and Nb are ignored).  Arithmetic, exact and order-free:
 *   nsq[i] = sum_d a[i][d]^2 (int32);  inv[i] = fp32(1 / sqrt(fp64(nsq[i]))), 1.0f for an all-zero atom (cosine 0 with
 *   everything, itself included);  dot(i, j) exact in int32;  c(i, j) = fp32(dot) * (inva[i] * invb[j]) -- the two
 *   inverse norms multiplied first, so c(i, j) and c(j, i) of one dictionary are the same bits.
 * keys [Na][k] (u64, overwritten): row i holds its k largest keys (order-preserving bits of c) << 32 | ~j in
 * descending order -- largest cosine first, equal bits to the lowest index; 0 = none, where fewer than k candidates
 * exist.  Keys of a row are distinct, so the result does not depend on tiling, grid or column split.
 * exclude_self != 0 skips j == i.  duplicate_of (int32 [Na], nullable, overwritten): the lowest j with atom j
 * identical to atom i (i itself when there is none lower), tested as dot(i, j) == nsq[i] == nsq[j]; all-zero atoms
 * are identical among themselves.  Both need self mode: QSAE_ERR_INVALID_ARG otherwise.
 * Limits: 1 <= k <= 64, D a multiple of 32 in [32, 4096] (zero-pad: padding changes no dot product and no norm),
 * otherwise QSAE_ERR_UNSUPPORTED; strides >= D and multiples of 16, pointers 16-byte aligned.  Bytes of a row at or
 * past D are not read.  Na == 0 or Nb == 0: nothing to do, no pointer is looked at.  QSAE_ERR_INVALID_ARG /
 * QSAE_ERR_UNSUPPORTED before any HIP call; QSAE_ERR_WORKSPACE when the workspace is missing or too small.
 * workspace: 16-byte aligned, qsae_nearest_atoms_i8_workspace_bytes(Na, Nb, D, k) bytes (norms of both sides and the
 * partial lists of a column split; self mode: pass Nb = Na; 0 for an invalid shape; monotone in Na, Nb and k). */
size_t qsae_nearest_atoms_i8_workspace_bytes(int Na, int Nb, int D, int k);
int qsae_nearest_atoms_i8(const int8_t* a, int64_t a_ld, int Na, const int8_t* b, int64_t b_ld, int Nb, int D, int k,
                          int exclude_self, uint64_t* keys, int32_t* duplicate_of, void* workspace,
                          size_t workspace_bytes, qsae_stream_t stream);

/* -- nearest atoms of an fp32 dictionary (scripts/analysis/analyze_sae.py:59-91 followed by a top-k) ----------- */
/* The k nearest atoms (cosine) of every atom of A among the atoms of B, for fp32 dictionaries, without the [Na][Nb]
 * matrix.  a [Na][a_ld], b [Nb][b_ld] fp32 on the device; b == NULL is self mode (B = A; b_ld and Nb are ignored).
 * Arithmetic, every step fixed:
 *   inv[i] = what qsae_atom_inv_norms computes: fp32(1 / max(sqrt(fp64 sum of squares), 1e-12)), so an all-zero atom
 *   has cosine +0 with everything, itself included;  acc(i, j) = the fmaf chain over d ascending from +0 (the bits of
 *   qsae_cosine_compare's accumulator);  c(i, j) = acc * (inva[i] * invb[j]) -- the two inverse norms multiplied
 *   first, so c(i, j) and c(j, i) of one dictionary are the same bits.
 * keys [Na][k] (u64, overwritten): row i holds its k largest keys (order-preserving bits of c, -0 as +0) << 32 | ~j in
 * descending order -- largest cosine first, equal bits to the lowest index; 0 = none, where fewer than k candidates
 * exist.  Keys of a row are distinct, so the result does not depend on tiling, grid or candidate split.
 * exclude_self != 0 skips j == i and needs self mode: QSAE_ERR_INVALID_ARG otherwise.  There is no duplicate_of here:
 * identity of fp32 vectors cannot be decided from rounded dot products.  Atoms with a non-finite component give
 * unspecified neighbours for the rows and columns they touch (never an access out of range).
 * Limits: 1 <= k <= 64 and D a positive multiple of 4 (zero-pad), otherwise QSAE_ERR_UNSUPPORTED; strides >= D and
 * multiples of 4, pointers 16-byte aligned.  Floats of a row at or past D are not read.  Na == 0 or Nb == 0: nothing
 * to do, no pointer is looked at.  QSAE_ERR_INVALID_ARG / QSAE_ERR_UNSUPPORTED before any HIP call;
 * QSAE_ERR_WORKSPACE when the workspace is missing or too small.
 * workspace: 16-byte aligned, qsae_nearest_atoms_f32_workspace_bytes(Na, Nb, D, k) bytes (inverse norms of both sides
 * and the partial lists of a candidate split; self mode: pass Nb = Na; 0 for an invalid shape; monotone in Na, Nb
 * and k). */
size_t qsae_nearest_atoms_f32_workspace_bytes(int Na, int Nb, int D, int k);
int qsae_nearest_atoms_f32(const float* a, int64_t a_ld, int Na, const float* b, int64_t b_ld, int Nb, int D, int k,
                           int exclude_self, uint64_t* keys, void* workspace, size_t workspace_bytes,
                           qsae_stream_t stream);

/* -- k-means over dictionary atoms (utils/inspector.py:137-165 k_means_analysis) ------------------------------- */
/* The assign step of Lloyd's algorithm without the [N][C] matrix.  atoms [N][a_ld], centers [C][c_ld] fp32 on the
 * device.  keys [N] (u64, overwritten): keys[i] = the largest (order-preserving bits of s(i, j), -0 as +0) << 32 | ~j
 * over j < C -- the largest score, equal bits to the lowest center; 0 = every score of the atom was NaN.
 * Scores, every step fixed:  acc(i, j) = the fmaf chain over d ascending from +0;
 *   metric 0 (cosine):     s = acc * (inv_a[i] * inv_c[j]), inv = what qsae_atom_inv_norms computes -- the bits of
 *                          qsae_nearest_atoms_f32(atoms, centers, k = 1); an all-zero atom or center has cosine +0;
 *   metric 1 (euclidean):  s = acc - h[j], h[j] = fp32(0.5 * nsq64[j]), nsq64 = the fp64 sum of squares of center j in
 *                          qsae_atom_inv_norms' order; one separately rounded subtraction.  The largest s is the
 *                          smallest |atom - center|^2.
 * The result does not depend on tiling, grid or the split of the centers (a maximum of distinct integers).
 * Limits: D a positive multiple of 4 (zero-pad), otherwise QSAE_ERR_UNSUPPORTED; C >= 1; strides >= D and multiples
 * of 4; atoms, centers and workspace 16-byte aligned.  Floats of a row at or past D are not read.  N == 0: nothing to
 * do, no pointer is looked at.  QSAE_ERR_INVALID_ARG / QSAE_ERR_UNSUPPORTED before any HIP call; QSAE_ERR_WORKSPACE when
 * the workspace is missing or too small.
 * workspace: qsae_kmeans_assign_f32_workspace_bytes(N, C, D) bytes (per-atom and per-center scale, padded to the tile;
 * 0 for an invalid shape; monotone in N, C and D). */
size_t qsae_kmeans_assign_f32_workspace_bytes(int N, int C, int D);
int qsae_kmeans_assign_f32(const float* atoms, int64_t a_ld, int N, const float* centers, int64_t c_ld, int C, int D,
                           int metric, uint64_t* keys, void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* The update step.  labels [N] int32: the cluster of every atom; a label outside [0, C) belongs to no cluster.
 * counts [C] int32, centers_new [C][new_ld], stats [2] double = {center_shift, n_empty}: all overwritten (floats of a
 * centers_new row at or past D are not written).  Members of a cluster are taken in ascending atom index; sum64[c][d] is
 * built from chunks of 64 consecutive members, each an fp64 chain from 0.0 in member order, the chunk partials added in
 * chunk order from 0.0; centers_new[c][d] = fp32(sum64 / count).  An empty cluster keeps centers_old[c] and counts in
 * n_empty.  center_shift = sum over c of sqrt(sum over d of (double(new) - double(old))^2) in fp64, in the fixed orders
 * DESIGN.md 4.20 states.  No float atomics: the same bits every run.
 * Limits, alignment, N == 0 and error codes as above; the three row strides are checked alike.
 * workspace: qsae_kmeans_update_f32_workspace_bytes(N, C, D) bytes (member bitmap C * ceil(N / 32) words, member
 * lists, chunk partials (N / 64 + C) * D doubles; 0 for an invalid shape; monotone in N, C and D). */
size_t qsae_kmeans_update_f32_workspace_bytes(int N, int C, int D);
int qsae_kmeans_update_f32(const float* atoms, int64_t a_ld, int N, int D, const int32_t* labels, int C,
                           const float* centers_old, int64_t old_ld, float* centers_new, int64_t new_ld, int32_t* counts,
                           double* stats, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- strongest activations per feature as streaming top-n lists (utils/inspector.py linguistic_analyze, ------- */
/*    print_feature_activations_overview: the examples its labelling prompt is built from) */
/* State: keys u64 [H][n] on the device, 1 <= n <= 64, every row descending and 0-padded; 0 = none.  The caller zeroes
 * it before the first batch and passes it to every update of one dataset.  A candidate of feature h is a pair (value,
 * position) with value > floor (NaN never is; at floor = 0 neither are 0.0, -0.0 and negatives: the reference's
 * `latent > 0`); position = base + row, a global token index below 2^32.  Its key is (order-preserving bits of the
 * value) << 32 | ~position: larger values win, equal values go to the lower position.  After an update keys[h] holds
 * the n largest of (old keys[h]) + (candidates of h in this batch).  Keys of one feature are distinct when positions
 * are, so the result depends only on the set of (value, position) pairs: not on batch boundaries, tiling, grid or
 * scheduling (no float atomics, no atomic counter decides a position).  Offering the same (value, position) pair
 * twice is outside the contract: the merge ranks distinct keys.
 * Errors: QSAE_ERR_INVALID_ARG (negative sizes, n < 1, NaN floor, base + B > 2^32, ld < H, null pointers) and
 * QSAE_ERR_UNSUPPORTED (n > 64, B * k >= 2^31) before any HIP call; QSAE_ERR_WORKSPACE when the workspace is missing or
 * too small; it must be 16-byte aligned.  B == 0 (or k == 0): nothing to do, no pointer is looked at.
 * The workspace sizes are 0 for an invalid shape and monotone in their arguments. */
/* Compact form: idx int32 [B][k], val fp32 [B][k] (NULL: every in-range entry is a candidate with value 1.0).  Entries
 * with idx outside [0, H) are skipped.  Precondition: the units of one row are distinct, as the top-k kernels produce
 * them; of a unit listed twice in one row, one entry is offered (which one is not fixed) and nothing is read or written
 * out of bounds.  The per-entry work is proportional to B k; every call also clears, counts and prefix-scans a bitmap
 * of one bit per (row, unit), whatever the entries hold.  qsae_top_examples_compact_workspace_bytes(B, k, H) = two
 * H * ceil(B / 32) word arrays (bitmap and prefix), 2 H + 1 and B k ints, each rounded up to 256 bytes: about 530 MiB
 * at B = 65536, k = 65, H = 32768, of which 512 MiB are written and read per call. */
size_t qsae_top_examples_compact_workspace_bytes(int B, int k, int H);
int qsae_top_examples_compact(const int32_t* idx, const float* val, int B, int k, int H, int n, float floor, uint32_t base,
                              uint64_t* keys, void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* Dense form: latent fp32 [B][ld], ld >= H; floats of a row at or past H are not read.  The workspace holds the
 * partial lists when the rows are split over several workgroups (0 bytes for B <= 64, where they never are). */
size_t qsae_top_examples_dense_workspace_bytes(int B, int H, int n);
int qsae_top_examples_dense(const float* latent, int64_t ld, int B, int H, int n, float floor, uint32_t base,
                            uint64_t* keys, void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* keys -> values fp32 [H][n] (0.0 for none), positions int64 [H][n] (-1 for none), counts int32 [H] (filled slots).
 * Needs no workspace. */
int qsae_top_examples_decode(const uint64_t* keys, int H, int n, float* values, int64_t* positions, int32_t* counts,
                             qsae_stream_t stream);

/* -- evaluation reports (scripts/evaluation/estimate_quantization_error.py, estimate_baseline_error.py) --------- */
/* Quantization error of a BinarySAE decoder: statistics of W_quant - W_float in one pass over the logits [H][D * n_bits]
 * (column d * n_bits + b is bit b of output d), without any [H][D] temporary.  Per entry (h, d), in registers:
 *   soft = what qsae_binary_soft_table computes (same helper, same order, fp32);  hard = the two's-complement integer of
 *   the sigmoid(logit) > 0.5 bits, as qsae_pack_binary packs it;  w_float = fp32(step * soft), w_quant = fp32(step * hard),
 *   diff = fp32(w_quant - w_float).
 * result: QSAE_QUANT_ERROR_WORDS 64-bit words on the device, overwritten:
 *   [0..5]  fp64 sums over all entries: diff^2, |diff|, w_float, w_float^2, w_quant, w_quant^2
 *   [6..9]  fp64 images of min w_float, max w_float, min w_quant, max w_quant (NaN entries are passed over)
 *   [10]    u64 key of the largest |diff|: (order-preserving bits of the fp32 value, NaN above +inf) << 32 | ~(h D + d),
 *           so equal values go to the lowest flat index
 *   [11]    int64 number of NaN logits (NaNs propagate into the sums)
 *   [16+b]  fp64 sum of |logit| over bit plane b;  [24+b] fp64 sum of p (1 - p), p = sigmoid(logit), over plane b;
 *   [32+b]  int64 number of logits of plane b with |logit| < margin_logit (the raw logit; NaN never is)
 *   [40+b]  the n_bits logits of the entry behind the key, as fp64;  every other word is 0.
 * unit_err_sq [H] fp64, overwritten: sum over d of diff^2 of unit h.
 * Every sum has a fixed order: within a unit, lane l of one wave adds d = l, l + 64, ... in ascending order and the 64
 * lane sums are joined by a butterfly (xor 32, 16, ..., 1); across units, thread t of 256 adds h = t, t + 256, ... in
 * ascending order and the thread sums are added in ascending t.  No float atomics: the same bits on every run.
 * Limits: 1 <= n_bits <= 8 and H * D < 2^31, otherwise QSAE_ERR_UNSUPPORTED (answered from the sizes alone, before any
 * pointer is looked at); H, D >= 1.  N = 4 and 8 read one and two 16-byte vectors per entry when logits is 16-byte
 * aligned.  workspace: 8-byte aligned, qsae_quantization_error_workspace_bytes(H, D, n_bits) = (11 + 3 n_bits) * H * 8
 * bytes rounded up to 256 (the per-unit partials); 0 for an invalid shape. */
#define QSAE_QUANT_ERROR_WORDS 48
size_t qsae_quantization_error_workspace_bytes(int H, int D, int n_bits);
int qsae_quantization_error(const float* logits, int H, int D, int n_bits, float step, float margin_logit, double* result,
                            double* unit_err_sq, void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* Dataset moments: adds the rows of x [B][D] (dtype 0 = fp32, 1 = fp16, 2 = bf16, converted in registers; contiguous)
 * to a caller-owned running state.  recon (nullable): fp32 [B][D], contiguous.  The rows of one call are cut into groups
 * of group_rows from the call's first row (the last group may be short).  A group holding a NaN in x contributes nothing
 * and its rows are counted as skipped (the reference's `if torch.isnan(batch).any(): continue` per DataLoader batch);
 * inf is summed.  State: sums fp64 [3][D] = per column sum x, sum x^2 (squared in fp64, exact) and sum fp32((recon - x)^2) (difference
 * and square in fp32, the terms of qsae_sq_err_sum; row 2 is touched only when recon is given), counts int64 [2] = {rows kept, rows skipped}; the caller zeroes both before the first call.
 * Order of every sum: inside a group, row lane r of 16 adds rows r, r + 16, ... in ascending order and the 16 lane sums
 * are added in ascending r; the unflagged groups are then added to the state in ascending group order -- the same bits
 * on every run, and whether the same rows arrive in one call or in several cut at multiples of group_rows.
 * Four columns per thread are read as one vector when D % 4 == 0 and x / recon are 4-element aligned.
 * Errors: QSAE_ERR_INVALID_ARG (B < 0, D < 1, group_rows < 1, null or misaligned pointers), QSAE_ERR_UNSUPPORTED (unknown
 * dtype, D > 16 * 65535) before any HIP call; QSAE_ERR_WORKSPACE.  B == 0: nothing to do, no pointer is looked at.
 * workspace: 8-byte aligned, qsae_dataset_moments_workspace_bytes(B, D, group_rows, with_recon) = the per-group partials
 * (2 or 3) * G * D * 8 and G flag words, each rounded up to 256 bytes, G = ceil(B / group_rows); 0 for an invalid shape. */
size_t qsae_dataset_moments_workspace_bytes(int B, int D, int group_rows, int with_recon);
int qsae_dataset_moments_add(const void* x, int dtype, const float* recon, int B, int D, int group_rows, double* sums,
                             int64_t* counts, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- BinarySAE training: the gradient of the soft-decoder forward (sae/binary.py:24-47, 91-103) ----------------- */
/* Device workspace of qsae_binary_soft_table_polarize (0 for an invalid shape). */
size_t qsae_binary_soft_table_polarize_workspace_bytes(int H, int D);
/* table[h][d] as qsae_binary_soft_table computes it, and *polarize (fp32, device) = mean over [H][D][n_bits] of
 * p (1 - p) 2^b, p = sigmoid(logit): summed in fp64 in a fixed order, divided by H D n_bits in fp64, rounded once --
 * the value BinarySAE.forward reports, without reading anything back to the host. */
int qsae_binary_soft_table_polarize(const float* logits, int H, int D, int n_bits, float* table, float* polarize,
                                    void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* Device workspace of qsae_train_csr (0 for an invalid shape). */
size_t qsae_train_csr_workspace_bytes(int B, int k, int H);
/* The top-k lists idx [B][k] grouped by unit: offsets[H + 1] (int32), entries[B k] = flat index r k + j of every entry
 * of unit h at entries[offsets[h] .. offsets[h + 1]), ordered by row.  O(B k + H B / 32), deterministic. */
int qsae_train_csr(const int32_t* idx, int B, int k, int H, int32_t* offsets, int32_t* entries, void* workspace,
                   size_t workspace_bytes, qsae_stream_t stream);
/* Per selected entry: gv[r][j] = g_latent[r][h] + step * <g_recon[r], table[h]>, h = idx[r][j] (g_recon or g_latent
 * NULL: that term is 0; g_latent is [B][g_latent_ld], ld 0 broadcasts one row); dx (nullable) [B][D] =
 * sum_j gv[r][j] W_enc[h].  D a multiple of 4 up to 4096, k <= 256. */
int qsae_train_row_grad(const int32_t* idx, int B, int k, const float* table, int H, int D, float step,
                        const float* g_recon, const float* g_latent, int64_t g_latent_ld, const float* W_enc, float* gv,
                        float* dx, qsae_stream_t stream);
/* Device workspace of qsae_train_unit_grad (0 for an unsupported shape). */
size_t qsae_train_unit_grad_workspace_bytes(int B, int k, int H, int D);
/* Over each unit's list (qsae_train_csr): dW_enc[h] = sum gv x[r], db_enc[h] = sum gv,
 * dInt[h][d] = step sum val g_recon[r][d], and the logit gradient
 *   dlogits[h][d n + b] = (dInt[h][d] bw[b] + g_polarize 2^b (1 - 2p) / (H D n)) p (1 - p)
 * (g_recon / g_polarize NULL: 0).  Every row of every non-NULL output is written once; lists longer than 256 entries
 * are split into chunks whose partials are added in chunk order.  No float atomics: bitwise reproducible. */
int qsae_train_unit_grad(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B, int k,
                         const float* x, const float* g_recon, const float* logits, int H, int D, int n_bits, float step,
                         const float* g_polarize, float* dW_enc, float* db_enc, float* dlogits, void* workspace,
                         size_t workspace_bytes, qsae_stream_t stream);
/* Device workspace of qsae_train_col_sum. */
size_t qsae_train_col_sum_workspace_bytes(int B, int D);
/* out[d] = sum_r g[r][d] in a fixed order (the decoder-bias gradient). */
int qsae_train_col_sum(const float* g, int B, int D, float* out, void* workspace, size_t workspace_bytes,
                       qsae_stream_t stream);

/* -- BaselineSparseAutoencoder training (sae/baseline.py:17-51; the baseline_sae branch of training/trainer.py:166-173) --- */
/* The baseline SAE's gradient is the one above without the sigmoid chain: qsae_train_row_grad with table =
 * decoder.weight transposed and step = 1, qsae_train_csr, then this call, then qsae_train_col_sum. */
/* Device workspace of qsae_train_table_unit_grad (0 for an unsupported shape: D not a multiple of 4 or over 4096,
 * k > 256, B k >= 2^31). */
size_t qsae_train_table_unit_grad_workspace_bytes(int B, int k, int H, int D);
/* Over each unit's list (qsae_train_csr): dW_enc[h][:] = sum gv x[r], db_enc[h] = sum gv, and column h of the
 * decoder.weight gradient, dW_dec[d][h] = sum val g_recon[r][d], stored in the nn.Linear layout [D][dW_dec_ld]
 * (the sums go to a [H][D] block of the workspace and through a tiled LDS transpose).  Every element of every non-NULL
 * output is written exactly once, units nobody selected included (zeros); g_recon NULL: dW_dec is all zeros.  Lists
 * longer than 256 entries are split into chunks whose partials are added in chunk order, as in qsae_train_unit_grad.
 * No float atomics: bitwise reproducible. */
int qsae_train_table_unit_grad(const int32_t* offsets, const int32_t* entries, const float* val, const float* gv, int B,
                               int k, const float* x, const float* g_recon, int H, int D, float* dW_enc, float* db_enc,
                               float* dW_dec, int64_t dW_dec_ld, void* workspace, size_t workspace_bytes,
                               qsae_stream_t stream);
/* normalize_decoder_weights() in one pass over W [D][H] (decoder.weight, contiguous, 16-byte aligned):
 * norm[h] = sqrt(sum_d W[d][h]^2), squares added for d = 0, 1, .. in fp32 (one fixed chain per column), then in place
 * W[d][h] /= max(norm[h], 1e-8) (a zero column stays zero, a NaN column stays NaN).  table (nullable) [H][D] receives
 * the normalised transpose, the rows the sparse decoder and qsae_train_row_grad gather.  H a multiple of 4, any D. */
int qsae_normalize_columns_table(float* W, int D, int H, float* table, qsae_stream_t stream);

/* -- QuantizedMatryoshkaSAE training: the gradient of the nested-dictionary forward under the straight-through estimators
 *    (sae/quantized_matryoshka.py:47-190; the q_sae / rq_sae branches of training/trainer.py:88-142).  Hidden units are in
 *    the packed order of qsae_pack_matryoshka (every level padded to a multiple of 32); index[slot] (nullable = identity)
 *    is the parameter row of a slot, -1 for an inert pad slot.  No float atomics anywhere: bitwise reproducible. -------- */
/* dst [D][H] = transpose of src [H][D] (fp32, D a multiple of 4, src 16-byte aligned). */
int qsae_transpose_rows(const float* src, int H, int D, float* dst, qsae_stream_t stream);
/* zbits[r][h / 32] bit h % 32 = (sigmoid(pre[r][h]) > 0.5) by the fp32 cutoff every bits path uses (pre >= 0x33C00001):
 * the z bits of a saved pre-activation [B][ld], equal to qsae_encode_bits' on the same operands.  H a multiple of 32, ld a
 * multiple of 4, pre 16-byte aligned. */
int qsae_train_pre_bits(const float* pre, int64_t ld, int B, int H, uint32_t* zbits, int64_t words_ld, qsae_stream_t stream);
/* sign_rows[slot][d] = S = sgn(sigmoid(w) >= .5) + sgn(sigmoid(wm) >= .5) in {-2, 0, 2} as fp32, 0 on pad slots: the
 * K-contiguous dictionary operand of qsae_train_matryoshka_dpre.  H = slots, D a multiple of 4. */
int qsae_train_matryoshka_sign_rows(const float* w, const float* wm, const int32_t* index, int H, int D, float* sign_rows,
                                    qsae_stream_t stream);
/* pre [B][pre_ld] holds the encoder pre-activation on entry and dpre on return:
 *   dpre[r][h] = (scale[h] <g_levels[i][r], sign_rows[h]> + g_groups[i] / B) p (1 - p),  p = sigmoid(pre[r][h]), h in level i
 * on the fp32 matrix pipe (k ascending).  g_levels [n_bits][B][D] / g_groups [n_bits] (device) may be NULL (that term is
 * 0).  level_sizes[n_bits] sum to H, each a multiple of 32; D a multiple of 4 up to 4096; B >= 1. */
int qsae_train_matryoshka_dpre(const float* g_levels, const float* g_groups, const float* sign_rows, const float* scale,
                               int B, int D, int H, int n_bits, const int32_t* level_sizes, float* pre, int64_t pre_ld,
                               qsae_stream_t stream);
/* C[m][n] = sum_k A[k][m] X[k][n], k ascending (one fp32 fmaf chain per element, on the matrix pipe): both operands with
 * the contraction index as the slow axis (A [K][lda], X [K][ldx], C [M][ldc]).  dW_enc = dpre^T x.  M, N, lda, ldx
 * multiples of 4, A and X 16-byte aligned, K >= 1 (any value: the last K slice is zero-filled). */
int qsae_train_gemm_tn(const float* A, int64_t lda, const float* X, int64_t ldx, int K, int M, int N, float* C, int64_t ldc,
                       qsae_stream_t stream);
/* dsum[h][d] = sum over rows r with z bit h set of g_levels[i][r][d] (h in level i), r ascending, as the same TN
 * contraction with A expanded from zbits [B][words_ld]: for dense activations.  Shapes as qsae_train_matryoshka_dpre. */
int qsae_train_matryoshka_dsum_dense(const uint32_t* zbits, int64_t words_ld, const float* g_levels, int B, int D, int H,
                                     int n_bits, const int32_t* level_sizes, float* dsum, qsae_stream_t stream);
/* Device workspace of qsae_train_bits_csr (0 for a refused shape: H not a multiple of 32, B < 1, B * H >= 2^31). */
size_t qsae_train_bits_csr_workspace_bytes(int B, int H);
/* The active rows of every unit from zbits [B][words_ld]: offsets[H + 1] (int32) and, for n_entries > 0,
 * entries[offsets[h] .. offsets[h + 1]) = the rows r whose bit h is set, ascending -- the lists qsae_train_csr builds, from
 * a bit transpose instead of top-k indices.  n_entries = capacity of entries (the batch's active-unit count; positions at or
 * beyond it are not written). */
int qsae_train_bits_csr(const uint32_t* zbits, int64_t words_ld, int B, int H, int32_t* offsets, int32_t* entries,
                        int64_t n_entries, void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* Device workspace of qsae_train_matryoshka_dsum_lists (0 for a refused shape: D not a multiple of 4 or over 4096,
 * n_entries >= 2^31, B < 1). */
size_t qsae_train_matryoshka_dsum_lists_workspace_bytes(int B, int64_t n_entries, int H, int D);
/* dsum as qsae_train_matryoshka_dsum_dense, summed over each unit's list (qsae_train_bits_csr) in list order: for sparse
 * activations.  Units nobody activates get exact zeros.  Lists longer than 256 rows are split into chunks whose partials
 * are added in chunk order. */
int qsae_train_matryoshka_dsum_lists(const int32_t* offsets, const int32_t* entries, int64_t n_entries, const float* g_levels,
                                     int B, int D, int H, int n_bits, const int32_t* level_sizes, float* dsum,
                                     void* workspace, size_t workspace_bytes, qsae_stream_t stream);
/* dweight[u][d] = scale[slot] dsum[slot][d] sw (1 - sw), sw = sigmoid(w[u][d]), u = index[slot]; dweight_mirror likewise
 * from wm: one pass over the two logit tensors.  dsum NULL: zeros.  H = slots. */
int qsae_train_matryoshka_finish(const float* dsum, const float* scale, const int32_t* index, const float* w, const float* wm,
                                 int H, int D, float* dweight, float* dweight_mirror, qsae_stream_t stream);
/* apply_secant_grad(): grad_weight[u][d] -= c counts[slot] scale[slot]^2 Bs sw (1 - sw) in place, Bs = sgn(sigmoid(w) >= .5);
 * the mirror likewise with wm.  counts int64 [H] = active rows per slot (qsae_activation_counts_bits), c = 1 / (B D). */
int qsae_train_matryoshka_secant(const int64_t* counts, float c, const float* scale, const int32_t* index, const float* w,
                                 const float* wm, int H, int D, float* grad_weight, float* grad_weight_mirror,
                                 qsae_stream_t stream);

/* -- TernarySparseAutoencoder training: the gradient of h = relu(x W_enc^T + b), recon = h T^T under the straight-through
 *    estimator of STEWeights, and the RigL mask maintenance of the decoder (sae/ternary.py:27-90,116-122; the t_sae branch
 *    of training/trainer.py:157-164).  w / mask are decoder.weight / decoder.mask [D][H].  No float atomics anywhere:
 *    bitwise reproducible. ------------------------------------------------------------------------------------------ */
/* t_rows [H][D] = the fp32 image of the ternary dictionary, transposed: sign(w[d][h]) (|w[d][h]| >= 0.5), the rule of
 * qsae_pack_ternary.  H a multiple of 4, w 16-byte aligned. */
int qsae_train_ternary_rows(const float* w, int D, int H, float* t_rows, qsae_stream_t stream);
/* dpre[r][h] = (g_latent[r][h] + <g_recon[r], t_rows[h]>) where h_act[r][h] > 0, else 0, on the fp32 matrix pipe (k
 * ascending).  g_recon [B][D] / g_latent [B][H] may be NULL (that term is 0); h_act, g_latent and dpre are [B][H]
 * contiguous and h_act is only read.  D a multiple of 4 up to 4096; B >= 1. */
int qsae_train_ternary_dpre(const float* g_recon, const float* t_rows, const float* g_latent, const float* h_act, int B, int D,
                            int H, float* dpre, qsae_stream_t stream);
/* dweight[d][h] = mask[d][h] sum_r g_recon[r][d] h_act[r][h], r ascending: the TN contraction of qsae_train_gemm_tn with
 * the mask on the store.  D a multiple of 4 up to 4096, H a multiple of 4, B >= 1. */
int qsae_train_ternary_dweight(const float* g_recon, const float* h_act, const float* mask, int B, int D, int H,
                               float* dweight, qsae_stream_t stream);
/* Device workspace of qsae_train_mask_init / qsae_train_mask_update (0 for a refused shape: D * H not below 2^31 or not a
 * multiple of 4). */
size_t qsae_train_mask_workspace_bytes(int D, int H);
/* init_mask: the n_inactive smallest |w| -- exactly that many, ties at the boundary value in ascending flat index d H + h
 * -- get mask 0, every other position mask 1; then w *= mask.  In place, nothing is read back.  0 <= n_inactive <= D H. */
int qsae_train_mask_init(float* w, float* mask, int D, int H, int64_t n_inactive, void* workspace, size_t workspace_bytes,
                         qsae_stream_t stream);
/* update_mask: active = (mask != 0).  Drop (n > 0): thr = the n-th smallest |w| over active positions; every active
 * position with |w| <= thr becomes inactive (n above the active count saturates: all of them drop).  Grow (n > 0, a and
 * delta given): the n largest |delta[d]| * |a[h]| (one fp32 multiply) over the positions inactive after the drop become
 * active -- exactly n, ties in ascending flat index; fewer inactive positions than n: all of them.  Then mask = active and
 * w *= mask, in one pass.  a [H], delta [D] (both NULL: drop only).  In place, nothing is read back.  0 <= n <= D H. */
int qsae_train_mask_update(float* w, float* mask, const float* a, const float* delta, int D, int H, int64_t n,
                           void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- BinaryLatentSAE training: the gradient of pre = x W_e^T + b_e, z = (sigmoid(pre) >= 0.5), recon = z W_d^T + b_d under
 *    the straight-through estimator decode(latent + (binary - latent).detach()) (sae/binary_latent.py:19-27; the bl_sae of
 *    training/trainer.py).  w_dec is decoder.weight [D][H] as nn.Linear keeps it; no transposed copy is made.  The encoder
 *    gradients come from dpre through qsae_train_gemm_tn / qsae_train_col_sum, the decoder bias from qsae_train_col_sum.
 *    All three take H a multiple of 32, B >= 1 and B * H below 2^31; every argument is checked before any HIP call.  No float
 *    atomics anywhere: bitwise reproducible. ------------------------------------------------------------------------- */
/* One pass over pre [B][H] (contiguous, 16-byte aligned): latent[r][h] = pre[r][h] >= cutoff ? 1 : 0 -- the bits of
 * qsae_threshold_ge; NaN gives 0 -- and zbits[r][h / 32] bit h % 32 the same predicate (zbits [B][H / 32], contiguous).
 * latent may be NULL (bits only).  Not the cutoff of qsae_train_pre_bits, which is the > 0.5 of the q_sae paths. */
int qsae_blatent_binarize(const float* pre, int B, int H, float cutoff, float* latent, uint32_t* zbits, qsae_stream_t stream);
/* pre [B][H] (contiguous) holds the encoder pre-activation on entry and dpre on return:
 *   dpre[r][h] = <g_recon[r], w_dec[:, h]> p (1 - p),  p = sigmoid(pre[r][h])
 * on the fp32 matrix pipe (k = d ascending).  g_recon [B][D] is read K-contiguous, w_dec [D][H] in its own layout through
 * the K-slow loader.  D a multiple of 4 up to 4096; g_recon and w_dec 16-byte aligned. */
int qsae_train_blatent_dpre(const float* g_recon, const float* w_dec, int B, int D, int H, float* pre, qsae_stream_t stream);
/* dweight[d][h] = sum over rows r with z bit h set of g_recon[r][d], r ascending: the TN contraction of qsae_train_gemm_tn
 * with the H-side operand expanded from zbits [B][words_ld] (K = B, the last K slice zero-filled), stored straight into the
 * [D][H] layout of decoder.weight.  D a multiple of 4 up to 4096; g_recon 16-byte aligned; words_ld >= H / 32. */
int qsae_train_blatent_dweight(const float* g_recon, const uint32_t* zbits, int64_t words_ld, int B, int D, int H,
                               float* dweight, qsae_stream_t stream);

/* -- Optimizer: the Adam step in one pass.  Per element, every line one IEEE fp32 operation, no
 *    contraction -- the op sequence of torch's single-tensor Adam with amsgrad, maximize and weight decay off:
 *        d = g - m;       m' = m + d * one_minus_b1
 *        a = v * b2;      q = g * g;          v' = a + q * one_minus_b2
 *        s = sqrtf(v');   r = s / bc2_sqrt;   den = r + eps
 *        u = m' / den;    p' = p - step_size * u
 *    The caller computes the scalars in double (step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t), one_minus_b1 =
 *    1 - b1, one_minus_b2 = 1 - b2) and rounds each to fp32 once.  NaN and inf propagate as the operations dictate. -- */
/* p, m, v [n] updated in place from g [n].  16-byte loads when all four pointers are 16-byte aligned, else element-wise;
 * both give the same bits.  n = 0 returns QSAE_OK without a launch, whatever the pointers (an empty tensor's are NULL). */
int qsae_adam_step(float* p, const float* g, float* m, float* v, long long n, float one_minus_b1, float b2,
                   float one_minus_b2, float bc2_sqrt, float eps, float step_size, qsae_stream_t stream);
/* The same step on the encoder weight W [H][D] and (all four non-NULL, or all four NULL) its bias [H], leaving Wq (fp16
 * [H][D]) and meta (4 device floats) bit-identical to what qsae_prefilter_pack_w(W', bias', H, D, Wq, meta) writes for the
 * updated values.  W and Wq 16-byte aligned.  No workspace: meta[0] carries max |W'| between the launches of the call. */
int qsae_adam_step_prefilter(float* W, const float* gW, float* mW, float* vW, float* bias, const float* gb, float* mb,
                             float* vb, int H, int D, float one_minus_b1, float b2, float one_minus_b2, float bc2_sqrt,
                             float eps, float step_size, void* Wq, float* meta, qsae_stream_t stream);

/* -- Trainer: what the epoch loop does around forward_train (training/trainer.py:73-173).  src is a
 *    chunk of hidden states [n_rows][D], contiguous, dtype 0 = fp32, 1 = fp16, 2 = bf16 (the codes of
 *    qsae_dataset_moments_add).  Invalid arguments are answered before any HIP call; no float atomics: the same bits on
 *    every run. --------------------------------------------------------------------------------------------------------- */
/* bits uint32 [ceil(n_rows / 32)], every word written once: bit r % 32 of word r / 32 is set where row r holds a NaN (tested
 * on the stored bits; inf does not count), the bits past n_rows are 0.  One pass over the chunk, 16-byte loads when src is
 * 16-byte aligned and a row is a whole number of 16-byte pieces.  Replaces `torch.isnan(batch).any()` per step
 * (trainer.py:84): built once per chunk, read once per chunk.  n_rows == 0: QSAE_OK without a launch, whatever the pointers.
 * Errors: QSAE_ERR_INVALID_ARG (n_rows < 0, D < 1, null or misaligned pointers), QSAE_ERR_UNSUPPORTED (unknown dtype,
 * n_rows > 32 * (2^31 - 1)). */
int qsae_rows_nan_bitmap(const void* src, int dtype, int64_t n_rows, int D, uint32_t* bits, qsae_stream_t stream);
/* out[b][:] = float(src[idx[b]][:]) for b < B: idx int64 [B] and out fp32 [B][D] on the device.  The widening is exact, so
 * out has the bits of the reference's `.float()` (data/dataset.py:32) for every value that is not a NaN; fp32 rows are
 * copied, a bf16 NaN keeps sign and payload, an fp16 NaN keeps them when it is quiet (the hardware conversion quiets a
 * signalling one; torch's CPU `.float()` maps every fp16 NaN to one pattern of its own).  Batches with a NaN are skipped by
 * the loop, so no such value reaches a model.  An index outside [0, n_rows)
 * is never dereferenced: its row is written as zeros and bit 0 of *flag (uint32, device, zeroed by the caller) is set
 * through an integer atomic.  16-byte loads and stores when src and out are 16-byte aligned and a source row is a whole
 * number of 16-byte pieces (D % 4 == 0 for fp32, D % 8 == 0 for the 16-bit types), element by element otherwise.
 * B == 0: QSAE_OK without a launch, whatever the pointers.  src may be NULL only when n_rows == 0. */
int qsae_gather_rows(const void* src, int dtype, int64_t n_rows, int D, const int64_t* idx, int B, float* out, uint32_t* flag,
                     qsae_stream_t stream);
/* The reconstruction losses of n <= 8 levels and their gradients in one pass (the per-type recipes of trainer.py:88-173).
 * x, every recon_ptrs[i] and every grads_ptrs[i] are fp32 [B][D], contiguous; recon_ptrs / grads_ptrs are HOST arrays of n
 * device pointers.  mode 0: the target of every level is t_i = x.  mode 1 (rq_sae): t_0 = x, t_{i+1} = fl(fl(t_i - r_i) * 2),
 * the arithmetic of qsae_residual_update.  With N = B D and s = fp32(2 coef / N) formed in double:
 *   grads_ptrs[i][e] = fl(fl(r_i[e] - t_i[e]) * s)
 *   losses[i] (fp32, device) = fp32((coef * S_i) / N), both operations in fp64, S_i = the fp64 sum of fp32(fl(r_i[e] - t_i[e])^2)
 * Order of S_i: workgroup b owns the elements [4096 b, 4096 (b + 1)) in 4 slabs of 1024; thread t of 256 adds the elements
 * 4 t .. 4 t + 3 of slab 0, then of slab 1, ...; the 64 lane sums of a wave are joined by a butterfly (xor 32, 16, ..., 1),
 * the 4 wave sums added in ascending order; then thread t of one workgroup per level adds the workgroup sums t, t + 256, ...
 * in ascending order and the 256 thread sums are joined the same way.  x and every r_i are read once; nothing of size
 * [B][D] is written other than the gradients.  16-byte loads and stores when all 2 n + 1 pointers are 16-byte aligned,
 * scalar ones otherwise: the same bits.  n == 0 or B == 0: QSAE_OK without a launch, nothing written.
 * Errors: QSAE_ERR_INVALID_ARG (negative n or B, D < 1, null or misaligned pointers), QSAE_ERR_UNSUPPORTED (n > 8, unknown
 * mode, B D above 4096 * (2^31 - 1)), QSAE_ERR_WORKSPACE.  workspace: 8-byte aligned,
 * qsae_trainer_loss_workspace_bytes(n, B, D) = n * ceil(B D / 4096) * 8 rounded up to 256 (0 for an invalid shape). */
size_t qsae_trainer_loss_workspace_bytes(int n, int B, int D);
int qsae_trainer_loss(const float* x, const float* const* recon_ptrs, int n, int B, int D, int mode, double coef,
                      float* const* grads_ptrs, float* losses, void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- Watch: the distributions of T tensors in one call (what `wandb.watch(model, log="all")` logs of every parameter and
 *    gradient).  ptrs and counts are HOST arrays of T device pointers and element counts (fp32,
 *    contiguous, any sizes, 4-byte aligned; a tensor off its 16-byte boundary is read with scalar loads and gives the same
 *    bits).  result (device, 8-byte aligned) holds T blocks of QSAE_TENSOR_STATS_HEAD + bins 8-byte words:
 *      0 lo, 1 hi   the minimum and maximum of the finite elements as fp64 (exact images of the fp32 values; a zero is +0.0)
 *      2 mean, 3 m2 fp64 over the finite elements: S / n_finite and the sum of (x - mean)^2 (std = sqrt(m2 / (n_finite - 1)))
 *      4 n_finite, 5 n_nonfinite, 6 n_zero (+-0.0), 7 zero   int64
 *      8 ..         counts int64 [bins]: torch.histc(finite elements, bins, lo, hi) as the CPU computes it in fp32,
 *                   q = ((x - lo) * float(bins)) / (hi - lo), bin = int(q) with bin == bins folded into bins - 1.  lo == hi:
 *                   the range is widened as torch does (lo - 1 and hi + 1, or the neighbouring floats where those round
 *                   back), so everything lands in bin bins / 2 for |lo| < 2^24.  hi - lo overflows: all counts 0, as in torch.
 *    A tensor with no element or no finite element has n_finite = 0, zero counts and zeros in words 0 .. 3.
 *    Two streaming passes and two joins; fp64 sums in a fixed order (per-thread chains in ascending index over chunks of
 *    8192 elements, a butterfly, chunk partials in ascending order), counts through integer atomics, no float atomics: the
 *    same bits on every run.  Nothing is read back.
 *    T == 0 or every count 0: QSAE_OK with nothing launched and nothing written.
 *    Errors, all before any launch: QSAE_ERR_INVALID_ARG (T < 0, a negative count, a null or misaligned tensor pointer with
 *    a non-zero count, bins outside 1 .. 256, null or misaligned result), QSAE_ERR_UNSUPPORTED (dtype other than 0 = fp32,
 *    T > 65536, a tensor above 2^40 elements, more than 2^30 chunks in all), QSAE_ERR_WORKSPACE.  workspace: 8-byte aligned,
 *    qsae_tensor_stats_workspace_bytes(counts, T) = 32 bytes per chunk and 24 per tensor, in seven arrays of 256-byte
 *    pieces (0 where there is nothing to do or the counts are not taken). ------------------------------------------------------------------------ */
#define QSAE_TENSOR_STATS_HEAD 8
size_t qsae_tensor_stats_workspace_bytes(const int64_t* counts, int T);
int qsae_tensor_stats(const void* const* ptrs, const int64_t* counts, int T, int dtype, int bins, void* result,
                      void* workspace, size_t workspace_bytes, qsae_stream_t stream);

/* -- Activity: which units of the dictionary are alive while a model trains.  The reference's
 *    one_epoch takes a dead_neuron_threshold that nothing reads and a `latents` list it never fills (training/trainer.py:66-78).
 *    State per tracker, on the device, 8-byte aligned, zeroed by the caller before the first call:
 *      fired int64 [H]  rows in which the unit was active, over the run
 *      last  int64 [H]  the stamp of the last batch in which it was active, 0 = never
 *      base  int64 [H]  fired as of the previous summary
 *    "Active" is the reference's activation mask (scripts/analysis/dynamic_analysis.py:30-73), as in qsae_activation_counts*.
 *    A batch carries a stamp >= 1 (the caller's clock after the batch: rows seen so far); every unit active in at least one
 *    of its rows gets last[u] = max(last[u], stamp), so a stamp out of order never lowers it, and fired[u] += its active rows.
 *    Both go through 64-bit integer atomics (atomicAdd / atomicMax), which do not depend on order: the same bits on every
 *    run.  fired[u] and last[u] of a unit that is active in no row of the batch are not written.  No float atomics.
 *    B == 0: QSAE_OK with nothing launched and no device needed.  Errors, all before any launch: QSAE_ERR_INVALID_ARG (null or
 *    misaligned pointers, B < 0, k < 1, nbits < 1, H <= 0, stamp < 1, ld < H, words_ld < nbits / 32, index == NULL with
 *    nbits > H), QSAE_ERR_UNSUPPORTED (nbits % 32 != 0, B * k >= 2^31). ----------------------------------------------------- */
/* Compact form of the top-k models: entry (b, idx[b][j]) is active iff val[b][j] > 0 (NaN, 0.0 and -0.0 are not; val == NULL:
 * every entry).  Indices outside [0, H) are dropped; a unit listed twice in one row counts twice in fired, as in
 * qsae_activation_counts.  One pass over the B k entries counts and stamps. */
int qsae_activity_add_compact(const int32_t* idx, const float* val, int B, int k, int H, int64_t stamp, int64_t* fired,
                              int64_t* last, qsae_stream_t stream);
/* Packed bits of the threshold models: zbits uint32 [B][words_ld], bit j of word w = packed position 32 w + j (the layout of
 * qsae_activation_counts_bits, whose column popcounts this repeats).  index int32 [nbits] (device) maps a packed position to
 * its unit, -1 = pad slot: ignored, its bits need not be zero; values >= H are dropped; index == NULL: identity, requires
 * nbits <= H.  Two positions that map to one unit are the caller's duty, as in qsae_coactivation_bits. */
int qsae_activity_add_bits(const uint32_t* zbits, int64_t words_ld, int B, int nbits, const int32_t* index, int H, int64_t stamp,
                           int64_t* fired, int64_t* last, qsae_stream_t stream);
/* Dense latent fp32 [B][ld] (the ternary model's h): active iff latent > 0 (NaN no, +inf yes, positive denormals yes).
 * Rows are read coalesced (16 bytes per lane when latent is 16-byte aligned and ld % 4 == 0, scalar loads otherwise: the
 * same counts); a thread counts its columns over the rows of its workgroup and only non-zero counts reach memory. */
int qsae_activity_add_dense(const float* latent, int64_t ld, int B, int H, int64_t stamp, int64_t* fired, int64_t* last,
                            qsae_stream_t stream);
/* The summary of a tracker at `clock` (>= 0: the rows added so far) with a window of `window` >= 1 rows:
 *   dead    clock - last[u] >= window (a unit that never fired becomes dead once clock >= window; before that nothing is)
 *   never   last[u] == 0
 *   silent  fired[u] == base[u]: nothing since the previous summary;  interval count c = fired[u] - base[u] (base <= fired is
 *           the caller's duty; base == NULL reads as zeros)
 *   octave  bit length of c: bin 0 holds c == 0, bin b holds 2^(b-1) <= c < 2^b, bins above 33 are folded into 33
 * result (device, 8-byte aligned) receives (1 + n_seg) blocks of QSAE_ACTIVITY_HEAD + QSAE_ACTIVITY_BINS int64: block 0 over
 * all units, block s over segment s - 1 of seg_sizes (HOST array of n_seg <= QSAE_ACTIVITY_MAX_SEGMENTS sizes >= 0 that add
 * up to H: consecutive slices of the units; NULL or n_seg == 0: block 0 alone).  Head words: 0 units, 1 never, 2 dead,
 * 3 silent, 4 the sum of the interval counts, 5 the sum of fired, 6 the largest interval count, 7 zero; then the octave bins.
 * advance != 0 writes base[u] = fired[u], in the thread that read both.  dead_out int32 [H] (NULL: no list) receives the dead
 * units in ascending order in [0, result[2]); the rest is left untouched.  The list is placed by prefix counts, never by an
 * atomic cursor: the same bits on every run (the rule of qsae_token_lists_*).  Nothing is read back.
 * Errors, all before any launch: QSAE_ERR_INVALID_ARG (H <= 0, clock < 0, window < 1, null or misaligned fired / last /
 * result, misaligned base / dead_out, n_seg outside 0 .. 16, n_seg > 0 without seg_sizes, a negative size, sizes that do not
 * add up to H), QSAE_ERR_WORKSPACE.  workspace: 8-byte aligned, qsae_activity_summary_workspace_bytes(H) = 4 bytes per chunk
 * of 1024 units rounded up to 256 (0 for H <= 0); it need not be zeroed. */
#define QSAE_ACTIVITY_HEAD 8
#define QSAE_ACTIVITY_BINS 34
#define QSAE_ACTIVITY_MAX_SEGMENTS 16
size_t qsae_activity_summary_workspace_bytes(int H);
int qsae_activity_summary(const int64_t* fired, int64_t* base, const int64_t* last, int H, int64_t clock, int64_t window,
                          const int32_t* seg_sizes, int n_seg, int advance, int64_t* result, int32_t* dead_out, void* workspace,
                          size_t workspace_bytes, qsae_stream_t stream);

/* -- Resampling: revive the dead units of a top-k dictionary from the rows it reconstructs worst,
 *    the consumer of qsae_activity_summary's dead list.  Five steps, each an entry point, chained on the device with no
 *    host read: row weights, the draw, the statistics of the alive units, and one of two writes.  Every floating-point sum
 *    is an fp64 sum in a fixed order (csrc/resample.hip states the two orders, tests/resample_util.py mirrors them); counts
 *    go through 64-bit integer atomicAdd, the owner of a row through 32-bit integer atomicMin: the same bits on every run.
 *    No float atomics.  D: a multiple of 4 up to QSAE_RESAMPLE_MAX_D (QSAE_ERR_UNSUPPORTED otherwise).  All argument
 *    errors are raised before any launch. ----------------------------------------------------------------------------------- */
#define QSAE_RESAMPLE_MAX_D 4096
/* int64 words of a report: 0 dead (n), 1 revived, 2 duplicate (the row has an earlier owner), 3 degenerate (the row equals
 * the decoder bias, or its norm is not finite), 4 no_weight (the total weight is 0 or not finite), 5 entries of the dead
 * list or of rows that were out of range or out of order and therefore skipped, 6 and 7 zero. */
#define QSAE_RESAMPLE_REPORT_WORDS 8
/* w[r] = e_r e_r with e_r = sum over d of (x[r][d] - recon[r][d])^2: the difference is one fp32 subtraction, widened
 * exactly, squared and summed in fp64; w[r] = 0 where e_r is not finite.  x fp32 [N][ldx], recon fp32 [N][ldr], w fp64 [N].
 * N == 0: QSAE_OK with nothing launched. */
int qsae_resample_row_weights(const float* x, int64_t ldx, const float* recon, int64_t ldr, int N, int D, double* w,
                              qsae_stream_t stream);
/* The draw: cdf = the inclusive fixed-order prefix sum of w (non-negative, finite: the caller's duty), total = cdf[N - 1].
 * Dead unit j takes t_j = u[j] total (u fp64 [n] in [0, 1)) and r_j = the smallest r with cdf[r] > t_j, by binary search
 * (a u outside [0, 1) or a NaN: the row at which the cdf reaches the total); a row of weight 0 is never drawn.  The
 * first drawer of a row (lowest j) owns it.  rows int32 [n]: r_j for the owner, -2 for a later drawer of the same row, -1
 * when total is 0 or not finite.  report (QSAE_RESAMPLE_REPORT_WORDS int64) is zeroed and receives words 0, 2 and 4.
 * n == 0: QSAE_OK with nothing launched and nothing written.  workspace: 8-byte aligned, need not be zeroed,
 * qsae_resample_draw_workspace_bytes(N) = 8 N, 8 per chunk of 1024 rows and 4 N bytes, each rounded up to 256 (0 for N <= 0).
 * Errors: QSAE_ERR_INVALID_ARG (N < 1, n < 0, null or misaligned pointers), QSAE_ERR_WORKSPACE. */
size_t qsae_resample_draw_workspace_bytes(int N);
int qsae_resample_draw(const double* w, int N, const double* u, int n, int32_t* rows, int64_t* report, void* workspace,
                       size_t workspace_bytes, qsae_stream_t stream);
/* stats[0] = enc_norm_mean: the mean over the alive units (those not in the ascending list dead int32 [n]; every unit when
 * none is alive) of sqrt(sum over d of W_enc[h][d]^2); stats[1] = logit_mean: the mean of |logits[h][c]| over the same rows
 * of logits fp32 [H][D n_bits] (NULL: stats[1] = 0, n_bits and unit_abs are not looked at).  unit_norm / unit_abs fp64 [H]
 * receive the per-unit root and sum.  Errors: QSAE_ERR_INVALID_ARG (H or D <= 0, n outside 0 .. H, n_bits outside 1 .. 8,
 * null or misaligned pointers, logits without unit_abs). */
int qsae_resample_alive_stats(const float* W_enc, int H, int D, const float* logits, int n_bits, const int32_t* dead, int n,
                              double* unit_norm, double* unit_abs, double* stats, qsae_stream_t stream);
/* The write, one workgroup per dead unit j with h = dead[j] and r = rows[j] >= 0 (negative: nothing is done):
 *   v_d = x[r][d] - dec_bias[d] (fp32), s = sum v_d^2 (fp64), nrm = sqrt(s); s == 0 or not finite: the unit is left untouched
 *   and counted as degenerate;  W_enc[h][d] = fp32(fp64(v_d) c) with c = (encoder_scale stats[0]) / nrm;  b_enc[h] = 0;
 *   table form (BaselineSparseAutoencoder, dec fp32 [D][H]): dec[d][h] = fp32(fp64(v_d) / nrm);
 *   binary form (BinarySAE, dec fp32 [H][D n_bits], bit b of dimension d at column d n_bits + b, LSB first, MSB negative):
 *     q_d = clamp(rint(fp64(v_d) (max(qmax, 1) / fp64(max_d |v_d|))), -2^(n_bits-1), qmax), qmax = 2^(n_bits-1) - 1; the logit
 *     is +L where bit b of q_d & (2^n_bits - 1) is set and -L elsewhere, L = fp32(logit_scale) when has_logit_scale, else
 *     fp32(stats[1]).
 * The Adam moments m_* / v_* (shapes of W_enc, b_enc, dec; each may be NULL) are set to 0 at exactly the written positions;
 * last (int64 [H], may be NULL) receives last[h] = rows_seen.  report gains words 1, 3 and 5.  An entry with dead[j] outside
 * [0, H), dead[j] <= dead[j - 1] or rows[j] >= N is skipped and counted in word 5, never written through.
 * n == 0: QSAE_OK with nothing launched.  Errors: QSAE_ERR_INVALID_ARG (n < 0, n > H, N < 1, H or D <= 0, ldx < D,
 * rows_seen < 0, n_bits outside 1 .. 8, null or misaligned pointers), QSAE_ERR_UNSUPPORTED (D, n > 65536). */
int qsae_resample_write_table(const int32_t* dead, const int32_t* rows, int n, const float* x, int64_t ldx, int N, int D, int H,
                              const float* dec_bias, const double* stats, double encoder_scale, float* W_enc, float* b_enc,
                              float* dec, float* m_We, float* v_We, float* m_be, float* v_be, float* m_dec, float* v_dec,
                              int64_t* last, int64_t rows_seen, int64_t* report, qsae_stream_t stream);
int qsae_resample_write_binary(const int32_t* dead, const int32_t* rows, int n, const float* x, int64_t ldx, int N, int D, int H,
                               int n_bits, const float* dec_bias, const double* stats, double encoder_scale, int has_logit_scale,
                               double logit_scale, float* W_enc, float* b_enc, float* dec, float* m_We, float* v_We, float* m_be,
                               float* v_be, float* m_dec, float* v_dec, int64_t* last, int64_t rows_seen, int64_t* report,
                               qsae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* QSAE_H */
