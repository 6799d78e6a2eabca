"""BinarySAE: fp32 encoder, top-k mask, n-bit two's-complement dictionary
(reference: sae/binary.py:10-103)."""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from .. import torch_ops as ops          # torch.ops.qsae.* (dispatcher ops over the C ABI)
from .base import HipEncoder, PackedCache, SparseAutoencoder, as_f32c, require_device_input
from .topk import SubmittedForward, TopKCore, sparse_backward


class binary_decoder(nn.Module):
    """Dictionary stored as per-bit logits ``weight[h, d*n_bits + b]`` (bit b of output d, LSB
    first, MSB weight negative), ``bias[d]`` (sae/binary.py:11-22).

    The reference forward multiplies the latent with the *soft* integers ``sum_b sigmoid(w_b) bw_b``
    (sae/binary.py:26-38); the *hard* two's-complement integers (``sigmoid(w) > 0.5``,
    ``quantized_int_weights()``, sae/binary.py:49-58) are what a trained, polarised checkpoint converges to
    and what the packed n-bit dictionary holds.  Which of the two a forward uses is decided when the
    dictionary is packed, from a number the packer measures on the way:

        soft_gap = max over (h, d) of |soft integer - hard integer|        (qsae_pack_binary)

    ``decode_mode``:
      * ``"auto"`` (default) -- hard packed decode when ``soft_gap <= hard_max_gap * (2^n_bits - 1)`` (1e-7 of the
        integer range: every logit beyond about +-16.2, whatever n_bits; reconstructions then equal the reference's to
        ~1e-6 relative), otherwise the reference's soft
        arithmetic over an fp32 ``[H, D]`` table (a warning says so once per checkpoint);
      * ``"hard"`` -- always the packed integers (the deployment form; differs from the reference forward
        on an unpolarised checkpoint by up to tens of percent, see scripts/evaluation/estimate_quantization_error.py);
      * ``"soft"`` -- always the soft table.
    """

    #: auto mode: largest |soft - hard|, as a fraction of the integer range 2^n_bits - 1 (a per-bit saturation measure:
    #: the gap of a dictionary whose logits all sit at +-L is (2^n_bits - 1) sigmoid(-L)), for which the hard decode
    #: stands in for the soft one
    hard_max_gap = 1e-7

    def hard_gap_limit(self) -> float:
        return self.hard_max_gap * float(2 ** self.n_bits - 1)

    def __init__(self, in_features, out_features, gamma=4.0, n_bits=8):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.n_bits = n_bits
        self.scale_factor = 2 ** n_bits
        self.gamma = gamma
        self.quantization_step = gamma / (2 ** (n_bits - 1))
        self.weight = nn.Parameter(torch.empty(in_features, out_features * n_bits))
        self.bias = nn.Parameter(torch.zeros(out_features))
        nn.init.kaiming_normal_(self.weight)
        self.decode_mode = "auto"
        self._cache = PackedCache()

    # -- packed state -------------------------------------------------------------------------
    def packed(self) -> dict:
        """{'packed': uint8 [H,row_bytes], 'polarize': fp32 0-d, 'soft_gap': float, ['soft_table': fp32 [H,D]]}"""
        def build():
            w = require_device_input(self.weight.detach(), "decoder.weight")
            packed, pol, gap = ops.pack_binary(w, self.out_features, self.n_bits, want_soft_gap=True)
            polarize = (pol / float(w.numel())).to(torch.float32)
            return {"packed": packed, "polarize": polarize, "soft_gap": float(gap)}   # one host read per checkpoint
        return self._cache.get((self.weight,), build)

    def invalidate_packed(self) -> None:
        """Forget the packed dictionary.  Needed only after an in-place edit THROUGH ``.data`` (``w.data.mul_()``),
        which bumps no version counter; ``load_state_dict``, ``.to()``, optimizer steps and ``no_grad`` in-place ops
        on the parameter itself are noticed automatically."""
        self._cache.clear()

    def soft_table(self) -> torch.Tensor:
        st = self.packed()
        if "soft_table" not in st:
            st["soft_table"] = ops.binary_soft_table(self.weight.detach(), self.out_features, self.n_bits)
        return st["soft_table"]

    def resolved_decode_mode(self) -> str:
        """"hard" or "soft": what decode_mode means for the current weights."""
        mode = self.decode_mode
        if mode in ("hard", "soft"):
            return mode
        if mode != "auto":
            raise ValueError(f"decode_mode must be 'auto', 'hard' or 'soft', got {mode!r}")
        st = self.packed()
        if st["soft_gap"] <= self.hard_gap_limit():
            return "hard"
        if not st.get("warned"):
            st["warned"] = True
            warnings.warn(
                f"binary_decoder: checkpoint is not polarised (max |soft - hard| integer gap {st['soft_gap']:.3g} > "
                f"{self.hard_gap_limit():g}); decoding with the reference's soft sigmoid-bit table (sae/binary.py:26-38). "
                "Set decode_mode='hard' for the packed two's-complement dictionary.", stacklevel=3)
        return "soft"

    # -- sparse decode (the hot path) -----------------------------------------------------------
    def decode_sparse(self, idx: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
        if self.resolved_decode_mode() == "soft":
            return ops.decode_table_sparse(idx, val, self.soft_table(), self.quantization_step, self.bias.detach())
        return ops.decode_binary_sparse(idx, val, self.packed()["packed"], self.out_features, self.n_bits,
                                        self.quantization_step, self.bias.detach())

    # -- reference-compatible dense entry point ---------------------------------------------------
    def forward(self, latent, true_sum=None):
        """(reconstruction, polarize_loss) for an arbitrary dense latent [B, H]
        (sae/binary.py:24-47; ``true_sum`` is ignored there as well)."""
        with torch.no_grad():
            latent = require_device_input(latent, "latent")
            st = self.packed()
            table = self.soft_table() if self.resolved_decode_mode() == "soft" else self._int_table()
            acc = ops.encode_dense(latent, table.t().contiguous(), None, ops.ACT_NONE)
            recon = ops.scale_bias_rows(acc, self.quantization_step, self.bias.detach())
            return recon, st["polarize"]

    def _int_table(self) -> torch.Tensor:
        return ops.unpack_binary(self.packed()["packed"], self.out_features, self.n_bits)

    def quantized_int_weights(self):
        """Two's-complement integer weights [H, D] as fp32 (sae/binary.py:49-58)."""
        with torch.no_grad():
            return self._int_table()

    def quantized_int_weights_continuous(self):
        """Soft (sigmoid-bit) integer weights [H, D] (sae/binary.py:60-69)."""
        with torch.no_grad():
            return ops.binary_soft_table(self.weight.detach(), self.out_features, self.n_bits)


class BinarySAE(ops.GraphForwardMixin, TopKCore, SparseAutoencoder):
    """``forward(x) -> (sparse_latent [B,H], reconstruction [B,D], polarize_loss [])``
    (sae/binary.py:71-103).  k = int(hidden_dim * self.k) with self.k = 0.002.

    Shape limits of the kernels (checked before every forward's first launch, ValueError): k <= 256, input_dim and
    hidden_dim multiples of 4, hidden_dim <= 32768 for batches under 2048 rows and the in-place path, <= 65536 otherwise; ``latent_path = "slabs"`` goes up to 2^20 at any batch
    (k <= 256 stays: past 128499 units lower ``self.k``).  k == 0 (hidden_dim < 500) is served like the reference: an
    all-zero latent and a bias-only reconstruction."""

    def __init__(self, input_dim, hidden_dim, gamma=4.0, n_bits=8):
        super().__init__(input_dim, hidden_dim)
        self.n_bits = n_bits
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.k = 0.002
        lin = nn.Linear(input_dim, hidden_dim)
        nn.init.xavier_uniform_(lin.weight, gain=1)
        nn.init.zeros_(lin.bias)
        self.encoder = HipEncoder(lin)
        self.decoder = binary_decoder(hidden_dim, input_dim, gamma=gamma, n_bits=self.n_bits)
        self._init_topk()
        #: the soft table of the last forward_train, keyed on the logits' version: forward_aux decodes from it
        self._train_cache = PackedCache()
        ops.module_handle(self)

    @property
    def top_k(self) -> int:
        return int(self.hidden_dim * self.k)

    #: a ``training.FeatureActivity`` or None: when set, ``forward_train`` (never ``forward``) adds every batch's active units
    #: to it from the tensors it already holds; outputs and gradients are the same bits either way
    activity = None
    #: "auto" | "fused" | "inplace" | "prefilter".  fused: exact-fp32 encoder+top-k without a dense
    #: latent in HBM (the dense [B,H] return value is zero-filled inside the sweep); inplace: dense
    #: contraction, top-k masks it in place; prefilter: an fp16 MFMA pass with a rigorous error bound
    #: picks ~90 candidates per row, which are re-evaluated and ranked in exact fp32.  All paths return
    #: bit-identical outputs; auto takes prefilter for large batches (fused where its shape limits do not
    #: hold) and inplace for small ones.  "slabs" (never chosen by auto): the selection over ``slab_width`` hidden units at
    #: a time, merged on the device -- the same bits again, and the one path for hidden_dim above 65536 (above 32768 for
    #: batches under 2048 rows), up to 2^20; it decodes with the separate sparse decoders.
    latent_path = "auto"
    #: prefilter path: the refinement kernel also decodes each row it has ranked (one launch less, the decode's work in
    #: the refinement's idle issue slots); False = separate decode kernel.  Bit-identical either way.
    fuse_decode = True

    def resolved_latent_path(self, batch_rows: int) -> str:
        """Which path forward() takes for a batch of this many rows (after the auto / shape fallbacks)."""
        path = self.latent_path
        if path not in ("auto", "fused", "inplace", "prefilter", "slabs"):
            raise ValueError(f"latent_path must be 'auto', 'fused', 'inplace', 'prefilter' or 'slabs', got {path!r}")
        if path == "slabs":                     # opt-in only: "auto" never resolves to it
            return path
        big = batch_rows >= 2048 and self.hidden_dim >= 8192
        if path == "auto":
            path = "prefilter" if big else "inplace"
        if path == "prefilter" and not ops.prefilter_supported(batch_rows, self.input_dim, self.hidden_dim, self.top_k):
            path = "fused" if big else "inplace"
        return path

    def invalidate_packed(self) -> None:
        """Forget every derived copy of the weights (packed dictionary, fp16 / K-interleaved encoder copies); see
        binary_decoder.invalidate_packed."""
        self.decoder.invalidate_packed()
        self._train_cache.clear()
        self._clear_encoder_copies()

    def _check_limits(self, path: str, rows: int) -> None:
        k = self.top_k
        if k > 256:
            raise ValueError(f"BinarySAE: top-k = int({self.hidden_dim} * {self.k}) = {k} exceeds the kernels' limit of 256 "
                             "(on every path, latent_path = 'slabs' included: lower model.k)")
        if path == "slabs":
            if not self._slabs_supported(rows, k):
                raise ValueError(f"BinarySAE: the slab selection does not take input_dim = {self.input_dim}, hidden_dim = "
                                 f"{self.hidden_dim}, top-k = {k} at slab_width = {self.slab_width} (input_dim and hidden_dim "
                                 "multiples of 4, hidden_dim <= 2^20, slab_width a multiple of 256 up to 32768, at most 32 "
                                 "slabs of at least top-k units)")
            return
        if self.hidden_dim > 32768 and path == "inplace":
            raise ValueError(f"BinarySAE: hidden_dim = {self.hidden_dim} exceeds the in-place top-k kernel's limit of 32768 "
                             "(batches of >= 2048 rows take the fused path up to 65536; latent_path = 'slabs' takes wider "
                             "dictionaries at any batch)")
        if not ops.encode_topk_supported(max(rows, 1), self.input_dim, self.hidden_dim, k):
            raise ValueError(f"BinarySAE: no top-k path takes input_dim = {self.input_dim}, hidden_dim = {self.hidden_dim} at "
                             f"a batch of {rows} rows (input_dim and hidden_dim multiples of 4; hidden_dim <= 32768, or up "
                             "to 65536 for batches of >= 2048 rows; latent_path = 'slabs' takes wider dictionaries)")

    def _zero_k(self, x, want_dense: bool):
        """k == 0: the reference's topk(0) keeps nothing -- zero latent, reconstruction = decoder bias (sae/binary.py:94-99)."""
        B = x.shape[0]
        latent = torch.zeros((B, self.hidden_dim), dtype=torch.float32, device=x.device) if want_dense else None
        recon = self.decoder.bias.detach().to(torch.float32).expand(B, -1).contiguous()
        idx = torch.empty((B, 0), dtype=torch.int32, device=x.device)
        val = torch.empty((B, 0), dtype=torch.float32, device=x.device)
        return idx, val, latent, recon

    def _run(self, x, want_dense: bool, soft_table=None):
        """-> (idx, val, dense latent or None, reconstruction): the one implementation behind forward(),
        forward_compact() and forward_train().  soft_table: decode with this fp32 [H, D] table of soft integers (the
        reference's arithmetic) instead of what decoder.decode_mode resolves to."""
        x = require_device_input(x, "x")
        if self.top_k == 0:
            return self._zero_k(x, want_dense)
        path = self.resolved_latent_path(x.shape[0])
        self._check_limits(path, x.shape[0])
        dec = self.decoder
        hard = soft_table is None and dec.resolved_decode_mode() == "hard"
        if path == "prefilter" and self.fuse_decode:
            enc = self._prefilter_operands(x)
            return self._forward_prefilter(enc, self.top_k, self._fused_decoder(hard, soft_table), dec.bias.detach(),
                                           want_dense)
        idx, val, latent = self._select(x, self.top_k, path, want_dense)
        if soft_table is not None:
            return idx, val, latent, ops.decode_table_sparse(idx, val, soft_table, dec.quantization_step, dec.bias.detach())
        return idx, val, latent, dec.decode_sparse(idx, val)

    def _fused_decoder(self, hard: bool, soft_table=None):
        """What the refinement kernel decodes every row it ranks from: the packed n-bit dictionary, or the fp32
        soft-integer table when the checkpoint is not polarised (the reference's own arithmetic)."""
        dec = self.decoder
        if hard:
            return "packed", dec.packed()["packed"], dec.n_bits, dec.quantization_step
        return "table", dec.soft_table() if soft_table is None else soft_table, dec.quantization_step

    def _graph_params(self):
        lin, dec = self.encoder.linear, self.decoder
        return [lin.weight, lin.bias, dec.weight, dec.bias]

    def forward_compact(self, x):
        """(idx int32 [B,k], val fp32 [B,k], reconstruction [B,D]) without the dense latent; same path
        selection (and the same bits) as forward()."""
        with torch.no_grad():
            if torch.compiler.is_compiling():          # one graph node: torch.ops.qsae.binary_sae_forward
                idx, val, _, recon, _ = torch.ops.qsae.binary_sae_forward(x, self._graph_params(), self._qsae_handle, False)
                return idx, val, recon
            idx, val, _, recon = self._run(x, want_dense=False)
            return idx, val, recon

    def forward(self, x):
        with torch.no_grad():
            if torch.compiler.is_compiling():          # one graph node: torch.ops.qsae.binary_sae_forward
                _, _, latent, recon, pol = torch.ops.qsae.binary_sae_forward(x, self._graph_params(), self._qsae_handle, True)
                return latent, recon, pol
            _, _, latent, recon = self._run(x, want_dense=True)
            return latent, recon, self.decoder.packed()["polarize"]

    # -- training -------------------------------------------------------------------------------------------------
    def forward_train(self, x, *, dense_latent: bool = True):
        """``(sparse_latent [B,H] or None, reconstruction [B,D], polarize_loss [])`` with a ``grad_fn``: the forward the
        reference trains through (sae/binary.py:91-103 with the soft sigmoid-bit decoder, whatever ``decoder.decode_mode``
        says), whose backward runs the HIP gradient kernels (csrc/train.hip).  ``loss.backward()`` fills the ``.grad`` of
        encoder.0.weight / .bias, decoder.weight / .bias (and of ``x`` if it requires grad).

        Same selection path and bits as ``forward()``: latent and reconstruction equal ``forward()`` with
        ``decode_mode = "soft"`` bit for bit, the polarize loss to within one fp32 ulp (a device-side fixed-order sum;
        nothing is read back to the host except the prefilter path's 4-byte flagged-row count).  ``dense_latent=False``:
        the first output is None and the dense [B, H] latent is never written.  Derived weights (prefilter copies, packed
        dictionary) are keyed on the parameters' version counters, so an optimizer step is picked up by the next call."""
        x = require_device_input(x, "x")
        lin, dec = self.encoder.linear, self.decoder
        if not ops.train_supported(self.input_dim, self.top_k):
            raise ValueError(f"BinarySAE.forward_train: the gradient kernels take input_dim a multiple of 4 up to 4096 and "
                             f"top-k <= 256 (got input_dim = {self.input_dim}, top-k = {self.top_k})")
        if x.shape[1] != self.input_dim:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {self.input_dim}]")
        latent, recon, pol = _BinaryTrainStep.apply(self, bool(dense_latent), x, lin.weight, lin.bias, dec.weight, dec.bias)
        return (latent if dense_latent else None), recon, pol

    def _aux_decoder(self):
        """-> (logits, soft table [H, D], step) for forward_aux: the table the step's forward_train built while the logits
        have not changed since (no second [H, D n_bits] pass per step), a fresh one when forward_aux is called on its own."""
        dec = self.decoder
        st = self._train_cache.get((dec.weight,), lambda: {
            "table": ops.binary_soft_table(dec.weight.detach(), dec.out_features, dec.n_bits)})
        return dec.weight, st["table"], dec.quantization_step

    def _aux_unit_grad(self, offsets, entries, val, gv, x, g_recon, want_encoder: bool, want_decoder: bool):
        dec = self.decoder
        return ops.train_unit_grad(offsets, entries, val, gv, x, g_recon, dec.weight.detach(), dec.n_bits,
                                   dec.quantization_step, None, want_encoder=want_encoder, want_logits=want_decoder)

    def _batch_unit_grad(self, offsets, entries, val, gv, x, g_recon, g_pol, want_encoder: bool, want_decoder: bool):
        """the unit sums of forward_train_batch_topk: forward_train's, polarize term included, over lists of stride cap"""
        dec = self.decoder
        return ops.train_unit_grad(offsets, entries, val, gv, x, g_recon, dec.weight.detach(), dec.n_bits,
                                   dec.quantization_step, g_pol, want_encoder=want_encoder, want_logits=want_decoder)

    # -- nested dictionaries ----------------------------------------------------------------------------------------
    def forward_train_nested(self, x, bounds, *, dense_latent: bool = True):
        """``forward_train`` with one reconstruction per dictionary prefix: ``(sparse_latent [B,H] or None, (recon_0, ...,
        recon_{L-1}), polarize_loss [])``, where ``recon_l`` [B,D] decodes the selected units below ``bounds[l]`` (ascending,
        the last one ``hidden_dim``) through the soft table and ``recon_{L-1}`` is ``forward_train``'s reconstruction bit for
        bit.  The levels are the rows of one [L,B,D] tensor, written by one walk over each row's list; the backward
        (csrc/nested.hip, csrc/train.hip) fills the same ``.grad`` as ``forward_train``'s from the gradients of all levels.
        Same selection path and bits as ``forward_train``; ``model.activity`` is fed once."""
        if not ops.train_supported(self.input_dim, self.top_k):
            raise ValueError(f"BinarySAE.forward_train_nested: the gradient kernels take input_dim a multiple of 4 up to 4096 "
                             f"and top-k <= 256 (got input_dim = {self.input_dim}, top-k = {self.top_k})")
        return self._forward_train_nested(x, bounds, dense_latent, self.decoder.weight, self.decoder.bias)

    def _nested_select(self, x, want_dense: bool):
        """-> (idx, val, dense latent or None): the selection of _run() without its decode"""
        if self.top_k == 0:
            return self._zero_k(x, want_dense)[:3]
        path = self.resolved_latent_path(x.shape[0])
        self._check_limits(path, x.shape[0])
        return self._select(x, self.top_k, path, want_dense)

    def _nested_decoder(self):
        """-> (decoder description, decoder bias) of forward_nested: what forward() decodes from"""
        return self._fused_decoder(self.decoder.resolved_decode_mode() == "hard"), self.decoder.bias.detach()

    def _nested_train_decoder(self):
        """-> (soft table [H, D], step, polarize loss): built once per step and left for forward_aux, as forward_train does"""
        dec = self.decoder
        table, pol = ops.binary_soft_table_polarize(dec.weight.detach(), dec.out_features, dec.n_bits)
        self._train_cache.put((dec.weight,), {"table": table})
        return table, dec.quantization_step, pol

    _LEVELS_UNIT_GRAD = {"nested": ops.train_unit_grad_nested, "multik": ops.train_unit_grad_multik}

    def _levels_unit_grad(self, family: str, offsets, entries, val, gv, x, G, levels, g_pol, want_encoder: bool,
                          want_decoder: bool):
        """the unit sums with g_recon = G[level of the unit] ("nested") or G[point of the entry's rank] ("multik")"""
        dec = self.decoder
        return self._LEVELS_UNIT_GRAD[family](offsets, entries, val, gv, x, G, levels, dec.weight.detach(), dec.n_bits,
                                              dec.quantization_step, g_pol, want_encoder=want_encoder, want_logits=want_decoder)

    # -- two batches in flight --------------------------------------------------------------------------------
    def forward_submit(self, x, slot: int = 0, want_dense: bool = True):
        """Queue one forward without waiting for the GPU anywhere: returns a handle whose ``result()`` gives
        ``(latent, reconstruction, polarize_loss)`` (``(idx, val, reconstruction)`` with want_dense=False).  With the
        default path this is the two-call form of the C ABI (qsae_prefilter_submit / _finish, or their _table forms for
        an unpolarised checkpoint): submit batch i+1, then
        call ``result()`` of batch i -- the 4-byte read-back of batch i no longer idles the GPU.  Batches in flight
        together need different ``slot`` numbers; other paths compute eagerly and return a finished handle."""
        def to_result(idx, val, latent, recon):
            return (latent, recon, self.decoder.packed()["polarize"]) if want_dense else (idx, val, recon)
        if self.latent_path == "slabs":
            raise ValueError("BinarySAE.forward_submit: the two-call form is not built for latent_path = 'slabs' (every slab "
                             "reads its flagged-row count back); call forward() or forward_compact()")
        with torch.no_grad():
            xd = require_device_input(x, "x")
            if self.top_k > 0 and self.resolved_latent_path(xd.shape[0]) == "prefilter" and self.fuse_decode:
                self._check_limits("prefilter", xd.shape[0])
                enc = self._prefilter_operands(xd)
                decoder = self._fused_decoder(self.decoder.resolved_decode_mode() == "hard")
                pending = self._submit_prefilter(enc, self.top_k, decoder, self.decoder.bias.detach(), want_dense, slot)
                return SubmittedForward(self, pending, None, to_result)
            return SubmittedForward(self, None, self._run(xd, want_dense), to_result)


class _BinaryTrainStep(torch.autograd.Function):
    """The BinarySAE soft-decoder forward and its gradient (the table in DESIGN.md section 4.10):
    gv = g_latent[r, h] + step <g_recon[r], T[h]> on the k selected entries of each row, then per unit the sums over
    the rows that selected it (dW_enc, db_enc, dInt -> the logit gradient with the polarize term), and db_dec."""

    @staticmethod
    def forward(ctx, model, dense_latent, x, W_enc, b_enc, logits, b_dec):
        dec = model.decoder
        table, pol = ops.binary_soft_table_polarize(logits.detach(), dec.out_features, dec.n_bits)
        model._train_cache.put((dec.weight,), {"table": table})
        xf = as_f32c(x.detach())
        idx, val, latent, recon = model._run(xf, dense_latent, soft_table=table)
        if model.activity is not None:
            model.activity.add_compact(idx, val)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val, table)
        ctx.model = model
        ctx.x_dtype = x.dtype
        if latent is None:
            return None, recon, pol
        return latent, recon, pol

    @staticmethod
    def backward(ctx, g_latent, g_recon, g_pol):
        xf, idx, val, table = ctx.saved_tensors
        model = ctx.model
        lin, dec = model.encoder.linear, model.decoder
        need_W, need_b, need_l = ctx.needs_input_grad[3:6]

        def unit_grad(offsets, entries, gv):
            return ops.train_unit_grad(offsets, entries, val, gv, xf, g_recon, dec.weight.detach(), dec.n_bits,
                                       dec.quantization_step, g_pol, want_encoder=need_W or need_b, want_logits=need_l)
        return (None, None) + sparse_backward(idx, table, dec.quantization_step, g_recon, g_latent, lin.weight, dec.bias,
                                              ctx.needs_input_grad[2:7], ctx.x_dtype, unit_grad)
