"""BaselineSparseAutoencoder: Linear -> top-32 -> Linear (reference: sae/baseline.py:4-51)."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import torch_ops as ops          # torch.ops.qsae.* (dispatcher ops over the C ABI)
from .base import HipEncoder, PackedCache, as_f32c, require_device_input
from .topk import SubmittedForward, TopKCore, sparse_backward


class BaselineSparseAutoencoder(ops.GraphForwardMixin, TopKCore, nn.Module):
    #: a ``training.FeatureActivity`` or None: when set, ``forward_train`` (never ``forward``) adds every batch's active units
    #: to it from the tensors it already holds; outputs and gradients are the same bits either way
    activity = None

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.encoder = HipEncoder(nn.Linear(input_dim, hidden_dim))   # no ReLU in the reference either
        self.decoder = nn.Linear(hidden_dim, input_dim)
        self.topk = 32
        self.latent_path = "auto"      # "auto" | "prefilter" | "fused" | "inplace" | "slabs" (see BinarySAE.latent_path)
        self._cache = PackedCache()
        self._init_topk()
        ops.module_handle(self)

    def _table(self) -> torch.Tensor:
        # decoder.weight is [D, H]; the sparse decode gathers rows of its transpose [H, D]
        return self._cache.get((self.decoder.weight,),
                               lambda: {"t": self.decoder.weight.detach().t().contiguous()})["t"]

    def resolved_latent_path(self, rows: int) -> str:
        """Which path _run() takes for a batch of this many rows.  Not BinarySAE's rule, and deliberately not aligned with
        it: ``latent_path`` is not validated here, and an explicit "prefilter" or "fused" on a small batch falls to the
        in-place path (BinarySAE honours it)."""
        H, D = self.encoder.linear.weight.shape
        if self.latent_path == "slabs":         # opt-in only: no other value resolves to it
            return "slabs"
        big = rows >= 2048 and H >= 8192
        if big and self.latent_path in ("auto", "prefilter") and ops.prefilter_supported(rows, D, H, self.topk):
            return "prefilter"
        return "fused" if (big and self.latent_path != "inplace") else "inplace"

    def _check_limits(self, rows: int) -> None:
        H, D = self.encoder.linear.weight.shape
        if self.latent_path == "slabs":
            if not self._slabs_supported(rows, self.topk):
                raise ValueError(f"BaselineSparseAutoencoder: the slab selection does not take input_dim = {D}, hidden_dim = {H}, "
                                 f"topk = {self.topk} at slab_width = {self.slab_width} (input_dim and hidden_dim multiples of 4, "
                                 "hidden_dim <= 2^20, topk <= 256, slab_width a multiple of 256 up to 32768, at most 32 slabs of "
                                 "at least topk units)")
            return
        if (H > 32768 and self.latent_path == "inplace") or not ops.encode_topk_supported(max(rows, 1), D, H, self.topk):
            raise ValueError(f"BaselineSparseAutoencoder: no top-k path takes input_dim = {D}, hidden_dim = {H} at a batch of "
                             f"{rows} rows (input_dim and hidden_dim multiples of 4; hidden_dim <= 32768, or up to 65536 for "
                             "batches of >= 2048 rows off the in-place path; latent_path = 'slabs' takes wider dictionaries)")

    def _run(self, x, want_dense: bool):
        """-> (idx, val, dense latent or None, reconstruction): the one implementation behind forward() and
        forward_compact()."""
        x = require_device_input(x, "x")
        self._check_limits(x.shape[0])
        path = self.resolved_latent_path(x.shape[0])
        if path == "prefilter":
            # one call: candidate sweep, exact refinement, and the row's reconstruction from the fp32 decoder rows as soon
            # as the row is ranked (qsae_table_forward_prefilter)
            enc = self._prefilter_operands(x)
            return self._forward_prefilter(enc, self.topk, ("table", self._table(), 1.0), self.decoder.bias.detach(),
                                           want_dense)
        idx, val, h = self._select(x, self.topk, path, want_dense)
        return idx, val, h, ops.decode_table_sparse(idx, val, self._table(), 1.0, self.decoder.bias.detach())

    def forward(self, x):
        """-> (h_sparse [B,H], recon [B,D])  (sae/baseline.py:17-31)."""
        with torch.no_grad():
            if torch.compiler.is_compiling():          # one graph node: torch.ops.qsae.baseline_sae_forward
                lin = self.encoder.linear
                _, _, h, recon = torch.ops.qsae.baseline_sae_forward(
                    x, [lin.weight, lin.bias, self.decoder.weight, self.decoder.bias], self._qsae_handle, True)
                return h, recon
            _, _, h, recon = self._run(x, want_dense=True)
            return h, recon

    # -- training -------------------------------------------------------------------------------------------------
    def forward_train(self, x, *, dense_latent: bool = True):
        """``(h_sparse [B,H] or None, reconstruction [B,D])`` with a ``grad_fn``: the forward the reference trains through
        (sae/baseline.py:17-40; the baseline_sae branch of training/trainer.py:166-173), whose backward runs the HIP gradient
        kernels (csrc/train.hip).  ``loss.backward()`` fills the ``.grad`` of encoder.0.weight / .bias and decoder.weight /
        .bias (and of ``x`` if it requires grad); a gradient arriving at ``h_sparse`` counts at the selected entries only, as
        through the reference's ``scatter_``.

        Same path selection and bits as ``forward()``.  ``dense_latent=False``: the first output is None and the dense
        [B, H] latent is never written.  ``self.topk`` is read per call.  Derived weights are keyed on the parameters'
        version counters, so an optimizer step is picked up by the next call."""
        x = require_device_input(x, "x")
        lin, dec = self.encoder.linear, self.decoder
        H, D = lin.weight.shape
        if not ops.train_supported(D, self.topk) or self.topk < 1:
            raise ValueError(f"BaselineSparseAutoencoder.forward_train: the gradient kernels take input_dim a multiple of 4 up "
                             f"to 4096 and 1 <= topk <= 256 (got input_dim = {D}, topk = {self.topk})")
        if x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        if x.shape[0] * self.topk >= 2 ** 31:
            raise ValueError(f"BaselineSparseAutoencoder.forward_train: batch * topk = {x.shape[0] * self.topk} is not below 2^31")
        self._check_limits(x.shape[0])
        latent, recon = _BaselineTrainStep.apply(self, bool(dense_latent), x, lin.weight, lin.bias, dec.weight, dec.bias)
        return (latent if dense_latent else None), recon

    def _aux_decoder(self):
        """-> (decoder.weight, its transpose [H, D], 1.0) for forward_aux"""
        return self.decoder.weight, self._table(), 1.0

    def _aux_unit_grad(self, offsets, entries, val, gv, x, g_recon, want_encoder: bool, want_decoder: bool):
        return ops.train_table_unit_grad(offsets, entries, val, gv, x, g_recon, want_encoder=want_encoder,
                                         want_decoder=want_decoder)

    def _batch_unit_grad(self, offsets, entries, val, gv, x, g_recon, g_extra, want_encoder: bool, want_decoder: bool):
        """the unit sums of forward_train_batch_topk: forward_train's, over lists of stride cap"""
        return ops.train_table_unit_grad(offsets, entries, val, gv, x, g_recon, want_encoder=want_encoder,
                                         want_decoder=want_decoder)

    # -- nested dictionaries ----------------------------------------------------------------------------------------
    def forward_train_nested(self, x, bounds, *, dense_latent: bool = True):
        """``forward_train`` with one reconstruction per dictionary prefix: ``(h_sparse [B,H] or None, (recon_0, ...,
        recon_{L-1}))``, where ``recon_l`` [B,D] decodes the selected units below ``bounds[l]`` (ascending, the last one
        ``hidden_dim``) and ``recon_{L-1}`` is ``forward_train``'s reconstruction bit for bit.  The levels are the rows of one
        [L,B,D] tensor; see BinarySAE.forward_train_nested."""
        H, D = self.encoder.linear.weight.shape
        if not ops.train_supported(D, self.topk) or self.topk < 1:
            raise ValueError(f"BaselineSparseAutoencoder.forward_train_nested: the gradient kernels take input_dim a multiple of "
                             f"4 up to 4096 and 1 <= topk <= 256 (got input_dim = {D}, topk = {self.topk})")
        if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[0] * self.topk >= 2 ** 31:
            raise ValueError(f"BaselineSparseAutoencoder.forward_train_nested: batch * topk = {x.shape[0] * self.topk} is not "
                             "below 2^31")
        return self._forward_train_nested(x, bounds, dense_latent, self.decoder.weight, self.decoder.bias)[:2]

    def _nested_select(self, x, want_dense: bool):
        """-> (idx, val, dense latent or None): the selection of _run() without its decode"""
        self._check_limits(x.shape[0])
        return self._select(x, self.topk, self.resolved_latent_path(x.shape[0]), want_dense)

    def _nested_decoder(self):
        """-> (decoder description, decoder bias) of forward_nested: what forward() decodes from"""
        return ("table", self._table(), 1.0), self.decoder.bias.detach()

    def _nested_train_decoder(self):
        return self._table(), 1.0, None

    _LEVELS_UNIT_GRAD = {"nested": ops.train_table_unit_grad_nested, "multik": ops.train_table_unit_grad_multik}

    def _levels_unit_grad(self, family: str, offsets, entries, val, gv, x, G, levels, g_extra, want_encoder: bool,
                          want_decoder: bool):
        """the unit sums with g_recon = G[level of the unit] ("nested") or G[point of the entry's rank] ("multik")"""
        return self._LEVELS_UNIT_GRAD[family](offsets, entries, val, gv, x, G, levels, want_encoder=want_encoder,
                                              want_decoder=want_decoder)

    def forward_compact(self, x):
        """(idx, val, reconstruction) without the dense latent; same path selection as forward()."""
        with torch.no_grad():
            idx, val, _, recon = self._run(x, want_dense=False)
            return idx, val, recon

    def forward_submit(self, x, slot: int = 0, want_dense: bool = True):
        """Queue one forward without waiting for the GPU anywhere (see BinarySAE.forward_submit): ``result()`` of the
        returned handle gives ``(h_sparse, reconstruction)`` (``(idx, val, reconstruction)`` with want_dense=False)."""
        def to_result(idx, val, h, recon):
            return (h, recon) if want_dense else (idx, val, recon)
        if self.latent_path == "slabs":
            raise ValueError("BaselineSparseAutoencoder.forward_submit: the two-call form is not built for latent_path = 'slabs' "
                             "(every slab reads its flagged-row count back); call forward() or forward_compact()")
        with torch.no_grad():
            xd = require_device_input(x, "x")
            self._check_limits(xd.shape[0])
            if self.resolved_latent_path(xd.shape[0]) == "prefilter":
                enc = self._prefilter_operands(xd)
                pending = self._submit_prefilter(enc, self.topk, ("table", self._table(), 1.0), self.decoder.bias.detach(),
                                                 want_dense, slot)
                return SubmittedForward(self, pending, None, to_result)
            return SubmittedForward(self, None, self._run(xd, want_dense), to_result)

    def invalidate_packed(self) -> None:
        """Forget the derived weight copies (transposed decoder table, fp16 / K-interleaved encoder copies): needed only
        after an in-place edit through ``.data`` -- normalize_decoder_weights() below does it itself."""
        self._cache.clear()
        self._clear_encoder_copies()

    def apply_topk_activation(self, h):
        """Dense in, dense out: keep the top-k entries of every row (sae/baseline.py:33-40)."""
        with torch.no_grad():
            out = require_device_input(h, "h").float().clone()
            ops.topk_rows(out, self.topk, zero_rest=True)
            return out

    def normalize_decoder_weights(self):
        """Unit-norm decoder columns (sae/baseline.py:42-51): one HIP pass that divides ``decoder.weight`` in place -- same
        storage, same Parameter, optimizer state untouched -- and leaves the normalised transpose, which becomes the cached
        decoder table of the next forward.  Shapes the kernel does not take (hidden_dim not a multiple of 4, a CPU or
        non-fp32 model) go through the reference's three torch ops."""
        with torch.no_grad():
            w = self.decoder.weight
            if w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.data_ptr() % 16 == 0 \
                    and ops.normalize_columns_supported(w.shape[1]):
                table = ops.normalize_columns_table(w.detach(), want_table=True)
                self.invalidate_packed()
                # the kernel wrote through the raw pointer: neither data_ptr nor (necessarily) the version counter moved,
                # so the cache could not notice by itself -- the table of the new weights replaces the old one explicitly
                self._cache.put((self.decoder.weight,), {"t": table})
                return
            w = self.decoder.weight.data
            self.decoder.weight.data = w / torch.clamp(torch.norm(w, dim=0, keepdim=True), min=1e-8)
            self.invalidate_packed()

    def project_decoder_grad(self):
        """Remove from ``decoder.weight.grad`` its component parallel to each atom (Bricken et al., Gao et al.): column h
        loses ``(g_h . w_h) w_h``, so that Adam's moments do not collect a radial part that the next
        normalize_decoder_weights() throws away.  One HIP pass over the gradient, in place; call it between the backward and
        the optimizer step.  Does nothing without a gradient.  Shapes the kernel does not take go through the torch
        composition (elementwise product, column sum, ``addcmul_``), as in normalize_decoder_weights."""
        w, g = self.decoder.weight, self.decoder.weight.grad
        if g is None:
            return
        with torch.no_grad():
            if w.is_cuda and w.dtype == torch.float32 and g.dtype == torch.float32 and w.is_contiguous() and g.is_contiguous() \
                    and w.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and ops.project_columns_supported(w.shape[1]):
                ops.project_columns(w.detach(), g)
                return
            dot = (g * w).sum(dim=0, keepdim=True)
            g.addcmul_(dot, w, value=-1)


class _BaselineTrainStep(torch.autograd.Function):
    """The baseline forward and its gradient (the table in DESIGN.md section 4.11): the BinarySAE gradient without the
    sigmoid chain.  gv = g_latent[r, h] + <g_recon[r], W_dec[:, h]> on the k selected entries of each row, then per unit
    the sums over the rows that selected it (dW_enc, db_enc, and column h of dW_dec), and db_dec.  Selected values may be
    negative (no ReLU in this model): nothing here looks at their sign."""

    @staticmethod
    def forward(ctx, model, dense_latent, x, W_enc, b_enc, W_dec, b_dec):
        xf = as_f32c(x.detach())
        idx, val, latent, recon = model._run(xf, dense_latent)
        if model.activity is not None:
            model.activity.add_compact(idx, val)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, idx, val, model._table())
        ctx.model = model
        ctx.x_dtype = x.dtype
        if latent is None:
            return None, recon
        return latent, recon

    @staticmethod
    def backward(ctx, g_latent, g_recon):
        xf, idx, val, table = ctx.saved_tensors
        lin, dec = ctx.model.encoder.linear, ctx.model.decoder
        need_W, need_b, need_Wd = ctx.needs_input_grad[3:6]

        def unit_grad(offsets, entries, gv):
            return ops.train_table_unit_grad(offsets, entries, val, gv, xf, g_recon, want_encoder=need_W or need_b,
                                             want_decoder=need_Wd)
        return (None, None) + sparse_backward(idx, table, 1.0, g_recon, g_latent, lin.weight, dec.bias,
                                              ctx.needs_input_grad[2:7], ctx.x_dtype, unit_grad)
