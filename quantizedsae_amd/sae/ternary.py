"""TernarySparseAutoencoder: ReLU encoder, {-1,0,+1} dictionary (reference: sae/ternary.py)."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import torch_ops as ops          # torch.ops.qsae.* (dispatcher ops over the C ABI)
from .base import HipEncoder, PackedCache, as_f32c, dense_encoder_backward, require_device_input

_GPU_ONLY = ("RigL mask maintenance (sae/ternary.py:27-39,54-90) runs on the GPU only: the decoder's parameters are on the "
             "host and there is no CPU fallback")


class STEWeights(nn.Module):
    """Ternary dictionary ``hard = sign(w) * (|w| >= threshold)``, no bias (sae/ternary.py:41-52).
    The straight-through expression of the reference evaluates to exactly ``hard`` and does not
    depend on ``mask``; the 2-bit packed codes are derived from ``weight`` alone."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.threshold = 0.5
        self.register_buffer("mask", torch.ones(out_features, in_features))
        self.input_activations = None   # the reference pins the last [B,H] input here; not kept
        self.output_grad = None
        # what update_mask() reads of them, left by forward_train (plain attributes, not buffers: no state_dict keys)
        self.activation_mean = None     # a [H] = mean over the batch of the latent, from the last forward_train
        self.output_grad_mean = None    # delta [D] = mean over the batch of the gradient at the reconstruction, from its backward
        nn.init.kaiming_normal_(self.weight)
        self._cache = PackedCache()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # checkpoints saved by the reference after a forward carry these hook buffers
        for name in ("input_activations", "output_grad"):
            state_dict.pop(prefix + name, None)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def codes(self) -> torch.Tensor:
        return self._packed()["c"]

    #: "auto" | "split" | "fp32".  split: the latent as three exact bf16 terms against the {-1, 0, +1} dictionary on the
    #: bf16 matrix pipe, fp32 accumulation (qsae_decode_ternary_dense_split) -- every product exact, the sum rounded in
    #: another order than the fp32 kernel's (both within 1e-5 of the fp64-accumulating oracle); fp32: the exact-fp32 MFMA
    #: chain.  auto = split where the kernel covers the shape (input_dim 512, hidden_dim % 64 == 0), else fp32.
    precision = "auto"

    def _packed(self) -> dict:
        if self.threshold != 0.5:
            raise NotImplementedError("only the reference threshold 0.5 is packed")
        return self._cache.get((self.weight,), lambda: {"c": ops.pack_ternary(self.weight.detach())})

    def dictionary_bf16(self) -> torch.Tensor:
        """The bf16 image of the dictionary the split kernel streams (once per checkpoint, 2 H D bytes)."""
        st = self._packed()
        if "tq" not in st:
            D, H = self.weight.shape
            st["tq"] = ops.expand_codes_bf16(st["c"], D, H)
        return st["tq"]

    def resolved_precision(self, rows: int) -> str:
        if self.precision not in ("auto", "split", "fp32"):
            raise ValueError(f"precision must be 'auto', 'split' or 'fp32', got {self.precision!r}")
        D, H = self.weight.shape
        ok = rows > 0 and ops.split_dec_supported(rows, H, D)
        if self.precision == "split" and not ok:
            raise ValueError(f"STEWeights: the bf16 split decoder needs input_dim 512 and hidden_dim % 64 == 0 (got {D}, {H})")
        return "split" if (ok and self.precision != "fp32") else "fp32"

    def forward(self, x):
        with torch.no_grad():
            x = require_device_input(x, "x")
            if x.dtype != torch.float32 or x.stride(1) != 1:
                x = x.float().contiguous()
            if self.resolved_precision(x.shape[0]) == "split" and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0:
                return ops.decode_ternary_dense_split(x, self.dictionary_bf16(), self.weight.shape[0])
            return ops.decode_ternary_dense(x, self.codes(), self.weight.shape[0])

    def ternary_rows(self) -> torch.Tensor:
        """The fp32 image of the dictionary transposed, [H, D] in {-1, 0, +1}: the K-contiguous operand of the backward's
        dh contraction (once per weight version, 4 H D bytes)."""
        st = self._packed()
        if "tr" not in st:
            st["tr"] = ops.train_ternary_rows(self.weight.detach())
        return st["tr"]

    def invalidate_packed(self) -> None:
        """Forget the derived weight copies (2-bit codes, bf16 and fp32 dictionaries): needed after an edit of ``weight``
        that moves neither its pointer nor its version counter -- the mask methods below do it themselves."""
        self._cache.clear()

    def _mask_operands(self):
        w, m = self.weight, self.mask
        if not (w.is_cuda and m.is_cuda):
            raise NotImplementedError(_GPU_ONLY)
        if w.dtype != torch.float32 or m.dtype != torch.float32 or not w.is_contiguous() or not m.is_contiguous():
            raise ValueError("STEWeights: the mask kernels take contiguous fp32 weight and mask")
        D, H = w.shape
        if not ops.train_mask_supported(D, H):
            raise ValueError(f"STEWeights: the mask kernels take input_dim * hidden_dim below 2^31 and a multiple of 4 "
                             f"(got {D} x {H})")
        return w.detach(), m

    def init_mask(self, sparsity):
        """``int(numel * sparsity)`` positions with the smallest ``|weight|`` get ``mask = 0`` (exactly that many), then
        ``weight *= mask`` (sae/ternary.py:27-39), in place on the device.  Where the reference leaves the order among
        equal ``|weight|`` at the boundary to ``torch.topk``, ties are taken in ascending flat index ``d * H + h``."""
        w, m = self._mask_operands()
        n = int(w.numel() * sparsity)
        if not 0 <= n <= w.numel():
            raise ValueError(f"init_mask: sparsity {sparsity} gives {n} inactive positions of {w.numel()}")
        ops.train_mask_init(w, m, n)
        self.invalidate_packed()          # written through the raw pointers: neither data_ptr nor version moved

    def update_mask(self, f_decay, sparsity_rate=0.7, *, check=False):
        """One RigL step (sae/ternary.py:54-87) in place on the device, ``n = int(f_decay * (1 - sparsity_rate) * numel)``:
        the drop (every active position with ``|weight|`` <= the n-th smallest active ``|weight|``, ties included), the grow
        (the n largest ``|delta[d]| * |a[h]|`` among the positions inactive after the drop; exactly n, ties at the boundary in
        ascending flat index ``d * H + h`` where the reference leaves them to ``torch.topk``; fewer inactive positions than n:
        all of them), then ``mask = active`` and ``weight *= mask``.  ``a`` / ``delta`` are ``activation_mean`` /
        ``output_grad_mean`` as the last ``forward_train`` and its backward left them; before the first backward only the
        drop happens, as in the reference.

        Nothing is read back to the host: n comes from the Python arithmetic above, every selection is made on the device.
        So an n above the number of active positions -- a RuntimeError from ``kthvalue`` in the reference -- cannot be seen
        here and saturates: every active position drops.  ``check=True`` spends one host read on the active count and raises
        ValueError before anything changes."""
        w, m = self._mask_operands()
        n = int(f_decay * (1 - sparsity_rate) * w.numel())
        if not 0 <= n <= w.numel():
            raise ValueError(f"update_mask: f_decay {f_decay}, sparsity_rate {sparsity_rate} give n = {n} of {w.numel()} positions")
        if check and n > 0:
            active = int((m != 0).sum().item())
            if n > active:
                raise ValueError(f"update_mask: n = {n} is above the {active} active positions")
        a, delta = self.activation_mean, self.output_grad_mean
        if a is None or delta is None:
            a = delta = None
        ops.train_mask_update(w, m, a, delta, n)
        self.invalidate_packed()          # written through the raw pointers: neither data_ptr nor version moved

    def mask_grad(self):
        """``weight.grad *= mask`` in place (sae/ternary.py:89-90).  forward_train's backward already returns the masked
        gradient, as the reference's autograd does, so this is idempotent."""
        if not self.weight.is_cuda:
            raise NotImplementedError(_GPU_ONLY)
        if self.weight.grad is not None:
            self.weight.grad.mul_(self.mask)


class TernarySparseAutoencoder(ops.GraphForwardMixin, nn.Module):
    """``forward(x) -> (h [B,H], recon [B,D])``; no top-k in forward (sae/ternary.py:116-122)."""

    #: a ``training.FeatureActivity`` or None: when set, ``forward_train`` (never ``forward``) adds every batch's active units
    #: to it from the tensors it already holds; outputs and gradients are the same bits either way
    activity = None

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.encoder = HipEncoder(nn.Linear(input_dim, hidden_dim), nn.ReLU())
        self.decoder = STEWeights(hidden_dim, input_dim)
        self.topk = int(hidden_dim * 0.002)
        ops.module_handle(self)

    def apply_topk_activation(self, h):
        """Top-k of each row with non-positive survivors zeroed (sae/ternary.py:102-114)."""
        with torch.no_grad():
            out = require_device_input(h, "h").float().clone()
            ops.topk_rows(out, self.topk, zero_rest=True)
            return torch.clamp_(out, min=0)

    def _forward_eager(self, x):
        h = self.encoder(require_device_input(x, "x"))
        return h, self.decoder(h)

    def forward_train(self, x):
        """``(h [B,H], recon [B,D])`` with a ``grad_fn``: the forward the reference trains through (sae/ternary.py:41-52,
        116-122; the t_sae branch of training/trainer.py:157-164), the same bits as ``forward()`` on whichever decoder
        ``precision`` resolves, whose backward runs the HIP gradient kernels.  ``loss.backward()``
        fills the ``.grad`` of encoder.0.weight / .bias and decoder.weight (already multiplied by ``decoder.mask``; the mask
        is a buffer and gets none), and of ``x`` if it requires grad.  A gradient arriving at ``h`` (an L1 term) is added.

        Kept alive between forward and backward: ``x`` (as fp32), ``h`` [B, H] -- the tensor handed to the caller, which
        the backward only reads -- the decoder's fp32 dictionary rows [H, D] (cached per weight version) and the mask.  The
        backward allocates its own [B, H] buffer for ``dpre`` (1 GiB at B = 8192, H = 32768).

        For ``decoder.update_mask`` the forward leaves ``decoder.activation_mean`` (a [H], the batch mean of ``h``) and the
        backward ``decoder.output_grad_mean`` (delta [D], the batch mean of the gradient at ``recon``); the [B, H] tensor the
        reference pins is not kept."""
        x = require_device_input(x, "x")
        lin = self.encoder.linear
        H, D = lin.weight.shape
        if not ops.train_ternary_supported(D, H):
            raise ValueError(f"TernarySparseAutoencoder.forward_train: the gradient kernels take input_dim a multiple of 4 up "
                             f"to 4096 and hidden_dim a multiple of 4 (got input_dim = {D}, hidden_dim = {H})")
        if x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        if x.shape[0] < 1:
            raise ValueError("TernarySparseAutoencoder.forward_train: empty batch")
        return _TernaryTrainStep.apply(self, x, lin.weight, lin.bias, self.decoder.weight)

    def forward(self, x):
        if torch.compiler.is_compiling():              # one graph node: torch.ops.qsae.ternary_sae_forward
            with torch.no_grad():
                lin = self.encoder.linear
                return torch.ops.qsae.ternary_sae_forward(x, [lin.weight, lin.bias, self.decoder.weight], self._qsae_handle)
        return self._forward_eager(x)


class _TernaryTrainStep(torch.autograd.Function):
    """The TernarySparseAutoencoder forward and its gradient (the table in DESIGN.md section 4.13).  The latent is dense
    (ReLU, no top-k), so the backward is three encoder-sized fp32 contractions: dh = gh + G T (NT, with the ReLU gate in the
    epilogue), dw = mask * (G^T h) (TN, the mask on the store), dW_enc = dpre^T x (TN)."""

    @staticmethod
    def forward(ctx, model, x, W_enc, b_enc, w):
        dec = model.decoder
        xf = as_f32c(x.detach())
        h = model.encoder(xf)
        recon = dec(h)
        if model.activity is not None:
            model.activity.add_dense(h)
        dec.activation_mean = ops.train_col_sum(h).div_(h.shape[0])
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, h, dec.ternary_rows(), dec.mask)
        ctx.model, ctx.x_dtype = model, x.dtype
        return h, recon

    @staticmethod
    def backward(ctx, g_h, g_recon):
        xf, h, t_rows, mask = ctx.saved_tensors
        model = ctx.model
        dec = model.decoder
        need_x, need_W, need_b, need_w = ctx.needs_input_grad[1:5]
        G = gh = None
        if g_recon is not None:
            G = as_f32c(g_recon)
            dec.output_grad_mean = ops.train_col_sum(G).div_(G.shape[0])
        if g_h is not None:
            gh = as_f32c(g_h)
        dx = dW = db = dw = None
        if need_w:
            dw = ops.train_ternary_dweight(G, h, mask) if G is not None else torch.zeros_like(dec.weight)
        if need_x or need_W or need_b:
            dpre = ops.train_ternary_dpre(h, G, gh, t_rows)
            dx, dW, db = dense_encoder_backward(dpre, xf, model.encoder.linear.weight.detach(), need_x, need_W, need_b,
                                                ctx.x_dtype)
        return (None, dx, dW, db, dw)
