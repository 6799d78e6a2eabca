"""BinaryLatentSAE: sigmoid encoder, latent binarised at 0.5, dense fp32 decoder
(reference: sae/binary_latent.py:6-28)."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import torch_ops as ops          # torch.ops.qsae.* (dispatcher ops over the C ABI)
from .base import HipEncoder, SparseAutoencoder, as_f32c, dense_encoder_backward, require_device_input

# sigmoid(w) >= 0.5 in the reference's fp32 op sequence  <=>  w >= this pre-activation (bit pattern 0xB43FFFFE,
# -1.79e-7; measured over all floats, tests/golden/sigmoid_cutoffs.npz)
_GE_HALF_CUTOFF = float(torch.tensor([0xB43FFFFE - (1 << 32)], dtype=torch.int32).view(torch.float32)[0])


class BinaryLatentSAE(SparseAutoencoder):
    """``forward(x) -> (binary_latent [B,H] in {0,1}, reconstruction [B,D])``.  The reference decodes
    ``latent + (binary - latent).detach()``, which is the binary latent up to one rounding (<= 6e-8); here the
    decoder contracts the binary latent itself."""

    #: a ``training.FeatureActivity`` or None: when set, ``forward_train`` (never ``forward``) adds every batch's active units
    #: to it from the tensors it already holds; outputs and gradients are the same bits either way
    activity = None

    def __init__(self, input_dim, hidden_dim):
        super().__init__(input_dim, hidden_dim)
        self.encoder = HipEncoder(nn.Linear(input_dim, hidden_dim), nn.Sigmoid())
        self.decoder = nn.Linear(hidden_dim, input_dim)

    def forward(self, x):
        with torch.no_grad():
            x = require_device_input(x, "x")
            lin = self.encoder.linear
            pre = ops.encode_dense(x if x.dtype == torch.float32 else x.float(), lin.weight.detach(), lin.bias.detach(),
                                   ops.ACT_NONE)
            binary_latent = ops.threshold_ge(pre, _GE_HALF_CUTOFF)
            recon = ops.encode_dense(binary_latent, self.decoder.weight.detach(), self.decoder.bias.detach(),
                                     ops.ACT_NONE)
            return binary_latent, recon

    def forward_train(self, x):
        """``(binary_latent [B,H], reconstruction [B,D])``, bit for bit the outputs of ``forward()`` (the same
        ``encode_dense`` contractions): the forward the reference trains through (sae/binary_latent.py:19-27, the bl_sae of
        training/trainer.py), whose backward runs the HIP gradient kernels (csrc/train_gemm.hip; the table in DESIGN.md
        section 4.24).  ``binary_latent`` is not differentiable (the reference computes it under ``no_grad``);
        ``reconstruction`` carries the ``grad_fn``.  ``loss.backward()`` fills the ``.grad`` of encoder.0.weight / .bias and
        decoder.weight / .bias, and of ``x`` if it requires grad; what does not require grad is not computed.

        Kept alive between forward and backward: ``x`` (as fp32), the encoder pre-activation [B, H] and the latent's packed
        bits [B, H / 32] -- not the fp32 latent handed to the caller.  The backward turns the pre-activation into its own
        gradient in place, so a second backward through the same step raises a RuntimeError.  It reads ``decoder.weight``
        and ``encoder.0.weight`` when it runs, as autograd's saved references would: a parameter edited in place between
        forward and backward is seen with its new values."""
        x = require_device_input(x, "x")
        lin = self.encoder.linear
        H, D = lin.weight.shape
        B = x.shape[0]
        if x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        if B < 1:
            raise ValueError("BinaryLatentSAE.forward_train: empty batch")
        if not ops.train_blatent_supported(D, H) or B * H >= 2 ** 31:
            raise ValueError(f"BinaryLatentSAE.forward_train: the gradient kernels take input_dim a multiple of 4 up to 4096, "
                             f"hidden_dim a multiple of 32 and batch * hidden_dim below 2^31 (got input_dim = {D}, "
                             f"hidden_dim = {H}, batch = {B})")
        return _BinaryLatentTrainStep.apply(self, x, lin.weight, lin.bias, self.decoder.weight, self.decoder.bias)


class _BinaryLatentTrainStep(torch.autograd.Function):
    """The BinaryLatentSAE forward and its gradient (the table in DESIGN.md section 4.24).  The binarisation is a
    straight-through estimator, so every unit of every row receives dz = <G, W_d[:, h]>; the latent is dense (about half of
    the bits are set), so the backward is encoder-sized fp32 contractions: dpre = dz p (1 - p) with decoder.weight read in
    its own [D, H] layout, dW_d = G^T z from the packed bits (TN), dW_e = dpre^T x (TN)."""

    @staticmethod
    def forward(ctx, model, x, W_enc, b_enc, W_dec, b_dec):
        xf = as_f32c(x.detach())
        pre = ops.encode_dense(xf, W_enc.detach(), b_enc.detach(), ops.ACT_NONE)
        binary_latent, zbits = ops.blatent_binarize(pre, _GE_HALF_CUTOFF)
        if model.activity is not None:
            model.activity.add_bits(zbits)
        recon = ops.encode_dense(binary_latent, W_dec.detach(), b_dec.detach(), ops.ACT_NONE)
        ctx.mark_non_differentiable(binary_latent)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xf, zbits)
        ctx.pre = pre
        ctx.model, ctx.x_dtype = model, x.dtype
        return binary_latent, recon

    @staticmethod
    def backward(ctx, _g_latent, g_recon):
        if g_recon is None:
            return (None,) * 6
        xf, zbits = ctx.saved_tensors
        model = ctx.model
        need_x, need_W, need_b, need_wd, need_bd = ctx.needs_input_grad[1:6]
        G = as_f32c(g_recon)
        dx = dW = db = dwd = dbd = None
        if need_bd:
            dbd = ops.train_col_sum(G)
        if need_wd:
            dwd = ops.train_blatent_dweight(G, zbits, zbits.shape[1] * 32)
        if need_x or need_W or need_b:
            if ctx.pre is None:
                raise RuntimeError("Trying to backward through BinaryLatentSAE.forward_train a second time: the saved "
                                   "pre-activation was turned into its gradient in place by the first backward")
            dpre = ops.train_blatent_dpre(ctx.pre, G, model.decoder.weight.detach())
            ctx.pre = None
            dx, dW, db = dense_encoder_backward(dpre, xf, model.encoder.linear.weight.detach(), need_x, need_W, need_b,
                                                ctx.x_dtype)
        return (None, dx, dW, db, dwd, dbd)
