"""AuxK, the auxiliary loss of the top-k SAEs (Gao et al. 2024, "Scaling and evaluating sparse autoencoders"): at every step
the dead units alone reconstruct the residual ``x - recon`` through a top-``k_aux`` of their own pre-activations, and the
normalised error of that reconstruction gives them the gradient the main loss cannot -- ``sparse_backward`` reaches only the
units a row selected, and a dead unit is selected by no row.

    e = x - recon (detached)      aux = model.forward_aux(x, units, k_aux)
    loss = coef * |aux - e|^2 / |e - mean_rows(e)|^2          (0 when the denominator is 0)

The selection comes from ``qsaex_encode_topk_units``, the loss and its gradient from ``qsaex_auxk_loss`` (csrc/auxk.hip); the
backward of ``forward_aux`` is the models' sparse backward.  Nothing is read back to the host.
"""
from __future__ import annotations

import torch

from .. import torch_ops as ops
from ..sae.base import as_f32c
from ..sae.topk import AUX_MAX_K

__all__ = ["aux_k_loss", "AUX_MAX_K"]


class _AuxKLoss(torch.autograd.Function):
    """The loss kernel as a node: its gradient at ``aux`` was computed with the loss; ``x`` and ``recon`` are constants."""

    @staticmethod
    def forward(ctx, x, recon, aux, coef):
        loss, grad = ops.auxk_loss(x, recon, aux.detach(), coef)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return None, None, grad * g, None


def aux_k_loss(model, x, recon, units, k_aux: int = 64, coef: float = 1 / 32) -> torch.Tensor:
    """The AuxK loss of ``model`` (a BinarySAE or BaselineSparseAutoencoder) on the batch ``x`` whose reconstruction by
    ``forward_train`` is ``recon`` (detached here), over the units listed in ``units`` (int32, ascending, on the device: the
    tracker's ``dead_indices``).  -> a 0-d fp32 tensor with a ``grad_fn``; ``(main_loss + aux).backward()`` works in any
    ``torch.optim`` loop.  ``k_aux`` (at most 64) is clamped to the number of listed units.  With no unit listed there is
    nothing to train: the result is a constant 0 without a ``grad_fn`` and no kernel of the library runs."""
    n = int(units.shape[0])
    if int(k_aux) > AUX_MAX_K:
        raise ValueError(f"aux_k_loss: k_aux = {k_aux} exceeds the subset top-k kernel's limit of {AUX_MAX_K}")
    if n == 0:
        return torch.zeros((), dtype=torch.float32, device=x.device)
    aux = model.forward_aux(x, units, min(int(k_aux), n))
    return _AuxKLoss.apply(as_f32c(x.detach()), as_f32c(recon.detach()), aux, float(coef))
