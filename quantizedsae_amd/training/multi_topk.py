"""The Multi-TopK objective for the two top-k models (Gao et al. 2024, "Scaling and evaluating sparse autoencoders", the loss
``L(k) + L(4k) / 8``): the model is trained on the reconstruction at its own ``k`` and on the reconstruction at wider ``k'``, so
that the code does not overfit to one ``k``.

    outputs = model.forward_train_multi_topk(batch, ks)      recon_p decodes the ks[p] best-ranked entries of one top-ks[-1] list
    loss    = sum_p w_p * c * mse(recon_p, batch)  [+ polarize_lambda * polarize_loss for b_sae]   c = 0.5 (b_sae), 1 (baseline_sae)

Every point's loss and its gradient come from one pass of ``qsae_trainer_loss`` (mode 0, n = P); a weight ``w_p != 1`` scales the
point's gradient rows in place (an exact fp32 product; the C ABI carries no weight).  The points are the rows of one tensor, so
``torch.autograd.backward`` gets one root for them, and the backward of ``forward_train_multi_topk`` turns the P gradients into
their suffix sums and runs the sparse backward once (csrc/multi_topk.hip).  Nothing is read back to the host.
"""
from __future__ import annotations

import torch

from .. import torch_ops as ops
from ..sae.topk import TopKCore
from .loss import _const, _levels_base, recon_recipe

__all__ = ["multi_topk_loss", "default_multi_topk", "default_multi_topk_weights", "MULTI_TOPK_TYPES"]

MULTI_TOPK_TYPES = ("b_sae", "baseline_sae")
default_multi_topk = TopKCore.default_multi_topk


def default_multi_topk_weights(ks, top_k: int):
    """1 for the point equal to ``top_k`` and 1/8 for every other: ``L(k) + L(4k) / 8`` for the default points."""
    return [1.0 if int(k) == int(top_k) else 0.125 for k in ks]


def multi_topk_loss(sae_type: str, outputs, batch: torch.Tensor, config: dict, weights=None) -> torch.Tensor:
    """The Multi-TopK loss on ``outputs = model.forward_train_multi_topk(batch, ks)``: returns the per-point reconstruction
    losses (fp32 [P] on the device, unweighted; the objective's reconstruction part is ``sum_p weights[p] * losses[p]``) and
    runs ONE ``torch.autograd.backward`` on the outputs the loss reads -- the kernel's gradients for the points, row p scaled by
    ``weights[p]``, and a cached constant for the polarize loss of ``b_sae``.  ``weights=None``: every point counts once."""
    if sae_type not in MULTI_TOPK_TYPES:
        raise ValueError(f"multi_topk_loss: the Multi-TopK objective is built for baseline_sae and b_sae, the two top-k models; "
                         f"got {sae_type!r}")
    if not batch.is_cuda:
        raise RuntimeError(f"multi_topk_loss: quantizedsae_amd runs on MI355X only; batch is on {batch.device} "
                           "(no CPU fallback exists)")
    _, coef = recon_recipe(sae_type)
    recons = list(outputs[1])
    if not 1 <= len(recons) <= ops.MULTIK_MAX_POINTS:
        raise ValueError(f"multi_topk_loss: {len(recons)} points; 1 .. {ops.MULTIK_MAX_POINTS} are supported")
    w = [1.0] * len(recons) if weights is None else [float(v) for v in weights]
    if len(w) != len(recons):
        raise ValueError(f"multi_topk_loss: {len(w)} weights for {len(recons)} points")
    for i, r in enumerate(recons):
        if not r.is_contiguous():
            raise ValueError(f"multi_topk_loss: point {i} is not contiguous (shape {tuple(r.shape)}, strides {r.stride()})")
    losses, G = ops.trainer_loss(batch, [r.detach() for r in recons], 0, coef)
    for p, wp in enumerate(w):
        if wp != 1.0:
            G[p].mul_(wp)
    base = _levels_base(recons)
    if base is not None:                                      # one root: the [P, B, D] tensor the points are rows of
        roots, grads = [base], [G]
    else:
        roots, grads = list(recons), [G[i] for i in range(len(recons))]
    if sae_type == "b_sae":
        pol = outputs[2]
        roots.append(pol); grads.append(_const(batch.device, tuple(pol.shape), float(config["polarize_lambda"])))
    keep = [(r, g) for r, g in zip(roots, grads) if r.requires_grad]
    if keep:
        torch.autograd.backward([r for r, _ in keep], [g for _, g in keep])
    return losses
