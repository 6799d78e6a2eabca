"""The nested-dictionary (Matryoshka) objective for the two top-k models (Bussmann et al., "Learning Multi-Level Features with
Matryoshka Sparse Autoencoders"): one reconstruction per dictionary prefix, and a loss that sums the type's reconstruction
term over the prefixes.

    outputs = model.forward_train_nested(batch, bounds)       recon_l decodes the selected units below bounds[l]
    loss    = sum_l c * mse(recon_l, batch)  [+ polarize_lambda * polarize_loss for b_sae]       c = 0.5 (b_sae), 1 (baseline_sae)

Every level's loss and its gradient come from one pass of ``qsae_trainer_loss`` (mode 0, n = L); the levels are the rows of one
tensor, so ``torch.autograd.backward`` gets one root for them, and the backward of ``forward_train_nested`` turns the L
gradients into their suffix sums and runs the sparse backward once (csrc/nested.hip).  Nothing is read back to the host.
"""
from __future__ import annotations

import torch

from .. import torch_ops as ops
from ..sae.topk import TopKCore
from .loss import _const, _levels_base, recon_recipe

__all__ = ["nested_loss", "default_nested_bounds", "NESTED_TYPES"]

NESTED_TYPES = ("b_sae", "baseline_sae")
default_nested_bounds = TopKCore.default_nested_bounds


def nested_loss(sae_type: str, outputs, batch: torch.Tensor, config: dict) -> torch.Tensor:
    """The nested loss on ``outputs = model.forward_train_nested(batch, bounds)``: returns the per-level reconstruction losses
    (fp32 [L] on the device; their sum is the reconstruction part of the objective) and runs ``torch.autograd.backward`` on
    the outputs the loss reads -- the kernel's gradients for the levels, a cached constant for the polarize loss of
    ``b_sae``."""
    if sae_type not in NESTED_TYPES:
        raise ValueError(f"nested_loss: the nested objective is built for baseline_sae and b_sae, the two top-k models; got "
                         f"{sae_type!r}")
    if not batch.is_cuda:
        raise RuntimeError(f"nested_loss: quantizedsae_amd runs on MI355X only; batch is on {batch.device} "
                           "(no CPU fallback exists)")
    _, coef = recon_recipe(sae_type)
    recons = list(outputs[1])
    if not 1 <= len(recons) <= ops.NESTED_MAX_LEVELS:
        raise ValueError(f"nested_loss: {len(recons)} levels; 1 .. {ops.NESTED_MAX_LEVELS} are supported")
    for i, r in enumerate(recons):
        if not r.is_contiguous():
            raise ValueError(f"nested_loss: level {i} is not contiguous (shape {tuple(r.shape)}, strides {r.stride()})")
    losses, G = ops.trainer_loss(batch, [r.detach() for r in recons], 0, coef)
    base = _levels_base(recons)
    if base is not None:                                      # one root: the [L, B, D] tensor the levels are rows of
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
