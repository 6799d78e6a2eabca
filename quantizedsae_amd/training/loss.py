"""The per-type losses of the reference's loop (training/trainer.py:88-173) on the outputs of ``forward_train``: every
level's reconstruction loss and its gradient come from one pass of ``qsae_trainer_loss`` (csrc/trainer.hip); the L0 terms
and the polarize term are linear in an output, so their gradients are constants.  ``torch.autograd.backward`` is called on
the outputs directly: no loss tensor, no graph of loss arithmetic.

    type          reconstruction term                                   other terms
    q_sae         sum_i 0.5 mse(recon_i, x)                             sparsity_lambda * sum_i latent_group_i
    rq_sae        sum_i 0.5 mse(recon_i, t_i), t_0 = x,                 sparsity_lambda * w_i * latent_group_i,
                  t_{i+1} = ((t_i - recon_i).detach() * 2)              w = 1, 2.5, 4, 8 (no term from level 4 on)
    b_sae         0.5 mse(recon, x)                                     polarize_lambda * polarize_loss
    t_sae, baseline_sae, bl_sae    mse(recon, x)                        --
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .. import torch_ops as ops

__all__ = ["trainer_loss", "SAE_TYPES", "RQ_STAGE_WEIGHTS", "recon_recipe"]

SAE_TYPES = ("t_sae", "bl_sae", "b_sae", "q_sae", "rq_sae", "baseline_sae")
RQ_STAGE_WEIGHTS = (1.0, 2.5, 4.0, 8.0)

_consts: Dict[tuple, torch.Tensor] = {}


def _const(device: torch.device, shape: Tuple[int, ...], value: float) -> torch.Tensor:
    """A cached fp32 constant on the device (made by a fill kernel: no host copy, no synchronisation)."""
    key = (device.type, device.index, shape, float(value))
    t = _consts.get(key)
    if t is None:
        t = _consts[key] = torch.full(shape, float(value), dtype=torch.float32, device=device)
    return t


def _f32_product(a: float, b: float) -> float:
    """fl32(fl32(a) * b): the factor the reference's ``latent_group[i] * sparsity_lambda * w`` leaves at the latent group"""
    return float(torch.tensor(a, dtype=torch.float32) * b)


def recon_recipe(sae_type: str) -> Tuple[int, float]:
    """-> (mode, coef) of qsae_trainer_loss for the type's reconstruction term."""
    if sae_type not in SAE_TYPES:
        raise ValueError(f"unknown sae_type {sae_type!r}; expected one of {', '.join(SAE_TYPES)}")
    return (1 if sae_type == "rq_sae" else 0), (0.5 if sae_type in ("q_sae", "rq_sae", "b_sae") else 1.0)


def _levels_base(views):
    """The tensor whose rows the views are, when they are exactly its rows in order (what forward_train of the
    matryoshka classes hands out), else None."""
    base = views[0]._base
    if base is None or base.shape[0] != len(views) or not base.is_contiguous() or tuple(base.shape[1:]) != tuple(views[0].shape):
        return None
    step = base.stride(0) * base.element_size()
    for i, v in enumerate(views):
        if v._base is not base or v.data_ptr() != base.data_ptr() + i * step or tuple(v.shape) != tuple(base.shape[1:]):
            return None
    return base


def trainer_loss(sae_type: str, outputs, batch: torch.Tensor, config: dict, extra=None) -> torch.Tensor:
    """The loss of the type's recipe on ``outputs = model.forward_train(batch)``: returns the per-level reconstruction
    losses (fp32 [n] on the device; what the reference appends to ``recon_losses``, or its ``loss`` / ``recon_loss``) and
    runs ``torch.autograd.backward`` on the outputs the loss reads -- the kernel's gradients for the reconstructions, cached
    constants for the latent groups and the polarize loss.  Outputs the loss does not read get no gradient.  Nothing is
    read back to the host.  ``extra``: further ``(output, gradient)`` pairs of terms that are linear in an output (the L0
    term of JumpReLU), which join the same ``backward`` call."""
    mode, coef = recon_recipe(sae_type)
    if not batch.is_cuda:
        raise RuntimeError(f"trainer_loss: quantizedsae_amd runs on MI355X only; batch is on {batch.device} "
                           "(no CPU fallback exists)")
    roots, grads = [], []
    if sae_type in ("q_sae", "rq_sae"):
        groups, recons = list(outputs[0]), list(outputs[1])
        lam = float(config["sparsity_lambda"])
    elif sae_type == "b_sae":
        groups, recons = [], [outputs[1]]
    else:
        groups, recons = [], [outputs[1]]
    for i, r in enumerate(recons):
        if not r.is_contiguous():                             # no forward_train hands one out; a silent copy would be a [B, D] pass
            raise ValueError(f"trainer_loss: reconstruction {i} is not contiguous (shape {tuple(r.shape)}, strides {r.stride()})")
    detached = [r.detach() for r in recons]
    losses, G = ops.trainer_loss(batch, detached, mode, coef)
    if sae_type == "q_sae":
        base, gbase = _levels_base(recons), _levels_base(groups)
        if base is not None:                                  # one root: the [n, B, D] tensor the levels are rows of
            roots.append(base); grads.append(G)
        else:
            roots += recons; grads += [G[i] for i in range(len(recons))]
        if gbase is not None:
            roots.append(gbase); grads.append(_const(batch.device, (len(groups),), lam))
        else:
            roots += groups; grads += [_const(batch.device, tuple(g.shape), lam) for g in groups]
    elif sae_type == "rq_sae":
        for i, r in enumerate(recons):
            base = _levels_base([r])
            if base is not None:
                roots.append(base); grads.append(G[i:i + 1])
            else:
                roots.append(r); grads.append(G[i])
        for i, g in enumerate(groups[:len(RQ_STAGE_WEIGHTS)]):
            gbase = _levels_base([g])
            root = gbase if gbase is not None else g
            roots.append(root); grads.append(_const(batch.device, tuple(root.shape), _f32_product(lam, RQ_STAGE_WEIGHTS[i])))
    else:
        roots.append(recons[0]); grads.append(G[0])
        if sae_type == "b_sae":
            pol = outputs[2]
            roots.append(pol); grads.append(_const(batch.device, tuple(pol.shape), float(config["polarize_lambda"])))
    for root, grad in (extra or ()):
        roots.append(root); grads.append(grad)
    keep = [(r, g) for r, g in zip(roots, grads) if r.requires_grad]
    if keep:
        torch.autograd.backward([r for r, _ in keep], [g for _, g in keep])
    return losses
