"""``quantizedsae_amd.optim.Adam``: the optimizer step in HIP (csrc/optim.hip).

A drop-in for ``torch.optim.Adam(model.parameters(), lr=...)`` (training/trainer.py:68): every parameter is stepped by one
pass of ``torch.ops.qsae.adam_step``.  With ``model=`` set to one of the top-k models (BinarySAE, BaselineSparseAutoencoder)
the encoder's weight and bias are stepped together by ``torch.ops.qsae.adam_step_prefilter``, which also leaves the fp16
candidate-pass copy of the new weights; the optimizer installs it in the model's cache, so the next forward does not
rebuild it.  The state (``step``, ``exp_avg``, ``exp_avg_sq``) has the names, dtypes and placement of torch's non-capturable
Adam: state dicts go back and forth between the two.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import torch_ops as ops
from .sae.topk import TopKCore

__all__ = ["Adam"]

# options of torch.optim.Adam that have no kernel here; kept in the param groups (off) so that state dicts stay
# interchangeable
_UNSUPPORTED = ("weight_decay", "amsgrad", "maximize", "capturable", "differentiable", "fused")


def _check_group(group: dict) -> None:
    for name in _UNSUPPORTED:
        if group.get(name):
            raise ValueError(f"quantizedsae_amd.optim.Adam does not support {name} (got {name}={group[name]!r})")
    lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
    if isinstance(lr, torch.Tensor):
        raise ValueError("quantizedsae_amd.optim.Adam takes lr as a Python float (a tensor lr belongs to capturable)")
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
        raise ValueError(f"Invalid betas: {(b1, b2)}")


class Adam(torch.optim.Optimizer):
    """Adam (no weight decay, amsgrad or maximize) with the step in HIP.

    ``model``: the SAE whose parameters these are.  For a top-k model the encoder pair takes the fused route in every step
    in which encoder weight and bias are both in this optimizer with the same lr / betas / eps and step count, both have
    a gradient, and the weight is 16-byte aligned; in any other step, and for any other model class, every parameter
    goes through the plain kernel and the model's caches notice the new version counters by themselves.

    The keyword-only options after ``model`` are torch.optim.Adam's and exist so that the param groups carry torch's keys
    (state dicts load both ways): a truthy ``weight_decay``, ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``
    or ``fused`` is a ``ValueError`` that names it (``fused`` also because torch reads it from a loaded state dict to place
    ``step`` on the device); ``foreach`` has no meaning here -- there is one implementation -- and is kept as given."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, *, model: Optional[torch.nn.Module] = None,
                 weight_decay: float = 0, amsgrad: bool = False, maximize: bool = False, foreach: Optional[bool] = None,
                 capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=False)
        _check_group(defaults)
        self._model = model if isinstance(model, TopKCore) else None
        super().__init__(params, defaults)

    def add_param_group(self, param_group: dict) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _check_group(group)
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise ValueError(f"quantizedsae_amd.optim.Adam steps fp32 parameters (got {p.dtype})")
                if not p.is_contiguous():
                    raise ValueError("quantizedsae_amd.optim.Adam steps contiguous parameters "
                                     f"(got shape {tuple(p.shape)}, strides {p.stride()})")
        except ValueError:
            self.param_groups.pop()
            raise

    def _state_of(self, p):
        state = self.state[p]
        if len(state) == 0:
            # a host scalar, fp32 (fp64 under a float64 default dtype): where torch's non-capturable Adam keeps it
            state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64
                                         else torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    @staticmethod
    def _scalars(group, t: float):
        """The six scalars of step t in Python floats, as torch's single-tensor Adam computes them."""
        lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
        return (1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** t), eps, lr / (1 - b1 ** t))

    def _encoder_pair(self, todo):
        """-> (weight, bias) when this step's encoder pair qualifies for the fused route, else None.  ``todo`` maps a
        parameter with a gradient to its group."""
        if self._model is None:
            return None
        lin = self._model.encoder.linear
        W, b = lin.weight, getattr(lin, "bias", None)
        if b is None or W not in todo or b not in todo:
            return None
        gW, gb = todo[W], todo[b]
        if (gW["lr"], tuple(gW["betas"]), gW["eps"]) != (gb["lr"], tuple(gb["betas"]), gb["eps"]):
            return None
        sW, sb = self.state.get(W), self.state.get(b)
        tW = float(sW["step"]) if sW else 0.0
        tb = float(sb["step"]) if sb else 0.0
        if tW != tb or W.dim() != 2 or W.data_ptr() % 16 != 0 or tuple(b.shape) != (W.shape[0],):
            return None
        return W, b

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = {}
        for group in self.param_groups:
            _check_group(group)                        # a loaded state dict may have brought other options
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("quantizedsae_amd.optim.Adam does not support sparse gradients")
                if not p.is_cuda:
                    raise RuntimeError(f"quantizedsae_amd.optim.Adam runs on MI355X only; a parameter is on {p.device} "
                                       "(no CPU fallback exists)")
                todo[p] = group
        pair = self._encoder_pair(todo)
        for p, group in todo.items():
            if pair is not None and p is pair[1]:
                continue                               # the bias goes with its weight
            state = self._state_of(p)
            state["step"] += 1
            scalars = self._scalars(group, float(state["step"]))
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            if pair is not None and p is pair[0]:
                self._step_pair(pair[1], g, state, scalars)
            else:
                ops.adam_step(p.detach(), g, state["exp_avg"], state["exp_avg_sq"], *scalars)
        return loss

    def _step_pair(self, b, gW, stateW, scalars) -> None:
        model = self._model
        lin = model.encoder.linear
        W = lin.weight
        stateb = self._state_of(b)
        stateb["step"] += 1
        gb = b.grad if b.grad.is_contiguous() else b.grad.contiguous()
        # the buffers of the copy that is about to go stale take the new one (work on one stream is ordered)
        Wq = meta = None
        old = model._pref_cache.peek()
        if isinstance(old, dict) and isinstance(old.get("Wq"), torch.Tensor) and isinstance(old.get("meta"), torch.Tensor):
            oq, om = old["Wq"], old["meta"]
            if oq.shape == W.shape and oq.dtype == torch.float16 and oq.device == W.device and oq.is_contiguous() \
                    and oq.data_ptr() % 16 == 0 and tuple(om.shape) == (4,) and om.dtype == torch.float32 \
                    and om.device == W.device:
                Wq, meta = oq, om
        Wq, meta = ops.adam_step_prefilter(W.detach(), gW, stateW["exp_avg"], stateW["exp_avg_sq"], b.detach(), gb,
                                           stateb["exp_avg"], stateb["exp_avg_sq"], *scalars, Wq=Wq, meta=meta)
        # after the op: its writes have moved the version counters that the cache key reads
        model._pref_cache.put((lin.weight, lin.bias), {"Wq": Wq, "meta": meta})
