"""What ``wandb.watch(model, log="all", log_freq=256)`` shows of a run (the reference's training/trainer.py:51): a 64-bin
histogram of every parameter and of every gradient -- here from one kernel call over all of them (``qsae_tensor_stats``,
csrc/watch.hip) and one small host copy, instead of wandb's isfinite / min / max / histc / tolist per tensor with its three
host synchronisations each.

Per tensor the recipe is wandb's ``log_tensor_stats``: the non-finite elements are dropped, ``lo`` and ``hi`` are the minimum
and maximum of the rest, the counts are ``torch.histc(flat, bins, lo, hi)`` as the CPU computes them and the edges
``torch.linspace(lo, hi, bins + 1)``; a tensor without a finite element has no histogram.  On top of that come the numbers
the reference's utils/encoder_debug.py collects by hand: mean, std, min, max, and the counts of zero and non-finite elements.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

from .. import torch_ops as ops

__all__ = ["TensorStats", "tensor_stats", "ModelWatch", "WATCH_MODES", "watch_line"]

WATCH_MODES = ("all", "parameters", "gradients")
_HEAD = 8


@dataclass
class TensorStats:
    """The distribution of one tensor.  ``counts`` int64 [bins] (host); ``lo`` / ``hi`` the exact fp32 minimum and maximum of
    the finite elements as Python floats; ``mean`` and ``std`` (``torch.std``'s: n - 1 below the root) from fp64 sums over the
    finite elements.  With ``n_finite == 0`` the counts are zero and lo, hi, mean are 0.0, std NaN."""
    counts: torch.Tensor
    lo: float
    hi: float
    n_finite: int
    n_nonfinite: int
    n_zero: int
    mean: float
    std: float

    @property
    def bins(self) -> int:
        return int(self.counts.numel())

    @property
    def edges(self) -> torch.Tensor:
        """fp32 [bins + 1]: ``torch.linspace(lo, hi, bins + 1)``, the edges wandb logs (of [lo, hi] also where lo == hi)"""
        return torch.linspace(self.lo, self.hi, steps=self.bins + 1)

    def np_histogram(self) -> Tuple[list, list]:
        """-> (counts list, edges list): the pair ``wandb.Histogram(np_histogram=...)`` takes"""
        return self.counts.tolist(), self.edges.tolist()


def _parse(block: torch.Tensor) -> List[TensorStats]:
    """block: the int64 [T, 8 + bins] result of ops.tensor_stats on the host"""
    f = block[:, :4].contiguous().view(torch.float64)
    out = []
    for t in range(block.shape[0]):
        lo, hi, mean, m2 = f[t].tolist()
        n_finite, n_nonfinite, n_zero = block[t, 4:7].tolist()
        std = math.sqrt(m2 / (n_finite - 1)) if n_finite > 1 else float("nan")
        out.append(TensorStats(block[t, _HEAD:].clone(), lo, hi, n_finite, n_nonfinite, n_zero, mean, std))
    return out


def tensor_stats(tensors, bins: int = 64) -> List[TensorStats]:
    """The distribution of every tensor of a list (fp32, contiguous, on the GPU; any shapes): one kernel call and one host copy
    for the whole list."""
    return _parse(ops.tensor_stats(list(tensors), bins).cpu())


class ModelWatch:
    """``ModelWatch(model, log="all").collect()`` -> ``{"parameters/<name>": TensorStats, "gradients/<name>": TensorStats}``
    over ``model.named_parameters()``, wandb's keys.  ``log``: "all", "parameters" or "gradients".  A parameter whose ``.grad``
    is None has no gradient entry, a tensor without a finite element no entry at all (wandb returns without logging it).  One
    kernel call covers the parameters and the gradients together."""

    def __init__(self, model: torch.nn.Module, log: str = "all", bins: int = 64):
        if log not in WATCH_MODES:
            raise ValueError(f"ModelWatch: log must be one of {', '.join(WATCH_MODES)}, got {log!r}")
        if not 1 <= int(bins) <= 256:
            raise ValueError(f"ModelWatch: bins must be in 1 .. 256, got {bins}")
        self.model, self.log, self.bins = model, log, int(bins)

    def _tensors(self):
        keys, tensors = [], []
        for name, p in self.model.named_parameters():
            if self.log in ("all", "parameters"):
                keys.append("parameters/" + name)
                tensors.append(p.detach())
            if self.log in ("all", "gradients") and p.grad is not None:
                keys.append("gradients/" + name)
                tensors.append(p.grad.detach())
        for key, t in zip(keys, tensors):
            if not t.is_cuda:
                raise RuntimeError(f"ModelWatch: quantizedsae_amd runs on MI355X only; {key} is on {t.device} "
                                   "(no CPU fallback exists)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"ModelWatch: {key} must be a contiguous fp32 tensor, got {t.dtype} {tuple(t.shape)} with "
                                 f"strides {t.stride()} (no silent copy is made)")
        return keys, tensors

    def collect(self) -> Dict[str, TensorStats]:
        keys, tensors = self._tensors()
        if not tensors:
            return {}
        return {k: s for k, s in zip(keys, tensor_stats(tensors, self.bins)) if s.n_finite > 0}


def watch_line(key: str, s: TensorStats) -> str:
    """One printed line per tensor: name, n, min, max, mean, std, zeros, non-finite"""
    return (f"  {key}: n={s.n_finite + s.n_nonfinite}, min={s.lo:.6g}, max={s.hi:.6g}, mean={s.mean:.6g}, std={s.std:.6g}, "
            f"zeros={s.n_zero}, non_finite={s.n_nonfinite}")
