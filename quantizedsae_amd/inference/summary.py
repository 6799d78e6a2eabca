"""The per-SAE summary block of scripts/analysis/summarize_stats.py: same function names and argument order, so that a
script switches by changing the import.

``average_coactivating_features`` reads ``coactivation > 0`` only (summarize_stats.py:37-70), so besides the [H, H]
int32 matrix it takes what ``analyze_dataset(..., coactivation="partners")`` returns: the per-feature partner counts or
the ``CoactivationPartners`` state.  A matrix is counted on the device in row slabs (``qsae_coactivation_partner_counts_dense``)
and never cloned; the reference clones it once per level.  Averages are the exact integer sum divided by the number of
selected features.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Union

import torch

from .. import torch_ops as T
from ..sae import QuantizedMatryoshkaSAE, ResidualQuantizedSAE
from .coactivation_partners import CoactivationPartners
from .token_overlap import average_unique_tokens_per_active_feature, top_token_sets

__all__ = ["summarize_activation_counts", "count_below_threshold", "average_coactivating_features", "level_sizes",
           "summarize_sae"]

_SLAB_BYTES = 256 << 20                 # a host matrix goes through the device in row slabs of about this size


def summarize_activation_counts(activation_counts: torch.Tensor) -> float:
    """Average activation count per feature (summarize_stats.py:22-24: the mean of the fp32 counts)."""
    return float(activation_counts.float().mean().item())


def count_below_threshold(activation_counts: torch.Tensor, threshold: int) -> int:
    """Number of features whose activation count is below ``threshold`` (summarize_stats.py:27-34)."""
    if activation_counts.numel() == 0:
        return 0
    return int((activation_counts < threshold).sum().item())


def _device_of(t: torch.Tensor) -> torch.device:
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("average_coactivating_features: a 2-D co-activation matrix is counted on MI355X only; "
                           f"tensor is on {t.device} and no device is present (no CPU fallback exists)")
    return torch.device("cuda", torch.cuda.current_device())


def _partner_counts_of_matrix(coactivation: torch.Tensor) -> torch.Tensor:
    """int64 [H] partner counts of an [H, H] count matrix, on the device, slab by slab"""
    if coactivation.shape[0] != coactivation.shape[1]:
        raise ValueError(f"coactivation: expected a square matrix, got {tuple(coactivation.shape)}")
    dev = _device_of(coactivation)
    if coactivation.dtype != torch.int32:
        raise TypeError(f"coactivation: expected dtype torch.int32, got {coactivation.dtype}")
    H = coactivation.shape[0]
    rows = max(1, min(H, _SLAB_BYTES // (4 * H)))
    parts = [T.coactivation_partner_counts_dense(coactivation[r:r + rows].to(dev), r) for r in range(0, H, rows)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def average_coactivating_features(coactivation: Union[torch.Tensor, CoactivationPartners], activation_counts: torch.Tensor,
                                  *, row_mask: Optional[torch.Tensor] = None) -> float:
    """summarize_stats.py:37-70: for each feature the number of distinct other features that co-activated with it at
    least once, averaged over the features with ``activation_counts > 0`` (and selected by ``row_mask``); 0.0 for an empty
    input, no active feature or an empty selection.  ``coactivation``: 1-D partner counts (pure torch, wherever they
    live), a ``CoactivationPartners``, or the 2-D int32 count matrix (counted on the device)."""
    if isinstance(coactivation, CoactivationPartners):
        per_feature = coactivation.counts()
    elif coactivation.numel() == 0 or activation_counts.numel() == 0:
        return 0.0
    elif coactivation.dim() == 1:
        per_feature = coactivation
    elif coactivation.dim() == 2:
        per_feature = _partner_counts_of_matrix(coactivation)
    else:
        raise ValueError("coactivation: expected 1-D partner counts, a 2-D count matrix or a CoactivationPartners")
    if activation_counts.numel() == 0:
        return 0.0
    active = activation_counts.to(per_feature.device).reshape(-1) > 0
    if row_mask is not None:
        active = active & row_mask.to(per_feature.device).reshape(-1)
    n = int(active.sum())
    if n == 0:
        return 0.0
    return int(per_feature.to(torch.int64)[active].sum()) / n


def level_sizes(sae) -> Optional[List[int]]:
    """Hidden sizes per level (summarize_stats.py:182-201): ``nested_dictionary_size`` of the matryoshka model,
    ``sae_hidden_dims`` of the residual model, None otherwise.  ``sae``: the wrapper or the model."""
    model = getattr(sae, "model", sae)
    if isinstance(model, QuantizedMatryoshkaSAE):
        return [int(s) for s in model.decoder.nested_dictionary_size]
    if isinstance(model, ResidualQuantizedSAE):
        return [int(s) for s in model.sae_hidden_dims]
    return None


def _block(activation_counts: torch.Tensor, partner_counts, token_sets, threshold: int, sl: Optional[slice]) -> Dict[str, Any]:
    act = activation_counts if sl is None else activation_counts[sl]
    row_mask = None
    if sl is not None:                   # rows restricted to the level, partners counted over all features
        row_mask = torch.zeros(activation_counts.shape, dtype=torch.bool)
        row_mask[sl] = True
    avg_tokens = None
    if token_sets is not None:
        part = token_sets if sl is None else type(token_sets)(token_sets.tokens[sl], token_sets.sizes[sl], token_sets.distinct[sl])
        avg_tokens = average_unique_tokens_per_active_feature(part, act)
    return {"mean_activation_count": summarize_activation_counts(act),
            "below_threshold": count_below_threshold(act, threshold),
            "avg_coactivating_features": None if partner_counts is None else
            average_coactivating_features(partner_counts, activation_counts, row_mask=row_mask),
            "avg_unique_tokens": avg_tokens}


def summarize_sae(stats: Dict[str, Any], level_sizes: Optional[Sequence[int]] = None, threshold: int = 1) -> Dict[str, Any]:
    """The summary of one SAE's statistics (summarize_stats.py:232-317) as a dict: ``mean_activation_count``,
    ``below_threshold``, ``avg_coactivating_features`` and ``avg_unique_tokens`` overall, and the same four per level under
    ``levels`` (a list, empty without ``level_sizes``).  ``stats``: what ``analyze_dataset`` / ``compute_activation_stats``
    return, or a loaded ``dynamic_stats_*.pt``.  The co-activation entry comes from ``coactivation_partner_counts`` when
    the stats hold them, else from the ``coactivation`` matrix (counted once, on the device), None when they hold
    neither; ``avg_unique_tokens`` is None without ``tokens_per_feature`` (Python lists or the CSR pair)."""
    activation_counts = stats["activation_counts"]
    partner_counts = stats.get("coactivation_partner_counts")
    if partner_counts is None and stats.get("coactivation") is not None:
        co = stats["coactivation"]
        partner_counts = _partner_counts_of_matrix(co) if co.numel() else co.reshape(-1)
    tokens = stats.get("tokens_per_feature")
    token_sets = None if tokens is None else top_token_sets(tokens, activation_counts, 1)
    out = _block(activation_counts, partner_counts, token_sets, threshold, None)
    out["levels"] = []
    start = 0
    for size in (level_sizes or ()):
        out["levels"].append(_block(activation_counts, partner_counts, token_sets, threshold, slice(start, start + int(size))))
        start += int(size)
    return out
