"""Reconstruction error per dictionary prefix of a top-k SAE (the levels a nested-dictionary model is read in): one selection
and one walk over each row's list per batch (``forward_nested``, csrc/nested.hip), one ``DatasetMoments`` per level.  The last
level is the model's own reconstruction, so its numbers equal ``evaluate_dataset``'s exactly.  With ``threshold=`` the selection
is that of a BatchTopK model at inference (``forward_nested_threshold``, csrc/nested_ragged.hip): every entry at or above the
learned threshold, a ragged number per row."""
from __future__ import annotations

from typing import Any, Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from ..sae.baseline import BaselineSparseAutoencoder
from ..sae.binary import BinarySAE
from ..sae.topk import TopKCore
from .evaluation import DatasetMoments, _rows
from .framework import SAEWrapper

__all__ = ["nested_errors"]


def nested_errors(sae, loader: Iterable[Any], bounds: Optional[Sequence[int]] = None, group_rows: int = 1024, *,
                  threshold=None, cap: Optional[int] = None) -> Dict[str, Any]:
    """One pass over a loader of batches ``[rows, D]``: -> ``bounds``, ``mse`` and ``fvu`` (numpy fp64 [L], level l decoding
    the selected units below ``bounds[l]``), ``variance``, ``rows``, ``skipped_rows`` and ``levels``, the L results of
    ``DatasetMoments.finish()``.  ``sae``: a ``BinarySAE`` or ``BaselineSparseAutoencoder`` or an ``SAEWrapper`` around one;
    ``bounds`` defaults to ``default_nested_bounds(hidden_dim)`` = ``[H/8, H/4, H/2, H]``.

    ``threshold`` (a ``training.BatchTopK`` or a number; ``cap`` as in ``forward_threshold``) evaluates through
    ``forward_nested_threshold`` instead of the model's own top-k and adds ``l0`` (numpy fp64 [L]: the mean number of selected
    units below ``bounds[l]`` per row, over all rows of the loader) and ``threshold`` (the number) to the result; the sums stay
    on the device until the end."""
    model = sae.model if isinstance(sae, SAEWrapper) else sae
    if not isinstance(model, (BinarySAE, BaselineSparseAutoencoder)):
        raise TypeError(f"nested_errors: expected a BinarySAE or a BaselineSparseAutoencoder, got {type(model).__name__}: the "
                        "dictionary prefixes are read from a top-k list, and the sparsity of the other classes is not a k; "
                        "compute_reconstruction_error_by_level gives the matryoshka levels")
    if isinstance(sae, SAEWrapper):
        sae.eval()
    H, D = model.encoder.linear.weight.shape
    device = model.encoder.linear.weight.device
    if bounds is None:
        bounds = TopKCore.default_nested_bounds(H)
    if cap is not None and threshold is None:
        raise ValueError("nested_errors: cap goes with threshold")
    moments, below, rows = None, None, 0
    for batch in loader:
        x = _rows(batch).to(device)
        if threshold is None:
            _, _, levels = model.forward_nested(x, bounds)      # validates x and the bounds
        else:
            _, _, _, levels, counts_below = model._nested_threshold(x, threshold, bounds, cap)
            sums = counts_below.sum(dim=1, dtype=torch.int64)
            below, rows = (sums if below is None else below + sums), rows + x.shape[0]
        if moments is None:
            moments = [DatasetMoments(D, group_rows, device) for _ in range(levels.shape[0])]
        for l, m in enumerate(moments):
            m.add(x, levels[l])
    if moments is None:
        raise ValueError("empty loader")
    results = [m.finish() for m in moments]
    last = results[-1]
    extra = {}
    if threshold is not None:
        extra = {"l0": below.to(torch.float64).cpu().numpy() / max(rows, 1),
                 "threshold": threshold.threshold() if hasattr(threshold, "threshold") else float(threshold)}
    return {**extra, "bounds": [int(b) for b in bounds], "mse": np.array([r["mse"] for r in results], dtype=np.float64),
            "fvu": np.array([r["fvu"] for r in results], dtype=np.float64), "variance": last["variance"], "rows": last["rows"],
            "skipped_rows": last["skipped_rows"], "levels": results}

