"""The strongest activations of every feature as streaming top-n lists on the device.

Reference: src/quantized_sae/utils/inspector.py -- ``feature_labeling`` builds its prompt from positions that
``print_feature_activations_overview`` collected from ``linguistic_analyze``, one Python tuple per token.  Here a
dataset streams through ``TopExamples`` batch by batch and what stays on the device is ``n`` 64-bit keys per feature
(``qsae_top_examples_*``, csrc/top_examples.hip): the order-preserving bits of the fp32 activation << 32 | ~position,
position = the global token index.  Larger activations win, equal activations go to the lower position, and the result
depends only on the set of (value, position) pairs, not on how the dataset was cut into batches.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from .. import torch_ops as T

__all__ = ["TopExamples", "examples_to_python"]


class TopExamples:
    """The ``n`` strongest activations (value > ``floor``) of each of ``H`` features over a dataset, on ``device``.

    ``add_compact`` takes the ``(idx, val)`` of ``forward_compact`` (the top-k models), ``add_dense`` a dense latent
    ``[B, H]`` (the ternary model's ReLU output, or any tensor); ``base`` is the global index of the batch's first row and
    positions must stay below 2^32.  ``finish()`` decodes the state: ``values`` fp32 [H, n] (descending, 0.0 past the
    end), ``positions`` int64 [H, n] (-1 past the end), ``counts`` int32 [H].  ``keys`` is the raw state, int64 [H, n]
    holding the bits of the unsigned keys (0 = none); no host read happens anywhere."""

    def __init__(self, H: int, n: int, device, floor: float = 0.0) -> None:
        H, n = int(H), int(n)
        if H <= 0:
            raise ValueError("H must be positive")
        if not 1 <= n <= T.TOP_EXAMPLES_MAX_N:
            raise ValueError(f"n must lie in 1 .. {T.TOP_EXAMPLES_MAX_N}, got {n}")
        floor = float(floor)
        if floor != floor:
            raise ValueError("floor must not be NaN")
        self.H, self.n, self.floor = H, n, floor
        self.device = torch.device(device)
        self.keys = torch.zeros((H, n), dtype=torch.int64, device=self.device)

    @staticmethod
    def _base(base: int, B: int) -> int:
        base = int(base)
        if base < 0 or base + int(B) > 2 ** 32:
            raise ValueError(f"positions are 32-bit: base + B <= 2^32 required, got base = {base}, B = {B}")
        return base

    def add_compact(self, idx: torch.Tensor, val: Optional[torch.Tensor], base: int) -> None:
        """One batch of a top-k model: ``idx`` int32 [B, k], ``val`` fp32 [B, k] or None (every entry at 1.0)."""
        T.top_examples_compact(idx, val, self.floor, self._base(base, idx.shape[0]), self.keys)

    def add_dense(self, latent: torch.Tensor, base: int) -> None:
        """One batch as a dense latent fp32 [B, H]."""
        T.top_examples_dense(latent, self.floor, self._base(base, latent.shape[0]), self.keys)

    def finish(self) -> Dict[str, torch.Tensor]:
        values, positions, counts = T.top_examples_decode(self.keys)
        return {"values": values, "positions": positions, "counts": counts}


def examples_to_python(result: Dict[str, Any], token_ids: torch.Tensor, tokens_per_context: int) -> List[List[Tuple[float, int, int, int]]]:
    """``finish()``'s result as, per feature, a list of ``(value, context, offset, token_id)``, strongest first: position
    g is token ``token_ids[g // tokens_per_context, g % tokens_per_context]`` (dynamic_analysis.py's row counter).  Three
    host copies."""
    tpc = int(tokens_per_context)
    values, positions = result["values"].cpu(), result["positions"].cpu()
    counts = result["counts"].cpu().tolist()
    ctx = torch.div(positions.clamp(min=0), tpc, rounding_mode="floor")
    off = positions.clamp(min=0) % tpc
    tok = token_ids.cpu()[ctx, off].tolist()
    values, ctx, off = values.tolist(), ctx.tolist(), off.tolist()
    return [[(values[f][j], ctx[f][j], off[f][j], tok[f][j]) for j in range(c)] for f, c in enumerate(counts)]
