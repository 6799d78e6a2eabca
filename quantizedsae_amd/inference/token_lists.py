"""Tokens per feature as ordered CSR lists on the device.

Reference: scripts/analysis/dynamic_analysis.py:283-306 -- a global row counter g runs over the batches, row g has token
``token_ids[g // tokens_per_context, g % tokens_per_context]``, and ``tokens_per_feature[f]`` collects the tokens of the
rows whose mask bit f is set, in ascending g (the order of ``mask.nonzero()``).  The reference extends H Python lists one
activation at a time; here a batch becomes per-feature lists by prefix counts over a row bitmap (``qsae_token_lists_*``,
csrc/token_lists.hip), from the compact ``(idx, val)`` of the top-k models or the packed bits of the threshold models,
and ``finish()`` joins the batches feature-major.  The result is the CSR pair that ``top_token_sets`` /
``jaccard_histogram`` take as they are; memory is proportional to the number of activations.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from .. import torch_ops as T

__all__ = ["TokenLists", "token_lists_to_python", "check_token_ids"]


def check_token_ids(token_ids: torch.Tensor) -> None:
    """Token ids are stored as int32: anything outside [0, 2^31) raises ValueError (one pass over ``token_ids``)."""
    if token_ids.numel() and (int(token_ids.min()) < 0 or int(token_ids.max()) >= 2 ** 31):
        raise ValueError("token_ids: token ids must lie in [0, 2^31)")


class TokenLists:
    """Accumulates ``tokens_per_feature`` of H features over the batches of a dataset, on ``device``.

    ``add_compact`` / ``add_bits`` take one batch each, in dataset order, with ``row_tokens`` [B] the token id of every
    row of the batch; ``finish()`` returns ``(offsets int64 [H + 1], tokens int32 [nnz])``.  One host read per batch (its
    entry count, which sizes its token buffer)."""

    def __init__(self, H: int, device) -> None:
        if int(H) <= 0:
            raise ValueError("H must be positive")
        self.H = int(H)
        self.device = torch.device(device)
        self._offsets: List[torch.Tensor] = []
        self._tokens: List[torch.Tensor] = []

    def _row_tokens(self, row_tokens: torch.Tensor, B: int) -> torch.Tensor:
        if row_tokens.shape != (B,):
            raise ValueError(f"row_tokens: expected [{B}] entries, got {tuple(row_tokens.shape)}")
        return row_tokens.to(device=self.device, dtype=torch.int32)

    def _add(self, offsets: torch.Tensor, workspace: torch.Tensor, row_tokens: torch.Tensor) -> None:
        n = int(offsets[-1])                                 # the batch's one host read
        self._offsets.append(offsets)
        self._tokens.append(T.token_lists_fill(workspace, offsets, row_tokens, n))

    def add_compact(self, idx: torch.Tensor, val: Optional[torch.Tensor], row_tokens: torch.Tensor) -> None:
        """One batch of a top-k model: ``idx`` int32 [B, k], ``val`` fp32 [B, k] (active = val > 0) or None."""
        rt = self._row_tokens(row_tokens, idx.shape[0])
        self._add(*T.token_lists_count(idx, val, self.H), rt)

    def add_bits(self, zbits: torch.Tensor, index: Optional[torch.Tensor], row_tokens: torch.Tensor) -> None:
        """One batch of a threshold model: ``zbits`` int32 [B, words] and the packed-position -> unit map ``index`` (None =
        identity), the pair that goes to ``coactivation_bits``."""
        rt = self._row_tokens(row_tokens, zbits.shape[0])
        self._add(*T.token_lists_count_bits(zbits, self.H, index), rt)

    def finish(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if not self._offsets:
            return (torch.zeros((self.H + 1,), dtype=torch.int64, device=self.device),
                    torch.zeros((0,), dtype=torch.int32, device=self.device))
        if len(self._offsets) == 1:                          # already feature-major
            return self._offsets[0], self._tokens[0]
        return T.token_lists_regroup(torch.stack(self._offsets), torch.cat(self._tokens))


def token_lists_to_python(offsets: torch.Tensor, tokens: torch.Tensor) -> List[List[int]]:
    """The CSR pair as the reference's list of H lists (what a ``dynamic_stats_*.pt`` file holds): two host copies and
    H slices."""
    bounds = offsets.cpu().tolist()
    flat = tokens.cpu().tolist()
    return [flat[bounds[f]:bounds[f + 1]] for f in range(len(bounds) - 1)]
