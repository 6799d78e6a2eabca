"""Token-overlap (Jaccard) comparison of two SAEs from the ``tokens_per_feature`` lists of ``analyze_dataset``.

Reference: scripts/analysis/summarize_stats.py -- ``_topk_token_set`` (:100-105), ``jaccard_between_saes`` (:108-156:
for every pair of live features, the ``k_tokens`` most frequent tokens of each, scored |A & B| / |A | B|), the report of
``main`` (:320-378: the mean over all pairs and the means of the 10 / 100 / 1000 / 10000 highest scores) and
``average_unique_tokens_per_active_feature`` (:73-97).  The reference is a Python double loop over ``set`` objects that
appends one float per pair; here the sets become packed bitsets, the intersections of all pairs one int8-MFMA product
(``qsae_token_overlap_hist``, csrc/token_overlap.hip), and the result the table of (intersection, union) counts, from
which the mean and every top-n mean follow exactly.

The top-token sets are plumbing (torch sorts, on the device or the host); the pair loop is the kernel, device only.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import torch_ops as T

__all__ = ["TokenSets", "JaccardHistogram", "top_token_sets", "average_unique_tokens_per_active_feature",
           "jaccard_histogram"]

TokenLists = Union[Sequence[Sequence[int]], Tuple[torch.Tensor, torch.Tensor]]


@dataclass
class TokenSets:
    """Top-token sets of the N features of one SAE.  ``tokens`` int64 [N, k]: the set of feature i in
    ``tokens[i, :sizes[i]]``, most frequent first, -1 beyond; ``sizes`` int64 [N], 0 = no set (a never-active feature
    or an empty list); ``distinct`` int64 [N]: distinct tokens in the feature's whole list, whatever its activity."""
    tokens: torch.Tensor
    sizes: torch.Tensor
    distinct: torch.Tensor


def _csr(tokens_per_feature: TokenLists, device) -> Tuple[torch.Tensor, torch.Tensor]:
    if isinstance(tokens_per_feature, tuple) and len(tokens_per_feature) == 2 and all(
            isinstance(t, torch.Tensor) for t in tokens_per_feature):
        offsets, tokens = tokens_per_feature
        if offsets.dim() != 1 or offsets.numel() < 1 or tokens.dim() != 1:
            raise ValueError("tokens_per_feature: a CSR pair is (offsets int64 [N + 1], tokens int64 [nnz])")
        device = tokens.device if device is None else device
        return offsets.to(device=device, dtype=torch.int64), tokens.to(device=device, dtype=torch.int64)
    lengths = torch.tensor([len(t) for t in tokens_per_feature], dtype=torch.int64)
    offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    tokens = torch.tensor([t for lst in tokens_per_feature for t in lst], dtype=torch.int64)
    return offsets.to(device or "cpu"), tokens.to(device or "cpu")


def top_token_sets(tokens_per_feature: TokenLists, activation_counts: torch.Tensor, k_tokens: int, *,
                   device=None) -> TokenSets:
    """The sets ``jaccard_between_saes`` compares: for a feature with ``activation_counts > 0`` the ``k_tokens`` tokens
    with the highest count in its list, ties going to the token that occurs first in the list (the order of
    ``Counter.most_common``); no set for a never-active feature, whatever its list holds, nor for an empty list.

    ``tokens_per_feature``: the list of lists of ``dynamic_stats_*.pt`` or a CSR pair (offsets int64 [N + 1], tokens
    int64 [nnz]).  Runs where the CSR tensors live (``device`` moves them): two sorts and a ``unique_consecutive``."""
    k = int(k_tokens)
    if k <= 0:
        raise ValueError("k_tokens must be positive")
    offsets, tokens = _csr(tokens_per_feature, device)
    dev = tokens.device
    N = offsets.numel() - 1
    active = torch.as_tensor(activation_counts).to(dev).reshape(-1) > 0
    if active.numel() != N:
        raise ValueError(f"activation_counts: expected {N} entries, got {active.numel()}")
    out = torch.full((N, k), -1, dtype=torch.int64, device=dev)
    if tokens.numel() == 0:
        zero = torch.zeros(N, dtype=torch.int64, device=dev)
        return TokenSets(out, zero, zero.clone())
    if int(tokens.min()) < 0:
        raise ValueError("tokens_per_feature: token ids must be non-negative")
    span = int(tokens.max()) + 1
    lengths = offsets[1:] - offsets[:-1]
    feature = torch.repeat_interleave(torch.arange(N, device=dev), lengths)
    # groups of equal (feature, token); the sort is stable, so the first entry of a group is its first occurrence
    key, order = torch.sort(feature * span + tokens, stable=True)
    group, count = torch.unique_consecutive(key, return_counts=True)
    first = order[torch.cumsum(count, 0) - count]
    gfeat, gtok = group // span, group % span
    distinct = torch.bincount(gfeat, minlength=N)
    # within a feature: count descending, then first occurrence ascending (stable sorts, least significant key first)
    o = torch.argsort(first, stable=True)
    o = o[torch.argsort(count[o], descending=True, stable=True)]
    o = o[torch.argsort(gfeat[o], stable=True)]
    gfeat, gtok = gfeat[o], gtok[o]
    rank = torch.arange(gfeat.numel(), device=dev) - (torch.cumsum(distinct, 0) - distinct)[gfeat]
    keep = (rank < k) & active[gfeat]
    out[gfeat[keep], rank[keep]] = gtok[keep]
    sizes = torch.where(active, distinct.clamp(max=k), torch.zeros_like(distinct))
    return TokenSets(out, sizes, distinct)


def average_unique_tokens_per_active_feature(token_sets: TokenSets, activation_counts: torch.Tensor) -> float:
    """summarize_stats.py:73-97: the mean number of distinct tokens over the features that activated at least once
    (0.0 when there is none) -- a by-product of the sort behind ``top_token_sets``."""
    active = torch.as_tensor(activation_counts).to(token_sets.distinct.device).reshape(-1) > 0
    n = int(active.sum())
    return float(int(token_sets.distinct[active].sum()) / n) if n else 0.0


class JaccardHistogram:
    """Every pair's score as counts of (intersection, union): ``counts[i, u]`` pairs scored ``i / u`` (``0.0`` for
    i == 0).  int64 [k + 1, 2k + 1] on the host; ``n_pairs`` = their sum = the length of the reference's score list."""

    def __init__(self, counts: torch.Tensor, n_pairs: Optional[int] = None):
        self.counts = counts.to(device="cpu", dtype=torch.int64)
        self.n_pairs = int(self.counts.sum()) if n_pairs is None else int(n_pairs)
        nz = self.counts.nonzero().tolist()
        # (score, count), highest score first; the score is the reference's own float: inter / union, 0.0 when disjoint
        self._bins = sorted(((i / u if i else 0.0, int(self.counts[i, u])) for i, u in nz), key=lambda b: -b[0])

    def mean(self) -> Optional[float]:
        """The mean of all scores: the exact sum of the pairs' floats, rounded once, over their number (what
        ``math.fsum(scores) / len(scores)`` gives)."""
        if not self.n_pairs:
            return None
        return float(sum(Fraction(s) * c for s, c in self._bins)) / self.n_pairs

    def top(self, n: int) -> List[float]:
        """The n highest scores in descending order (``heapq.nlargest(n, scores)``)."""
        out: List[float] = []
        for s, c in self._bins:
            if len(out) >= n:
                break
            out.extend([s] * min(c, n - len(out)))
        return out

    def top_mean(self, n: int) -> Tuple[Optional[float], int]:
        """(mean of the n highest scores, how many there were): ``sum(nlargest(n, scores)) / len``, summed in descending
        order as summarize_stats.py:341-349 does."""
        vals = self.top(n)
        return (float(sum(vals) / len(vals)) if vals else None), len(vals)

    def summary(self, tops: Sequence[int] = (10, 100, 1000, 10000)) -> Dict[str, Any]:
        """The numbers of the script's Jaccard block: {"n_pairs", "mean", "top": {n: (mean, used)}}."""
        return {"n_pairs": self.n_pairs, "mean": self.mean(), "top": {int(n): self.top_mean(int(n)) for n in tops}}


def _pack(tokens: torch.Tensor, words: int) -> torch.Tensor:
    """int32 [N, words] bitsets of the padded sets ``tokens`` (-1 = nothing): bit t & 31 of word t >> 5.  The tokens of
    a row are distinct, so summing their bit masks is or-ing them."""
    N = tokens.shape[0]
    row, col = (tokens >= 0).nonzero(as_tuple=True)
    t = tokens[row, col]
    acc = torch.zeros(N * words, dtype=torch.int64, device=tokens.device)
    acc.index_add_(0, row * words + (t >> 5), torch.ones_like(t) << (t & 31))
    return acc.to(torch.int32).view(N, words)           # keeps the low 32 bits


def jaccard_histogram(stats_a: Dict[str, Any], stats_b: Dict[str, Any], k_tokens: int = 100, *, device=None,
                      compact: bool = True) -> JaccardHistogram:
    """``jaccard_between_saes(stats_a, stats_b, k_tokens)`` as a histogram.  ``stats_*``: dicts with
    ``tokens_per_feature`` (list of lists or CSR pair) and ``activation_counts``, as ``analyze_dataset`` returns them.

    ``compact`` (default) renumbers the tokens that occur in sets of both sides and drops the others before packing:
    only those can be in an intersection, and the true sizes travel separately, so this shortens the contraction and
    changes nothing else.  ``compact=False`` packs over the whole range of token ids.  Raises when the table does not
    account for every pair of live features."""
    k = int(k_tokens)
    if not 1 <= k <= 128:
        raise ValueError("jaccard_histogram: 1 <= k_tokens <= 128 (the kernel's table lives in LDS)")
    dev = torch.device("cuda" if device is None else device)
    sets = [top_token_sets(s["tokens_per_feature"], s["activation_counts"], k, device=dev) for s in (stats_a, stats_b)]
    toks = [s.tokens for s in sets]
    present = [torch.unique(t[t >= 0]) for t in toks]
    if compact:
        both, seen = torch.unique(torch.cat(present), return_counts=True)
        common = both[seen == 2]                          # sorted token ids that occur on both sides
        V = max(int(common.numel()), 1)
        for i, t in enumerate(toks):
            if common.numel():
                pos = torch.searchsorted(common, t.clamp(min=0)).clamp(max=common.numel() - 1)
                toks[i] = torch.where((t >= 0) & (common[pos] == t), pos, torch.full_like(t, -1))
            else:
                toks[i] = torch.full_like(t, -1)
    else:
        V = max([int(p.max()) + 1 for p in present if p.numel()] + [1])
    words = (V + 31) // 32
    sizes = [s.sizes.to(torch.int32) for s in sets]
    hist = T.token_overlap_hist(_pack(toks[0], words), sizes[0], _pack(toks[1], words), sizes[1], V, k)
    live = int((sizes[0] > 0).sum()) * int((sizes[1] > 0).sum())
    result = JaccardHistogram(hist)
    if result.n_pairs != live:
        raise RuntimeError(f"token_overlap_hist counted {result.n_pairs} of {live} live pairs")
    return result
