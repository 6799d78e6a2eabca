"""Inspection of a dictionary on the GPU: the k nearest atoms of every atom, duplicates, value counts.

Reference: src/quantized_sae/utils/inspector.py (``TernarySparseAutoencoderInspector``).  Its nearest-feature query
forms the [H, H] fp32 cosine matrix with ``torch.mm``, copies it to numpy and hands it to sklearn; here one call of
``qsae_nearest_atoms_i8`` (csrc/dictionary_neighbors.hip) contracts the int8 atoms on the matrix pipe and keeps k keys
per row, so no [H, H] matrix exists.  The dictionaries are integers (ternary {-1, 0, +1}; BinarySAE's n-bit two's
complement table), so every dot product and every squared norm is exact and the ranking needs no tolerance: the
arithmetic is spelled out in DESIGN.md 4.18.  Two deliberate differences from the reference: the k columns are
returned and not the matrix, and equal cosines are ordered by the lowest index (sklearn's order there is unspecified).
fp32 dictionaries (baseline, matryoshka, residual, a BinarySAE wider than 8 bits, or any pair with one such side) take
``qsae_nearest_atoms_f32`` (csrc/dictionary_neighbors_f32.hip): the same keys from the exact-fp32 contraction that
``compare_decoders`` uses, k per row instead of one.  ``k_means_analysis`` clusters the atoms with
``kmeans_atoms`` (inference/clustering.py) in place of ``kmeans_pytorch`` on the CPU.
The activation side of the reference's ``linguistic_*`` block (``linguistic_analyze``,
``print_feature_activations_overview``, ``check_sensitivity`` / ``check_specificity``) runs on the device too, with
``top_examples`` for the strongest activations per feature; ``evaluate_feature`` and ``feature_labeling``
call an external API and are not ported.
"""
from __future__ import annotations

from typing import Any, Dict, Iterator, List, Sequence, Tuple

import torch

from .. import torch_ops as T
from ..sae.base import HipEncoder
from ..sae.binary import BinarySAE
from ..sae.ternary import STEWeights, TernarySparseAutoencoder
from .dictionary import _decode_keys, _model, decoder_atoms
from .token_lists import TokenLists
from .top_examples import TopExamples

__all__ = ["integer_atoms", "nearest_atoms", "DictionaryInspector", "FeatureOverview"]

_ROWS_PER_CALL = 8192        # rows of a [lines, tokens, D] dataset encoded at once (a dense [rows, H] latent per call)


def _pad32(a: torch.Tensor) -> torch.Tensor:
    pad = -a.shape[1] % 32
    return torch.nn.functional.pad(a, (0, pad)) if pad else a


def _integer_atoms(sae) -> torch.Tensor:
    """integer_atoms without the padding."""
    if isinstance(sae, torch.Tensor):
        if sae.dtype != torch.int8 or sae.dim() != 2:
            raise TypeError(f"integer_atoms: a tensor must be int8 [N, D], got {sae.dtype} {tuple(sae.shape)}")
        return sae
    model = _model(sae)
    with torch.no_grad():
        if isinstance(model, BinarySAE):
            if model.n_bits > 8:
                raise TypeError(f"integer_atoms: BinarySAE with n_bits = {model.n_bits} > 8 does not fit int8; "
                                "use compare_decoders (fp32)")
            return model.decoder.quantized_int_weights().to(torch.int8)
        ste = model.decoder if isinstance(model, TernarySparseAutoencoder) else model
        if isinstance(ste, STEWeights):
            w = ste.weight.detach()
            hard = torch.sign(w) * (torch.abs(w) >= ste.threshold)
            return hard.t().to(torch.int8).contiguous()
    raise TypeError(f"integer_atoms: {type(model).__name__} has no integer dictionary; use compare_decoders for the "
                    "fp32 dictionaries")


def integer_atoms(sae) -> torch.Tensor:
    """The dictionary as int8 ``[N, Dp]`` on the model's device, D zero-padded to a multiple of 32 (padding changes
    no dot product and no norm).

      * BinarySAE with ``n_bits <= 8``: ``decoder.quantized_int_weights()``;
      * TernarySparseAutoencoder or ``STEWeights``: ``sign(w) * (|w| >= threshold)`` transposed to ``[H, D]``
        (inspector.py:32-39);
      * an int8 tensor ``[N, D]`` passes through (padded).
    Any other model raises TypeError: its dictionary is fp32, ``compare_decoders`` is the route."""
    return _pad32(_integer_atoms(sae))


def _is_integer(side) -> bool:
    """Whether ``integer_atoms`` accepts this side."""
    if isinstance(side, torch.Tensor):
        return side.dtype == torch.int8
    model = _model(side)
    if isinstance(model, BinarySAE):
        return model.n_bits <= 8
    return isinstance(model.decoder if isinstance(model, TernarySparseAutoencoder) else model, STEWeights)


def _fp32_atoms(side) -> torch.Tensor:
    """The dictionary as fp32 ``[N, D]``, unpadded: ``decoder_atoms`` of a model; an fp32 tensor passes through, an
    int8 tensor is converted."""
    if isinstance(side, torch.Tensor):
        if side.dtype not in (torch.float32, torch.int8) or side.dim() != 2:
            raise TypeError(f"nearest_atoms: a tensor must be fp32 or int8 [N, D], got {side.dtype} {tuple(side.shape)}")
        return side.float() if side.dtype == torch.int8 else side
    return decoder_atoms(side)


def _pad4(a: torch.Tensor) -> torch.Tensor:
    pad = -a.shape[1] % 4
    return torch.nn.functional.pad(a, (0, pad)) if pad else a


def _nearest_atoms_fp32(lhs, rhs, k: int, include_self: bool) -> Dict[str, Any]:
    a = _fp32_atoms(lhs)
    b = None
    if rhs is not None:
        b = _fp32_atoms(rhs)
        if a.device != b.device:
            raise ValueError(f"atoms live on different devices ({a.device} vs {b.device})")
        if a.shape[1] != b.shape[1]:
            raise ValueError(f"atoms have different sizes (D = {a.shape[1]} vs {b.shape[1]})")
        if not include_self:
            raise ValueError("include_self=False is valid in self mode only (rhs=None)")
        b = _pad4(b)                                         # a zero column changes no chain and no norm
    keys = T.nearest_atoms_f32(_pad4(a), b, int(k), exclude_self=not include_self)
    sim, idx = _decode_keys(keys)
    return {"similarity": sim, "index": idx, "distance": torch.clamp(1.0 - sim, min=0.0)}


def nearest_atoms(lhs, rhs=None, k: int = 10, *, include_self: bool = True, atoms: str = "auto") -> Dict[str, Any]:
    """The ``k`` nearest atoms (cosine) of every atom of ``lhs`` among the atoms of ``rhs`` (None: ``lhs`` itself).
    ``lhs`` / ``rhs`` are SAEs or atom tensors ``[N, D]`` (int8 or fp32).

    ``atoms="auto"``: when both sides are integer (int8 tensors, or models ``integer_atoms`` accepts) the int8 path
    below; otherwise, and always with ``atoms="fp32"``, the fp32 path on ``decoder_atoms`` (an int8 tensor is converted,
    D is zero-padded to a multiple of 4): ``c = acc * (inv_a * inv_b)`` with the exact fmaf chain and the inverse norms
    of ``compare_decoders``.  The fp32 result has ``similarity``, ``index`` and ``distance`` and no
    ``duplicate_of`` / ``n_duplicate_groups``: identity of fp32 vectors is not decidable from rounded dot products.

    Result (tensors on the device):
      similarity  fp32 [Na, k]   c = fp32(dot) * (inv_a * inv_b), largest first; an all-zero atom has cosine 0 with
                                 everything, itself included (the reference's safe_norms)
      index       int64 [Na, k]  equal cosine bits go to the lowest index; past the candidates: -inf / -1
      distance    fp32 [Na, k]   clamp(1 - similarity, min=0) (inspector.py:57-58)
    self mode only:
      duplicate_of        int32 [Na]  the lowest index holding an identical atom (the atom's own where none is lower)
      n_duplicate_groups  int         distinct atoms that occur more than once (what ``count_duplicates`` returns)
    ``include_self=True`` keeps j == i in self mode, as sklearn on a precomputed matrix does (the reference's callers
    drop column 0 themselves); ``include_self=False`` is valid in self mode only.  A different D or device raises
    ValueError."""
    if atoms not in ("auto", "fp32"):
        raise ValueError(f"atoms must be 'auto' or 'fp32', got {atoms!r}")
    if atoms == "fp32" or not (_is_integer(lhs) and (rhs is None or _is_integer(rhs))):
        return _nearest_atoms_fp32(lhs, rhs, k, include_self)
    a = integer_atoms(lhs)
    b = None
    if rhs is not None:
        b = integer_atoms(rhs)
        if a.device != b.device:
            raise ValueError(f"atoms live on different devices ({a.device} vs {b.device})")
        if a.shape[1] != b.shape[1]:
            raise ValueError(f"atoms have different sizes (D = {a.shape[1]} vs {b.shape[1]})")
        if not include_self:
            raise ValueError("include_self=False is valid in self mode only (rhs=None)")
    keys, dup = T.nearest_atoms_i8(a, b, int(k), exclude_self=not include_self, want_duplicates=b is None)
    sim, idx = _decode_keys(keys)
    out: Dict[str, Any] = {"similarity": sim, "index": idx, "distance": torch.clamp(1.0 - sim, min=0.0)}
    if b is None:
        out["duplicate_of"] = dup
        out["n_duplicate_groups"] = int(torch.unique(dup[dup != torch.arange(dup.numel(), device=dup.device)]).numel())
    return out


class FeatureOverview:
    """What ``print_feature_activations_overview`` returns: for every feature how often it was the most activated one
    (``counts`` int64 [F]) and where, as CSR -- ``positions[offsets[f] : offsets[f + 1]]`` are the flat positions
    ``line * tokens_per_line + pos`` of feature f in ascending order, the order the reference's loop appends them in."""

    def __init__(self, counts: torch.Tensor, offsets: torch.Tensor, positions: torch.Tensor, tokens_per_line: int):
        self.counts, self.offsets, self.positions = counts, offsets, positions
        self.tokens_per_line = int(tokens_per_line)

    def to_python(self) -> Dict[int, Dict[str, Any]]:
        """The reference's ``feature_dict``: ``{id: {"cnt": n, "pos": [(line, pos), ...]}}`` for the features that won at
        least once.  Two host copies."""
        bounds, flat, t = self.offsets.cpu().tolist(), self.positions.cpu().tolist(), self.tokens_per_line
        return {f: {"cnt": bounds[f + 1] - bounds[f], "pos": [(g // t, g % t) for g in flat[bounds[f]:bounds[f + 1]]]}
                for f in range(len(bounds) - 1) if bounds[f + 1] > bounds[f]}


def _activation_table(feature_activations) -> torch.Tensor:
    """[lines, tokens] integer tensor from the reference's list of per-line lists (or a tensor, returned as it is)."""
    fa = feature_activations if isinstance(feature_activations, torch.Tensor) else torch.as_tensor(feature_activations)
    if fa.dim() != 2 or fa.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool):
        raise ValueError(f"feature_activations: expected integer feature ids [lines, tokens], got {fa.dtype} {tuple(fa.shape)}")
    return fa


def _match_mask(match_mask, fa: torch.Tensor) -> torch.Tensor:
    m = match_mask if isinstance(match_mask, torch.Tensor) else torch.as_tensor(match_mask)
    if m.dtype != torch.bool or m.shape != fa.shape:
        raise ValueError(f"match_mask: expected bool {tuple(fa.shape)}, got {m.dtype} {tuple(m.shape)}")
    return m.to(fa.device)


class DictionaryInspector:
    """``TernarySparseAutoencoderInspector`` (utils/inspector.py) for any dictionary, with the reference's method names
    and meanings.  ``sae`` is an SAE (wrapper or module) or atoms ``[N, D]``: an integer dictionary (or int8 atoms) is
    held as int8, any other as fp32 (``decoder_atoms``).  The methods that read activations (``linguistic_analyze``,
    ``top_examples``) need the model, not only its atoms."""

    def __init__(self, sae):
        # int8 or fp32 [N, D], unpadded (the kernel call pads)
        self.atoms = _integer_atoms(sae) if _is_integer(sae) else _fp32_atoms(sae)
        self.dictionary_in_ternary = self.atoms             # the reference's attribute name
        self.model = None if isinstance(sae, torch.Tensor) else _model(sae)

    # ---- activations (inspector.py:173-208, 266-292) ------------------------------------------------------------------
    def _encoder(self) -> HipEncoder:
        enc = getattr(self.model, "encoder", None)
        if not isinstance(enc, HipEncoder) or enc._act != T.ACT_RELU:
            raise TypeError("this method reads activations: the inspector must be built from a model with a linear + ReLU "
                            "encoder (TernarySparseAutoencoder), not from atoms")
        return enc

    def _batches(self, dataset) -> Iterator[Tuple[torch.Tensor, int]]:
        """(rows fp32 [r, D] on the model's device, lines they complete) of a dataset: a tensor [lines, tokens, D] in
        chunks of whole lines, or an iterable of contexts [tokens, D] one by one, as the reference walks it."""
        dev = self._encoder().linear.weight.device
        if isinstance(dataset, torch.Tensor) and dataset.dim() == 3:
            lines, tokens, D = dataset.shape
            step = max(1, _ROWS_PER_CALL // max(tokens, 1))
            for l0 in range(0, lines, step):
                part = dataset[l0:l0 + step]
                yield part.reshape(-1, D).to(dev, torch.float32).contiguous(), part.shape[0]
            return
        for context in dataset:
            yield torch.as_tensor(context).to(dev, torch.float32).contiguous(), 1

    def linguistic_analyze(self, dataset) -> torch.Tensor:
        """The most activated feature of every token: int64 [lines, tokens] on the device (``.tolist()`` is the
        reference's list of lists).  One ``encode_topk`` with k = 1 per batch on the exact encoder, no dense latent: the
        largest pre-activation, equal values to the lowest index (``torch.max``'s documented choice); where it is not
        above 0 the ReLU row is all zero and the result is index 0, as ``argmax`` of such a row is."""
        lin = self._encoder().linear
        out: List[torch.Tensor] = []
        with torch.no_grad():
            for x, n_lines in self._batches(dataset):
                idx, val = T.encode_topk(x, lin.weight.detach(), None if lin.bias is None else lin.bias.detach(), 1)
                win = torch.where(val[:, 0] > 0, idx[:, 0], torch.zeros_like(idx[:, 0])).long()
                out.append(win.reshape(n_lines, -1))
        if not out:
            return torch.zeros((0, 0), dtype=torch.int64, device=lin.weight.device)
        return torch.cat(out, dim=0)

    def top_examples(self, dataset, n: int, floor: float = 0.0) -> Dict[str, torch.Tensor]:
        """The ``n`` strongest activations of every feature over ``dataset`` (``TopExamples.finish()``: values, positions,
        counts), from the model's dense ReLU latent; position = ``line * tokens + pos``."""
        enc = self._encoder()
        state = TopExamples(enc.linear.weight.shape[0], n, enc.linear.weight.device, floor)
        base = 0
        with torch.no_grad():
            for x, _ in self._batches(dataset):
                state.add_dense(enc(x), base)
                base += x.shape[0]
        return state.finish()

    def print_feature_activations_overview(self, feature_activations) -> FeatureOverview:
        """How often and where each feature was the most activated one, from ``linguistic_analyze``'s table (tensor or
        list of lists): a ``FeatureOverview`` on the device, built by ``TokenLists`` with positions in place of tokens;
        ``.to_python()`` is the reference's dict.  Ids outside [0, number of atoms) are dropped."""
        fa = _activation_table(feature_activations)
        lines, tokens = fa.shape
        if lines * tokens >= 2 ** 31:
            raise ValueError("print_feature_activations_overview: positions are stored as int32")
        dev = self.atoms.device
        F = self.atoms.shape[0]
        ids = fa.reshape(-1, 1).to(dev)
        ids = torch.where((ids >= 0) & (ids < F), ids, torch.full_like(ids, -1)).to(torch.int32)
        lists = TokenLists(F, dev)
        lists.add_compact(ids, None, torch.arange(lines * tokens, dtype=torch.int32, device=dev))
        offsets, positions = lists.finish()
        return FeatureOverview(offsets[1:] - offsets[:-1], offsets, positions, tokens)

    @staticmethod
    def check_sensitivity(feature_activations, match_mask, feature_id: int) -> float:
        """Of the tokens that match the targets (``match_mask`` bool [lines, tokens]: the caller's
        ``any(t in token for t in target_tokens)``), the share whose most activated feature is ``feature_id``
        (inspector.py:266-280).  No matching token: ZeroDivisionError, as there."""
        fa = _activation_table(feature_activations)
        m = _match_mask(match_mask, fa)
        return int((m & (fa == int(feature_id))).sum()) / int(m.sum())

    @staticmethod
    def check_specificity(overview: FeatureOverview, match_mask, feature_id: int) -> float:
        """Of the positions where ``feature_id`` was the most activated feature, the share that matches the targets
        (inspector.py:282-292).  A feature that never won: KeyError, as the reference's dict lookup."""
        f = int(feature_id)
        beg, end = int(overview.offsets[f]), int(overview.offsets[f + 1])
        if end == beg:
            raise KeyError(f)
        m = match_mask if isinstance(match_mask, torch.Tensor) else torch.as_tensor(match_mask)
        if m.dtype != torch.bool or m.dim() != 2 or m.shape[1] != overview.tokens_per_line:
            raise ValueError(f"match_mask: expected bool [lines, {overview.tokens_per_line}], got {m.dtype} {tuple(m.shape)}")
        pos = overview.positions[beg:end].long()
        return int(m.reshape(-1).to(pos.device)[pos].sum()) / (end - beg)

    def get_feature(self, feature_idx):
        return self.atoms[feature_idx]

    def calculate_k_nearest_features_cluster(self, k, type="cosine"):
        """-> ``(distances [N, k], indices [N, k])``: each atom's k nearest atoms, itself included (column 0 unless a
        duplicate with a lower index precedes it).  Unlike the reference, ``distances`` holds the k columns that belong
        to ``indices`` and not the [N, N] matrix, and equal distances are ordered by index.  ``type="cosine"``:
        ``clamp(1 - c, 0)``; ``type="euclidean"``: the distance of the normalised atoms, ``sqrt(clamp(2 - 2c, 0))`` --
        with an all-zero atom the reference's ``cdist`` ordering is no longer a function of the cosine: ValueError."""
        if type not in ("cosine", "euclidean"):
            raise ValueError(f"type must be 'cosine' or 'euclidean', got {type!r}")
        if type == "euclidean" and self.zero_entries() > 0:
            raise ValueError("euclidean neighbours are not defined by the cosine when the dictionary has an all-zero atom")
        res = nearest_atoms(self.atoms, None, k)
        if type == "cosine":
            return res["distance"], res["index"]
        return torch.sqrt(torch.clamp(2.0 - 2.0 * res["similarity"], min=0.0)), res["index"]

    def _unit(self, f) -> torch.Tensor:
        v = self.atoms[f].to(torch.float32)
        n = torch.linalg.norm(v)
        return v / torch.where(n == 0, torch.ones_like(n), n)

    def distance(self, f1, f2, type="cosine"):
        u, v = self._unit(f1), self._unit(f2)
        if type == "cosine":
            return 1 - u @ v
        if type == "euclidean":
            return torch.sqrt(torch.sum((u - v) ** 2))
        raise ValueError(f"type must be 'cosine' or 'euclidean', got {type!r}")

    def analyze_ternary_distribution(self) -> Dict[int, int]:
        """{value: count} for whatever integer values occur (the reference prints the counts of -1, 0 and +1)."""
        if self.atoms.dtype != torch.int8:
            raise TypeError("analyze_ternary_distribution: the dictionary is fp32, not integer")
        vals, counts = torch.unique(self.atoms, return_counts=True)
        return {int(v): int(c) for v, c in zip(vals.tolist(), counts.tolist())}

    def zero_entries(self) -> int:
        return int((self.atoms == 0).all(dim=1).sum().item())

    def count_duplicates(self) -> int:
        if self.atoms.dtype != torch.int8:
            _, counts = torch.unique(self.atoms, dim=0, return_counts=True)
            return int((counts > 1).sum().item())
        return nearest_atoms(self.atoms, None, 1)["n_duplicate_groups"]

    def check_same_entries(self, indices: Sequence[int]):
        if len(indices) < 2:
            return []
        matching = self.atoms[indices[0]] == self.atoms[indices[1]]
        for i in indices[2:]:
            matching = (self.atoms[i] == self.atoms[indices[0]]) & matching
        return int(matching.sum().item()), torch.nonzero(matching, as_tuple=True)

    def sparsity_rate(self) -> float:
        return float((self.atoms == 0).sum().item()) / self.atoms.numel()

    def k_means_analysis(self, num_clusters, type="cosine", **kmeans_kwargs):
        """-> ``(cluster_ids_x [N], cluster_centers [C, D], cluster_ids_by_group, center_features)`` as
        inspector.py:137-165, with ``kmeans_atoms`` (inference/clustering.py) in place of ``kmeans_pytorch`` on the CPU;
        ``kmeans_kwargs`` go to it (seed, tol, max_iter, init_indices, ...).  ``cluster_ids_by_group[c]`` is the
        ascending list of members of cluster c; ``center_features[c]`` is the member with the smallest
        ``1 - atom . center`` on the raw vectors (cosine, inspector.py:155) or ``|atom - center|`` (euclidean, the intent
        of :157; ranked by ``|atom|^2 / 2 - atom . center``, the same order), evaluated in fp64, the lowest index among
        equals, -1 for an empty cluster."""
        from .clustering import kmeans_atoms
        if type not in ("cosine", "euclidean"):
            raise ValueError(f"type must be 'cosine' or 'euclidean', got {type!r}")
        res = kmeans_atoms(self.atoms, num_clusters, distance=type, **kmeans_kwargs)
        labels, centers = res["labels"], res["centers"]
        groups, center_features = _groups_and_center_features(_fp32_atoms(self.atoms), labels, centers, type)
        return labels, centers, groups, center_features


def _groups_and_center_features(atoms: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, type: str):
    """What inspector.py:143-163 computes around its kmeans call, by segment reductions on the device: the members of
    every cluster in ascending order, and per cluster the member nearest to the center (see ``k_means_analysis``)."""
    N, C = atoms.shape[0], centers.shape[0]
    ok = labels >= 0
    lab = labels.clamp(min=0)
    a64, own = atoms.double(), centers[lab].double()
    dot = (a64 * own).sum(1)
    if type == "cosine":
        rank = dist = 1.0 - dot
    else:
        # ranked by |a|^2 / 2 - a . c, which orders the members as |a - c| does and, unlike the sum of squared
        # differences, is exact in fp64 for an integer dictionary: members at the same distance compare equal
        rank = 0.5 * (a64 * a64).sum(1) - dot
        dist = torch.sqrt(torch.clamp(2.0 * rank + (own * own).sum(1), min=0.0))
    # the reference starts its search at min_distance = 99999: a member at or beyond that (or NaN) is never chosen
    valid = ok & (dist < 99999.0)
    rank = torch.where(valid, rank, torch.full_like(rank, float("inf")))
    best = torch.full((C,), float("inf"), dtype=torch.float64, device=atoms.device)
    best = best.scatter_reduce(0, lab, rank, "amin")
    index = torch.arange(N, device=atoms.device)
    cand = torch.where(valid & (rank == best[lab]), index, torch.full_like(index, N))
    first = torch.full((C,), N, dtype=torch.int64, device=atoms.device).scatter_reduce(0, lab, cand, "amin")
    center_features = [int(i) if i < N else -1 for i in first.tolist()]
    order = torch.argsort(torch.where(ok, labels, torch.full_like(labels, C)), stable=True)
    sizes = torch.bincount(labels[ok], minlength=C).tolist()
    members = order.tolist()
    groups, at = [], 0
    for n in sizes:
        groups.append(members[at:at + n])
        at += n
    return groups, center_features
