"""Consumers of the sparse latent: activation masks, L0 per level, activation / co-activation counts.

Mirror of the reference's analysis helpers (scripts/analysis/dynamic_analysis.py): same function names,
arguments and result keys, so an analysis script switches over by changing the import.  The reference reduces
the dense [B, H] latent to a boolean mask and forms ``mask.sum(0)`` and ``mask.T @ mask`` (a dense [H,B]x[B,H]
product per batch); here the top-k variants work from the compact ``(idx, val)`` output of
``forward_compact`` -- k and k^2 integer increments per row (``qsae_activation_counts``,
``qsae_coactivation_sparse``) -- and the threshold variants from the bit-packed encoder output: per-unit popcounts
(``qsae_activation_counts_bits``) and the int8-MFMA rank-B update of ``qsae_coactivation_bits``.  The tokens per feature
come in two forms: ``with_tokens="csr"`` builds them on the device as ordered CSR lists (``TokenLists``,
``qsae_token_lists_*``) from the same ``(idx, val)`` or packed bits, with no [B, H] mask in memory for any model;
``with_tokens=True`` returns the reference's list of Python lists and, for the threshold models, goes through the mask.
"""
from __future__ import annotations

import weakref
from typing import Any, Dict, Iterable, List, Optional, Union

import torch

from .. import torch_ops as ops          # torch.ops.qsae.* (dispatcher ops over the C ABI)
from ..sae import (BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, ResidualQuantizedSAE)
from .framework import SAEWrapper, _ensure_tensor, compute_reconstruction_error  # noqa: F401  (re-export)
from .coactivation_partners import CoactivationPartners
from .token_lists import TokenLists, check_token_ids
from .top_examples import TopExamples


def _hidden_dim(sae: SAEWrapper) -> int:
    """Total number of hidden units (dynamic_analysis.py:17-27)."""
    model = sae.model
    if isinstance(model, (BinarySAE, QuantizedMatryoshkaSAE)):
        return int(model.hidden_dim)
    if isinstance(model, BaselineSparseAutoencoder):
        return int(model.encoder.linear.weight.shape[0])
    if isinstance(model, ResidualQuantizedSAE):
        return int(sum(s.hidden_dim for s in model.saes))
    raise ValueError(f"Unable to determine hidden_dim for model type {type(model)}")


def _bits_to_mask(zbits: torch.Tensor, index: Optional[torch.Tensor], H: int) -> torch.Tensor:
    """int32 [B, words] packed bits (bit j of word w = packed unit 32 w + j) -> bool [B, H] in the model's own
    hidden order (``index[p]`` = original unit of packed position p, -1 for padding)."""
    B, words = zbits.shape
    shifts = torch.arange(32, device=zbits.device, dtype=torch.int32)
    bits = ((zbits.unsqueeze(-1) >> shifts) & 1).to(torch.bool).reshape(B, words * 32)
    if index is None:
        return bits[:, :H]
    mask = torch.zeros((B, H), dtype=torch.bool, device=zbits.device)
    valid = index >= 0
    mask[:, index[valid]] = bits[:, valid]
    return mask


def _stage_bits(model: QuantizedMatryoshkaSAE, x: torch.Tensor):
    """(packed bits, packed-position -> original-unit index or None) of one matryoshka encoder."""
    zb = model.activation_bits(x)
    index = model.decoder.padded_index(zb.device) if model.decoder.needs_padding else None
    return zb, index


def _residual_stages(model: ResidualQuantizedSAE, x: torch.Tensor):
    """Yields (stage, packed bits, index) with the residual updated as in the forward pass
    (sae/residual_quantized.py:53-69; dynamic_analysis.py:56-70)."""
    residual = x if x.dtype == torch.float32 else x.float()
    for sub in model.saes:
        zb, index = _stage_bits(sub, residual)
        _, levels = sub.decoder.decode_bits(zb)
        yield sub, zb, index
        residual = (residual - levels[-1]) * 2


def _packed_bits(model, x: torch.Tensor):
    """(packed bits int32 [B, words], index int32 [32 * words] or None) of a threshold model in the order of
    ``_hidden_dim``: the matryoshka encoder's own words, the residual model's stages side by side with each stage's
    unit offset added to its map -- one bit matrix, so one counts call and one co-activation call cover the cross-stage
    blocks too."""
    if isinstance(model, QuantizedMatryoshkaSAE):
        stages = [(model, *_stage_bits(model, x))]
    elif isinstance(model, ResidualQuantizedSAE):
        stages = list(_residual_stages(model, x))
    else:
        raise TypeError(f"Unsupported SAE model type: {type(model)}")
    zbits = stages[0][1] if len(stages) == 1 else torch.cat([zb for _, zb, _ in stages], dim=1)
    # the map depends on the model's structure alone: built and converted to int32 once per model, device and widths
    key = (zbits.device, tuple(zb.shape[1] for _, zb, _ in stages))
    cache = _packed_index_cache.setdefault(model, {})
    if key not in cache:
        cache[key] = _packed_index(stages)
    return zbits, cache[key]


_packed_index_cache: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _packed_index(stages) -> Optional[torch.Tensor]:
    """int32 packed position -> unit of (sub-model, packed bits, stage index) side by side, None for the identity"""
    if len(stages) == 1 and stages[0][2] is None and stages[0][1].shape[1] * 32 == stages[0][0].hidden_dim:
        return None
    maps, offset = [], 0
    for sub, zb, index in stages:
        nbits = zb.shape[1] * 32
        if index is None:                                   # identity; positions past hidden_dim are pad slots
            index = torch.arange(nbits, device=zb.device)
            index = torch.where(index < sub.hidden_dim, index, torch.full_like(index, -1))
        maps.append(torch.where(index >= 0, index + offset, index))
        offset += int(sub.hidden_dim)
    return torch.cat(maps).to(torch.int32)


def _threshold_stats(model, x: torch.Tensor, H: int, counts: torch.Tensor, coact: Optional[torch.Tensor], with_tokens: bool,
                     lists: Optional[TokenLists] = None, batch_tok: Optional[torch.Tensor] = None,
                     partners: Optional[CoactivationPartners] = None) -> Optional[torch.Tensor]:
    """counts / coact += this batch's activation statistics of a threshold model, from the packed bits; ``lists`` takes
    the batch's tokens per feature and ``partners`` its co-activation bits from the same bits (``coact`` None: no
    counts matrix).  Returns the bool mask [B, H] (on the device) when the tokens per feature are wanted as Python
    lists, else None: nothing else needs it."""
    zb, index = _packed_bits(model, x)
    counts += _packed_counts_to_units(ops.activation_counts_bits(zb), index, H)
    if coact is not None:
        ops.coactivation_bits(zb, H, index, coact)
    if partners is not None:
        partners.add_bits(zb, index)
    if lists is not None:
        lists.add_bits(zb, index, batch_tok)
    return _bits_to_mask(zb, index, H) if with_tokens else None


def _token_lists_mode(with_tokens, token_ids: torch.Tensor) -> bool:
    """True for ``with_tokens="csr"``, False for a bool; any other value raises.  The CSR form stores token ids as int32,
    so ``token_ids`` is checked here, once."""
    if isinstance(with_tokens, bool):
        return False
    if not (isinstance(with_tokens, str) and with_tokens == "csr"):
        raise ValueError(f'with_tokens: expected True, False or "csr", got {with_tokens!r}')
    check_token_ids(token_ids)
    return True


def _coactivation_mode(coactivation, H: int, dev):
    """(int32 [H, H] counts or None, CoactivationPartners or None) for ``coactivation="counts" | "partners" | None``"""
    if coactivation is None:
        return None, None
    if coactivation == "counts":
        return torch.zeros((H, H), dtype=torch.int32, device=dev), None
    if coactivation == "partners":
        return None, CoactivationPartners(H, dev)
    raise ValueError(f'coactivation: expected "counts", "partners" or None, got {coactivation!r}')


def _coactivation_result(coact: Optional[torch.Tensor], partners: Optional[CoactivationPartners]) -> Dict[str, Any]:
    out: Dict[str, Any] = {"coactivation": None if coact is None else coact.cpu()}
    if partners is not None:
        out["coactivation_partner_counts"] = partners.counts().cpu()
        out["coactivation_partners"] = partners
    return out


def _top_examples_mode(top_examples: Optional[int], model, H: int, dev) -> Optional[TopExamples]:
    """A ``TopExamples`` state for ``top_examples=n``, None for None.  Only the top-k models feed it here (from their
    compact output); the threshold models keep one bit per unit, so there is nothing to rank by, and a model with a dense
    latent goes through ``DictionaryInspector.top_examples``: TypeError for both."""
    if top_examples is None:
        return None
    if isinstance(model, (QuantizedMatryoshkaSAE, ResidualQuantizedSAE)):
        raise TypeError(f"top_examples: {type(model).__name__} is a threshold model -- its activations are one bit per unit "
                        "and have no magnitude to rank by; only BinarySAE and BaselineSparseAutoencoder are supported")
    if not isinstance(model, (BinarySAE, BaselineSparseAutoencoder)):
        raise TypeError(f"top_examples: {type(model).__name__} has no compact top-k output; for a model with a dense latent "
                        "use DictionaryInspector(model).top_examples(dataset, n)")
    return TopExamples(H, int(top_examples), dev)


def _top_examples_result(examples: Optional[TopExamples]) -> Dict[str, Any]:
    return {} if examples is None else {"top_examples": examples.finish()}


def activation_indices(sae: SAEWrapper, x: torch.Tensor):
    """Compact activation set of the top-k variants: (idx int32 [B,k], val fp32 [B,k]); an entry is active
    when val > 0 (the reference's ``latent > 0``)."""
    model = sae.model
    if not isinstance(model, (BinarySAE, BaselineSparseAutoencoder)):
        raise TypeError(f"{type(model).__name__} has no compact top-k output; use _activation_mask")
    idx, val, _recon = model.forward_compact(x)
    return idx, val


def _activation_mask(sae: SAEWrapper, x: torch.Tensor) -> torch.Tensor:
    """Boolean mask [batch, hidden_dim] of the active features, on the CPU like the reference's
    (dynamic_analysis.py:30-73): BinarySAE / baseline ``latent > 0``, matryoshka ``sigmoid(encoder) > 0.5``,
    residual: the stages' masks concatenated."""
    model = sae.model
    H = _hidden_dim(sae)
    with torch.no_grad():
        x = _ensure_tensor(x).to(sae.device)
        if isinstance(model, (BinarySAE, BaselineSparseAutoencoder)):
            idx, val = activation_indices(sae, x)
            mask = torch.zeros((x.shape[0], H), dtype=torch.bool, device=x.device)
            mask.scatter_(1, idx.long(), val > 0)
        elif isinstance(model, QuantizedMatryoshkaSAE):
            zb, index = _stage_bits(model, x)
            mask = _bits_to_mask(zb, index, H)
        elif isinstance(model, ResidualQuantizedSAE):
            parts = [_bits_to_mask(zb, index, sub.hidden_dim) for sub, zb, index in _residual_stages(model, x)]
            mask = torch.cat(parts, dim=1)
        else:
            raise TypeError(f"Unsupported SAE model type: {type(model)}")
    return mask.cpu()


def _packed_counts_to_units(counts_packed: torch.Tensor, index: Optional[torch.Tensor], H: int) -> torch.Tensor:
    if index is None:
        return counts_packed[:H]
    out = torch.zeros((H,), dtype=torch.int64, device=counts_packed.device)
    valid = index >= 0
    out[index[valid]] = counts_packed[valid]
    return out


def compute_l0_by_level(sae: SAEWrapper, loader: Iterable[Any], device: Optional[Any] = None) -> torch.Tensor:
    """Average number of active units per token for each level (dynamic_analysis.py:168-251): matryoshka
    levels = nested dictionary slices, residual levels = stages, other SAEs a length-1 tensor."""
    if device is not None:
        sae.to(device)
    sae.eval()
    model = sae.model
    n_tokens = 0
    with torch.no_grad():
        if isinstance(model, QuantizedMatryoshkaSAE):
            sizes = list(model.decoder.nested_dictionary_size)
            H = int(model.hidden_dim)
            per_unit = torch.zeros((H,), dtype=torch.int64, device=sae.device)
            for batch in loader:
                x = _ensure_tensor(batch).to(sae.device)
                zb, index = _stage_bits(model, x)
                per_unit += _packed_counts_to_units(ops.activation_counts_bits(zb), index, H)
                n_tokens += x.shape[0]
            bounds = torch.tensor([0] + sizes).cumsum(0).tolist()
            total = torch.stack([per_unit[bounds[i]:bounds[i + 1]].sum() for i in range(len(sizes))])
            return total.to(torch.float64).cpu() / max(float(n_tokens), 1.0)
        if isinstance(model, ResidualQuantizedSAE):
            total = torch.zeros((len(model.saes),), dtype=torch.float64)
            for batch in loader:
                x = _ensure_tensor(batch).to(sae.device)
                for i, (sub, zb, index) in enumerate(_residual_stages(model, x)):
                    total[i] += float(ops.activation_counts_bits(zb).sum().item())   # padding bits are never set
                n_tokens += x.shape[0]
            return total / max(float(n_tokens), 1.0)
        total_act = 0.0
        for batch in loader:
            x = _ensure_tensor(batch).to(sae.device)
            _idx, val = activation_indices(sae, x)
            total_act += float((val > 0).sum().item())
            n_tokens += x.shape[0]
        return torch.tensor([total_act / max(float(n_tokens), 1.0)], dtype=torch.float64)


def _tokens_per_feature(feat: torch.Tensor, tok: torch.Tensor, H: int, into: List[List[int]]) -> None:
    """Append token ids per feature; within a feature in ascending row order, like the reference's loop over
    ``mask.nonzero()`` (row-major)."""
    if feat.numel() == 0:
        return
    order = torch.sort(feat, stable=True).indices
    feat_s, tok_s = feat[order].cpu(), tok[order].cpu()
    uniq, counts = torch.unique_consecutive(feat_s, return_counts=True)
    start = 0
    toks = tok_s.tolist()
    for f, c in zip(uniq.tolist(), counts.tolist()):
        into[f].extend(toks[start:start + c])
        start += c


def compute_activation_stats(sae: SAEWrapper, loader: Iterable[Any], *, token_ids: torch.Tensor,
                             tokens_per_context: int, device: Optional[Any] = None,
                             with_tokens: Union[bool, str] = True,
                             coactivation: Optional[str] = "counts",
                             top_examples: Optional[int] = None) -> Dict[str, Any]:
    """activation_counts [H] (int64), coactivation [H,H] (int32, mask^T mask) and tokens_per_feature
    (dynamic_analysis.py:255-311).  Counts are accumulated on the device and copied to the host once.
    ``with_tokens="csr"``: tokens_per_feature is the tuple (offsets int64 [H + 1], tokens int32 [nnz]) on the SAE's device,
    in the reference's order, as ``top_token_sets`` / ``jaccard_histogram`` take it.
    ``coactivation="partners"``: the [H, H] matrix is never allocated; ``coactivation`` is None and the result has
    ``coactivation_partner_counts`` (int64 [H] on the host: the number of other features each feature ever fired
    with, what ``summary.average_coactivating_features`` needs) and ``coactivation_partners`` (the
    ``CoactivationPartners`` state on the device).  ``coactivation=None`` skips co-activation altogether.
    ``top_examples=n`` (top-k models only, TypeError otherwise): the result gains ``top_examples``, the ``n`` strongest
    activations of every feature from the same ``(idx, val)`` (``TopExamples.finish()``: values, positions, counts on the
    device; positions are the global row index that ``token_ids`` is indexed by)."""
    csr = _token_lists_mode(with_tokens, token_ids)
    if device is not None:
        sae.to(device)
    sae.eval()
    model = sae.model
    H = _hidden_dim(sae)
    dev = sae.device
    counts = torch.zeros((H,), dtype=torch.int64, device=dev)
    coact, partners = _coactivation_mode(coactivation, H, dev)
    lists = TokenLists(H, dev) if csr else None
    examples = _top_examples_mode(top_examples, model, H, dev)
    tokens_per_feature: List[List[int]] = [] if csr else [[] for _ in range(H)]
    with_lists = with_tokens is True
    global_index = 0
    compact = isinstance(model, (BinarySAE, BaselineSparseAutoencoder))
    with torch.no_grad():
        for batch in loader:
            x = _ensure_tensor(batch).to(dev)
            B = x.shape[0]
            flat = torch.arange(global_index, global_index + B, dtype=torch.long)
            batch_tok = token_ids[torch.div(flat, tokens_per_context, rounding_mode="floor"), flat % tokens_per_context]
            if compact:
                idx, val = activation_indices(sae, x)
                ops.activation_counts(idx, val, H, counts)
                if coact is not None:
                    ops.coactivation_sparse(idx, val, H, coact)
                if partners is not None:
                    partners.add_compact(idx, val)
                if examples is not None:
                    examples.add_compact(idx, val, global_index)
                if csr:
                    lists.add_compact(idx, val, batch_tok)
                elif with_lists:
                    on = val > 0
                    rows = torch.arange(B, device=dev).unsqueeze(1).expand_as(idx)[on]
                    _tokens_per_feature(idx[on].long(), batch_tok.to(dev)[rows], H, tokens_per_feature)
            else:
                # threshold variants: hundreds to thousands of active units per row, so mask^T mask is a dense rank-B
                # update (dynamic_analysis.py:405-415) -- of single bits: formed from the packed encoder output on the
                # int8 matrix pipe (qsae_coactivation_bits), exact in int32, without a [B, H] mask in memory
                mask = _threshold_stats(model, x, H, counts, coact, with_lists, lists, batch_tok, partners)
                if with_lists:
                    nz = mask.nonzero(as_tuple=False)
                    _tokens_per_feature(nz[:, 1], batch_tok.to(dev)[nz[:, 0]], H, tokens_per_feature)
            global_index += B
    return {"activation_counts": counts.cpu(), **_coactivation_result(coact, partners),
            "tokens_per_feature": lists.finish() if csr else tokens_per_feature, **_top_examples_result(examples)}


def compute_reconstruction_error_by_level(sae: SAEWrapper, loader: Iterable[Any], device: Optional[Any] = None) -> torch.Tensor:
    """Per-level reconstruction MSE (dynamic_analysis.py:103-165): matryoshka = every cumulative level against the
    input; residual = every stage's reconstruction against the residual it was given (the training objective);
    other SAEs a length-1 tensor with the overall MSE.  Squared errors are summed on the device in fp64
    (qsae_sq_err_sum) and read once at the end."""
    if device is not None:
        sae.to(device)
    sae.eval()
    model = sae.model
    if not isinstance(model, (QuantizedMatryoshkaSAE, ResidualQuantizedSAE)):
        return torch.tensor([compute_reconstruction_error(sae, loader)], dtype=torch.float64)
    sums: Optional[List[torch.Tensor]] = None
    n_elements = 0
    with torch.no_grad():
        for batch in loader:
            x = _ensure_tensor(batch).to(sae.device)
            x = x if x.dtype == torch.float32 else x.float()
            _groups, levels = model(x)
            if sums is None:
                sums = [torch.zeros((), dtype=torch.float64, device=sae.device) for _ in levels]
            target = x.contiguous()
            for i, recon in enumerate(levels):
                ops.sq_err_sum(recon, target, sums[i])
                if isinstance(model, ResidualQuantizedSAE):
                    target = ((target - recon) * 2).contiguous()
            n_elements += x.numel()
    if sums is None:
        raise ValueError("empty loader")
    return torch.stack(sums).cpu() / float(max(n_elements, 1))


def analyze_dataset(sae: SAEWrapper, loader: Iterable[Any], *, token_ids: torch.Tensor, tokens_per_context: int,
                    device: Optional[Any] = None, with_tokens: Union[bool, str] = True,
                    coactivation: Optional[str] = "counts", top_examples: Optional[int] = None) -> Dict[str, Any]:
    """One pass over the data: final reconstruction MSE, activation counts, co-activation matrix and tokens per
    feature (dynamic_analysis.py:317-440; same result keys, ``mse_per_level`` / ``l0_per_level`` are None there
    too).  Top-k variants run ``forward_compact`` once per batch and feed its (idx, val, reconstruction) to the
    integer kernels and the fp64 squared-error sum; the threshold variants take the reconstruction from the
    forward pass and the masks from the bit-packed encoder output.  ``with_tokens="csr"``: tokens_per_feature is the
    CSR tuple on the SAE's device (see ``compute_activation_stats``), built without a mask or a Python list.
    ``coactivation``: "counts" (the int32 matrix), "partners" (one bit per pair on the device and the partner counts) or
    None, as in ``compute_activation_stats``.  ``top_examples=n``: the ``n`` strongest activations per feature, as in
    ``compute_activation_stats`` (top-k models only)."""
    csr = _token_lists_mode(with_tokens, token_ids)
    if device is not None:
        sae.to(device)
    sae.eval()
    model = sae.model
    H = _hidden_dim(sae)
    dev = sae.device
    counts = torch.zeros((H,), dtype=torch.int64, device=dev)
    coact, partners = _coactivation_mode(coactivation, H, dev)
    sq = torch.zeros((), dtype=torch.float64, device=dev)
    lists = TokenLists(H, dev) if csr else None
    examples = _top_examples_mode(top_examples, model, H, dev)
    tokens_per_feature: List[List[int]] = [] if csr else [[] for _ in range(H)]
    with_lists = with_tokens is True
    global_index, n_elements = 0, 0
    compact = isinstance(model, (BinarySAE, BaselineSparseAutoencoder))
    with torch.no_grad():
        for batch in loader:
            x = _ensure_tensor(batch).to(dev)
            x = (x if x.dtype == torch.float32 else x.float()).contiguous()
            B = x.shape[0]
            flat = torch.arange(global_index, global_index + B, dtype=torch.long)
            batch_tok = token_ids[torch.div(flat, tokens_per_context, rounding_mode="floor"), flat % tokens_per_context]
            if compact:
                idx, val, recon = model.forward_compact(x)
                ops.sq_err_sum(recon, x, sq)
                ops.activation_counts(idx, val, H, counts)
                if coact is not None:
                    ops.coactivation_sparse(idx, val, H, coact)
                if partners is not None:
                    partners.add_compact(idx, val)
                if examples is not None:
                    examples.add_compact(idx, val, global_index)
                if csr:
                    lists.add_compact(idx, val, batch_tok)
                elif with_lists:
                    on = val > 0
                    rows = torch.arange(B, device=dev).unsqueeze(1).expand_as(idx)[on]
                    _tokens_per_feature(idx[on].long(), batch_tok.to(dev)[rows], H, tokens_per_feature)
            else:
                ops.sq_err_sum(sae(x)["reconstruction"].to(dev).contiguous(), x, sq)
                mask = _threshold_stats(model, x, H, counts, coact, with_lists, lists, batch_tok, partners)
                if with_lists:
                    nz = mask.nonzero(as_tuple=False)
                    _tokens_per_feature(nz[:, 1], batch_tok.to(dev)[nz[:, 0]], H, tokens_per_feature)
            global_index += B
            n_elements += x.numel()
    return {"mse_final": float(sq.item()) / max(n_elements, 1), "mse_per_level": None, "l0_per_level": None,
            "activation_counts": counts.cpu(), **_coactivation_result(coact, partners),
            "tokens_per_feature": lists.finish() if csr else tokens_per_feature, **_top_examples_result(examples)}
