"""Decoder dictionaries compared on the GPU: cosine similarities between the atoms of two SAEs.

Reference: scripts/analysis/analyze_sae.py:24-91 (``_decoder_features``, ``decoder_cosine_similarity`` and the mean of
the top-100 row maxima), analyze_cosine_sim.py (directional overlap, ``a_to_b_max``) and data/load_baseline.py:102-122
(``analyze_cosine_similarities``: statistics over the pairs i < j of one dictionary).  The reference brings the
dictionaries to the host and reduces the whole [Na, Nb] product with eager ops; here one launch of
``qsae_cosine_compare`` (csrc/dictionary.hip) reduces every tile of the exact-fp32 MFMA contraction as it finishes, and
the matrix exists only when it is asked for.

Precision: every cosine returned is within 1e-5 of fp64 on the same atoms; an argmax points at an
entry whose fp64 value is within 2e-5 of the fp64 row maximum.  Indices are not promised to equal the reference's (its
sgemm summation order is unspecified); ties go to the lowest index.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, List, Optional

import torch
from torch import nn

from .. import torch_ops as T
from ..sae.binary import BinarySAE
from ..sae.quantized_matryoshka import QuantizedMatryoshkaSAE
from ..sae.residual_quantized import ResidualQuantizedSAE

__all__ = ["decoder_atoms", "decoder_cosine_similarity", "compare_decoders"]


def _model(sae) -> nn.Module:
    return sae.model if hasattr(sae, "model") and isinstance(sae.model, nn.Module) else sae


def _input_dim(model: nn.Module) -> int:
    """analyze_sae.py:_input_dim: input_dim, else the decoder bias size, else the first stage's decoder bias size."""
    if hasattr(model, "input_dim"):
        return int(model.input_dim)
    dec = getattr(model, "decoder", None)
    if dec is not None and getattr(dec, "bias", None) is not None:
        return int(dec.bias.numel())
    saes = getattr(model, "saes", None)
    if saes is not None and len(saes) > 0:
        first = getattr(saes[0], "decoder", None)
        if first is not None and getattr(first, "bias", None) is not None:
            return int(first.bias.numel())
    raise ValueError("Unable to determine input dimension for SAE.")


def _dictionary_tensors(model: nn.Module) -> List[torch.Tensor]:
    """The tensors analyze_sae.py:_decoder_features selects from ``decoder_dictionary()``, built on the model's device:
    the ``effective_weight`` entries where there are any (matryoshka, residual: weight + weight_mirror per stage, in
    stage order), else ``weight`` (binary: quantization_step * integer weights; linear decoders: decoder.weight)."""
    with torch.no_grad():
        if isinstance(model, ResidualQuantizedSAE):
            return [s.decoder.weight.detach() + s.decoder.weight_mirror.detach() for s in model.saes]
        if isinstance(model, QuantizedMatryoshkaSAE):
            return [model.decoder.weight.detach() + model.decoder.weight_mirror.detach()]
        if isinstance(model, BinarySAE):
            dec = model.decoder
            return [dec.quantization_step * dec.quantized_int_weights().to(torch.float32)]
        return [model.decoder.weight.detach()]


def decoder_atoms(sae) -> torch.Tensor:
    """Decoder atoms ``[n_atoms, D]`` fp32 on the model's device: the rows analyze_sae.py:_decoder_features takes from
    ``decoder_dictionary()``, without the host round trip.

    ``sae`` is an ``SAEWrapper`` (``load_sae``) or the module itself.  Per model:
      * BinarySAE: ``quantization_step * quantized_int_weights()`` (the integer table is unpacked on the device) -- the
        tensor ``framework._decoder_binary`` returns;
      * QuantizedMatryoshkaSAE: ``weight + weight_mirror``;
      * ResidualQuantizedSAE: every stage's ``weight + weight_mirror``, concatenated in stage order;
      * baseline and the other linear decoders (t_sae): ``decoder.weight``.
    Orientation follows the reference rule exactly: a tensor whose dim 1 equals the input dimension is taken as is, else
    one whose dim 0 equals it is transposed, else it is taken as is.  So a square dictionary (H == D) is NOT transposed,
    whatever its layout."""
    model = _model(sae)
    D = _input_dim(model)
    feats = []
    for t in _dictionary_tensors(model):
        t = t.to(torch.float32)
        if t.shape[1] == D:
            feats.append(t)
        elif t.shape[0] == D:
            feats.append(t.t())
        else:
            feats.append(t)
    return torch.cat(feats, dim=0).contiguous()


def _check_pair(a: torch.Tensor, b: torch.Tensor) -> None:
    if a.device != b.device:
        raise ValueError(f"decoder atoms live on different devices ({a.device} vs {b.device})")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"decoder atoms have different sizes (D = {a.shape[1]} vs {b.shape[1]})")


def decoder_cosine_similarity(lhs, rhs) -> torch.Tensor:
    """Pairwise cosine similarities between the decoder atoms of two SAEs, ``[Na, Nb]`` fp32 -- the name, arguments and
    meaning of analyze_sae.py:59-69 (``F.normalize`` rows, then the product).  Unlike the reference the result stays on
    the models' device (call ``.cpu()`` for the reference's placement)."""
    a, b = decoder_atoms(lhs), decoder_atoms(rhs)
    _check_pair(a, b)
    return T.cosine_compare(a, b, (), 0, True)[6]


def _decode_keys(keys: torch.Tensor):
    """Keys (mono(c) << 32 | ~index, 0 = none) -> (fp32 values, int64 indices); none -> (-inf, -1)."""
    hi = (keys >> 32) & 0xFFFFFFFF
    lo = keys & 0xFFFFFFFF
    bits = torch.where(hi >= 0x80000000, hi - 0x80000000, 0xFFFFFFFF - hi)       # undo the order-preserving map
    bits = torch.where(bits >= 0x80000000, bits - (1 << 32), bits).to(torch.int32)
    vals = bits.view(torch.float32)
    idx = 0xFFFFFFFF - lo
    none = keys == 0
    vals = torch.where(none, torch.full_like(vals, -math.inf), vals)
    idx = torch.where(none, torch.full_like(idx, -1), idx)
    return vals, idx


def _mono_to_float(k: int) -> float:
    bits = k - 0x80000000 if k >= 0x80000000 else 0xFFFFFFFF - k
    return torch.tensor([bits - (1 << 32) if bits >= 0x80000000 else bits], dtype=torch.int32).view(torch.float32).item()


def compare_decoders(lhs, rhs=None, *, thresholds: Iterable[float] = (0.5, 0.9), top: int = 100, bins: int = 0,
                     return_matrix: bool = False) -> Dict[str, Any]:
    """Cosine-similarity statistics of the decoder atoms of ``lhs`` (A) against ``rhs`` (B), in one kernel pass that
    forms no [Na, Nb] matrix unless ``return_matrix``.  ``lhs`` / ``rhs`` are SAEs (wrapper or module) or atom tensors
    ``[n, D]``.  ``rhs=None`` is self mode: the pairs i < j of one dictionary (data/load_baseline.py:102-122), and each
    atom's nearest *other* atom.

    Keys of the result (tensors on the device, scalars as Python numbers):
      mean, std, min, max         over all pairs (self mode: i < j); std is the population std (numpy's default)
      a_to_b_max / a_to_b_argmax  fp32 / int64 [Na]: best B atom of each A atom (analyze_cosine_sim.py:44)
      b_to_a_max / b_to_a_argmax  fp32 / int64 [Nb]: best A atom of each B atom (self mode: the same as a_to_b)
      mean_top_k                  mean of the `top` largest a_to_b_max (analyze_sae.py:84-91: k = min(top, Nb))
      count_above                 {t: number of pairs with c > t}  (strict, as load_baseline.py:118)
      overlap                     {t: fraction of A atoms whose a_to_b_max > t}
    with ``bins`` (<= 4096): ``histogram`` (int64 [bins] over [-1, 1], values just past +-1 in the end bins),
    ``bin_edges`` (fp64 [bins + 1]) and ``median`` / ``p25`` / ``p75``: the centre of the bin that holds the quantile,
    i.e. within one bin width (2 / bins) of the exact value; with ``return_matrix``: ``matrix`` (fp32 [Na, Nb]).
    An atom with no partner (self mode, one atom) has max -inf and argmax -1; with no pair at all mean / std / min / max
    are nan.  lhs and rhs on different devices or with different D raise ValueError."""
    a = lhs if isinstance(lhs, torch.Tensor) else decoder_atoms(lhs)
    b = None
    if rhs is not None:
        b = rhs if isinstance(rhs, torch.Tensor) else decoder_atoms(rhs)
        _check_pair(a, b)
    thresholds = [float(t) for t in thresholds]
    row, col, moments, extrema, counts, hist, matrix = T.cosine_compare(a, b, thresholds, bins, return_matrix)
    Na = a.shape[0]
    Nb = Na if b is None else b.shape[0]
    a_max, a_arg = _decode_keys(row)
    if b is None:
        b_max, b_arg = a_max, a_arg
        npairs = Na * (Na - 1) // 2
    else:
        b_max, b_arg = _decode_keys(col)
        npairs = Na * Nb
    mom = moments.tolist()
    ext = extrema.tolist()
    if npairs > 0:
        mean = mom[0] / npairs
        std = math.sqrt(max(mom[1] / npairs - mean * mean, 0.0))
    else:
        mean = std = math.nan
    vmax = _mono_to_float(ext[0]) + 0.0 if ext[0] else math.nan
    vmin = _mono_to_float(0xFFFFFFFF - ext[1]) + 0.0 if ext[1] else math.nan
    k = min(int(top), Nb, Na)
    out: Dict[str, Any] = {
        "mean": mean, "std": std, "min": vmin, "max": vmax, "n_pairs": npairs,
        "a_to_b_max": a_max, "a_to_b_argmax": a_arg, "b_to_a_max": b_max, "b_to_a_argmax": b_arg,
        "mean_top_k": torch.topk(a_max, k).values.double().mean().item() if k > 0 else math.nan,
        "count_above": {t: int(c) for t, c in zip(thresholds, counts.tolist())},
        "overlap": {t: (a_max > t).double().mean().item() for t in thresholds},
    }
    if bins:
        out["histogram"] = hist
        out["bin_edges"] = torch.linspace(-1.0, 1.0, bins + 1, dtype=torch.float64)
        cum = torch.cumsum(hist, 0).tolist()
        total = cum[-1]
        for name, q in (("p25", 0.25), ("median", 0.5), ("p75", 0.75)):
            if total == 0:
                out[name] = math.nan
                continue
            target = q * total
            bi = next(i for i, cv in enumerate(cum) if cv >= target)
            out[name] = -1.0 + (bi + 0.5) * (2.0 / bins)
    if return_matrix:
        out["matrix"] = matrix
    return out
