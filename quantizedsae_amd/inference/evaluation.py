"""The two evaluation reports on the device.

Reference: scripts/evaluation/estimate_quantization_error.py (how far a trained BinarySAE's hard integer dictionary is
from the probability-weighted one it was trained with) and scripts/evaluation/estimate_baseline_error.py (variance and
predict-zero MSE of the hidden-state dataset, what every reconstruction MSE is read against).

``quantization_error`` is one pass over the decoder logits (``qsae_quantization_error``, csrc/evaluation.hip): no [H, D]
temporary, fp64 sums in a fixed order, and one device-to-host copy of a 384-byte result block.  ``DatasetMoments`` keeps
per-column fp64 sums on the device (``qsae_dataset_moments_add``) and reads them once in ``finish()``.

Deliberate differences from the reference scripts:

* sums are fp64 in a fixed order, where the reference reduces fp32 tensors (quantization) or adds one fp32 ``.sum().item()``
  per batch (moments);
* the NaN rule of the moments -- ``if torch.isnan(batch).any(): continue`` at the DataLoader's batch size of 1024 -- is kept
  as *groups of ``group_rows`` rows counted from the first row of every ``add`` call*, whatever the caller's batch size;
* with no row kept, ``DatasetMoments.finish()`` raises ``ValueError`` where the reference divides by zero.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, List, Optional

import numpy as np
import torch

from .. import torch_ops as T
from ..sae.binary import BinarySAE
from .framework import SAEWrapper, _default_device, _ensure_tensor

__all__ = ["quantization_error", "format_quantization_report", "DatasetMoments", "estimate_baseline_error", "evaluate_dataset"]

_SIG_GT_BITS = 0x33C00001        # sigmoid(w) > 0.5 in fp32  <=>  w >= this fp32 (csrc/common.h)


def _key_value(key: int) -> float:
    """The fp32 value behind the high word of a key (the inverse of the order-preserving map; NaN for its top code)."""
    m = (key >> 32) & 0xFFFFFFFF
    if m == 0xFFFFFFFF:
        return float("nan")
    u = (m & 0x7FFFFFFF) if m & 0x80000000 else (~m & 0xFFFFFFFF)
    return float(np.array([u], np.uint32).view(np.float32)[0])


def _bit_details(logits: np.ndarray, step: float) -> List[Dict[str, Any]]:
    """The per-bit table of one entry (collect_bit_details), fp32 host arithmetic on its n logits."""
    n = logits.size
    l32 = logits.astype(np.float32)
    with np.errstate(over="ignore"):
        prob = (np.float32(1.0) / (np.float32(1.0) + np.exp(-l32))).astype(np.float32)
    hard = (l32 >= np.array([_SIG_GT_BITS], np.uint32).view(np.float32)[0]).astype(np.float32)
    bw = np.float32(2.0) ** np.arange(n, dtype=np.float32)
    bw[-1] *= -1
    s = np.float32(step)
    fc, qc = (prob * bw) * s, (hard * bw) * s
    return [{"bit_index": b, "logit": float(l32[b]), "prob": float(prob[b]), "hard": int(hard[b]), "bit_weight": float(bw[b]),
             "float_contrib": float(fc[b]), "quant_contrib": float(qc[b])} for b in range(n)]


def quantization_error(sae_or_model, margin_logit: float = math.log(3.0)) -> Dict[str, Any]:
    """Statistics of ``W_quant - W_float`` of a BinarySAE (or an ``SAEWrapper`` around one; ``TypeError`` otherwise).

    The reference's keys: ``mse``, ``mean_abs``, ``max_abs``, ``l2_norm``; ``float_mean/std/min/max/l2_norm`` and
    ``quant_*`` alike (``std`` is the population one); and its ``find_max_diff_entry`` fields ``row_index``,
    ``col_index``, ``w_float_value``, ``w_quant_value``, ``signed_diff``, ``abs_diff``, ``bit_details`` (of equal largest
    differences the lowest flat index; the two values and ``bit_details`` are fp32 host arithmetic on that entry's n logits).
    Beyond the reference: ``unit_err_sq`` (fp64 [H] on the device: the squared error per atom), per bit plane
    ``mean_abs_logit_per_bit`` (the trainer's mag_LSB .. mag_MSB), ``polarize_per_bit`` (mean p (1 - p)) and
    ``undecided_per_bit`` (logits with ``|logit| < margin_logit``; log 3 = a bit probability inside (0.25, 0.75)),
    ``polarize_loss`` (what the training forward reports), ``n_nan`` and ``soft_gap`` = max |diff| / step, the packer's
    number (+inf when a logit is NaN, as there).  NaN logits propagate into the float-side statistics."""
    model = sae_or_model.model if isinstance(sae_or_model, SAEWrapper) else sae_or_model
    if not isinstance(model, BinarySAE):
        raise TypeError(f"quantization_error: expected a BinarySAE, got {type(model).__name__} (only the binary decoder has a "
                        "soft and a hard form)")
    dec = model.decoder
    D, n, H = dec.out_features, dec.n_bits, dec.in_features
    step = float(dec.quantization_step)
    with torch.no_grad():
        block, unit_err_sq = T.quantization_error(dec.weight.detach(), D, n, step, float(margin_logit))
    f = block.cpu().numpy()                                   # the one device-to-host copy
    i = f.view(np.int64)
    count = float(H * D)
    n_nan = int(i[11])
    key = int(f.view(np.uint64)[10])
    flat = (~key) & 0xFFFFFFFF
    row, col = divmod(flat, D)
    max_abs = _key_value(key)

    def matrix(prefix, s, s2, lo, hi):
        mean = s / count
        return {f"{prefix}_mean": mean, f"{prefix}_std": math.sqrt(max(s2 / count - mean * mean, 0.0)) if s2 == s2 else float("nan"),
                f"{prefix}_min": lo, f"{prefix}_max": hi, f"{prefix}_l2_norm": math.sqrt(s2) if s2 == s2 else float("nan")}

    nan = float("nan")
    out: Dict[str, Any] = {"mse": float(f[0]) / count, "mean_abs": float(f[1]) / count, "max_abs": max_abs,
                           "l2_norm": math.sqrt(float(f[0])) if f[0] == f[0] else nan}
    out.update(matrix("float", float(f[2]), float(f[3]), nan if n_nan else float(f[6]), nan if n_nan else float(f[7])))
    out.update(matrix("quant", float(f[4]), float(f[5]), float(f[8]), float(f[9])))
    details = _bit_details(f[40:40 + n], step)
    s32 = np.float32(step)
    soft = np.float32(0.0)
    for b in details:                                        # the kernel's chain, on the host's expf
        soft = np.float32(soft + np.float32(np.float32(b["prob"]) * np.float32(b["bit_weight"])))
    code = sum(b["hard"] << b["bit_index"] for b in details)
    hard = code - ((code >> (n - 1)) << n)
    w_float, w_quant = float(np.float32(s32 * soft)), float(np.float32(s32 * np.float32(hard)))
    out.update({"row_index": int(row), "col_index": int(col), "w_float_value": w_float, "w_quant_value": w_quant,
                "signed_diff": w_quant - w_float, "abs_diff": max_abs, "bit_details": tuple(details)})
    per_plane = float(H * D)
    pol = [float(v) / per_plane for v in f[24:24 + n]]
    out.update({"unit_err_sq": unit_err_sq,
                "mean_abs_logit_per_bit": [float(v) / per_plane for v in f[16:16 + n]],
                "polarize_per_bit": pol,
                "polarize_loss": sum(float(v) * float(2 ** b) for b, v in enumerate(f[24:24 + n])) / (per_plane * n),
                "undecided_per_bit": [int(v) for v in i[32:32 + n]],
                "n_nan": n_nan,
                "soft_gap": float("inf") if n_nan else max_abs / step})
    return out


def format_quantization_report(result: Dict[str, Any]) -> str:
    """The text of the reference's report (format_report) for a ``quantization_error`` result."""
    r = result
    e = lambda key: f"{r[key]:.6e}"                          # noqa: E731
    lines = ["=== Decoder Weight Quantization Report ===",
             "MSE(W_quant - W_float):    " + e("mse"),
             "Mean |ΔW|:                 " + e("mean_abs"),
             "Max  |ΔW|:                 " + e("max_abs"),
             "L2  ||ΔW||:                " + e("l2_norm"),
             ""]
    for name in ("float", "quant"):
        lines.append(f"W_{name} mean/std/min/max: (" + ", ".join(e(f"{name}_{k}") for k in ("mean", "std", "min", "max")) + ")")
    lines += ["", "||W_float||_2: " + e("float_l2_norm"), "||W_quant||_2: " + e("quant_l2_norm"), "",
              "Largest absolute difference entry:",
              f"  Indices (hidden, input): ({r['row_index']}, {r['col_index']})",
              "  W_float value:           " + e("w_float_value"),
              "  W_quant value:           " + e("w_quant_value"),
              "  Signed diff:             " + e("signed_diff"),
              "  Absolute diff:           " + e("abs_diff"),
              "",
              "  Bit-level details (index, logit, prob, hard, bit_weight, float_contrib, quant_contrib):"]
    for b in r["bit_details"]:
        lines.append(f"    bit {b['bit_index']}: logit={b['logit']:.6e}, prob={b['prob']:.6e}, hard={b['hard']}, "
                     f"weight={b['bit_weight']:.6e}, float={b['float_contrib']:.6e}, quant={b['quant_contrib']:.6e}")
    return "\n".join(lines)


class DatasetMoments:
    """Running per-column fp64 sums of a dataset ``[rows, input_dim]`` on ``device``: Σx, Σx², and Σ(recon − x)² when
    reconstructions are fed along.

    ``add(x, recon=None)``: ``x`` fp32, fp16 or bf16 on the device (converted in registers), ``recon`` fp32.  The rows of
    one call are cut into groups of ``group_rows`` from the call's first row; a group holding a NaN in ``x`` is skipped
    whole (the reference's NaN rule at its DataLoader batch size of 1024); inf is summed.  Either every ``add`` of one
    state carries ``recon`` or none does.  The sums do not depend on how the rows were cut into calls as long as the cuts
    fall on multiples of ``group_rows``.  ``merge(other)`` adds another state (another device's share); ``finish()`` reads
    the state once and returns the reference's five keys and the per-dimension numbers."""

    def __init__(self, input_dim: int, group_rows: int = 1024, device=None) -> None:
        self.input_dim, self.group_rows = int(input_dim), int(group_rows)
        if self.input_dim < 1 or self.group_rows < 1:
            raise ValueError(f"input_dim and group_rows must be positive, got {input_dim} and {group_rows}")
        self.device = _default_device(device)
        self.sums = torch.zeros((3, self.input_dim), dtype=torch.float64, device=self.device)
        self.counts = torch.zeros((2,), dtype=torch.int64, device=self.device)
        self.with_recon: Optional[bool] = None

    def _mode(self, with_recon: bool) -> None:
        if self.with_recon is None:
            self.with_recon = with_recon
        elif self.with_recon != with_recon:
            raise ValueError("DatasetMoments: either every add() of one state carries recon or none does")

    def add(self, x: torch.Tensor, recon: Optional[torch.Tensor] = None) -> None:
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.input_dim:
            raise ValueError(f"x: expected a tensor [rows, {self.input_dim}], got {tuple(getattr(x, 'shape', ()))}")
        if not x.is_cuda:
            raise RuntimeError(f"x: quantizedsae_amd runs on MI355X only; tensor is on {x.device} (no CPU fallback exists)")
        if x.shape[0] == 0:
            return
        self._mode(recon is not None)
        T.dataset_moments_add(x, recon, self.group_rows, self.sums, self.counts)

    def merge(self, other: "DatasetMoments") -> None:
        if other.input_dim != self.input_dim:
            raise ValueError("merge: states of different input_dim")
        if other.with_recon is not None:
            self._mode(other.with_recon)
        self.sums += other.sums.to(self.device)
        self.counts += other.counts.to(self.device)

    def finish(self) -> Dict[str, Any]:
        state = torch.cat([self.sums.reshape(-1), self.counts.view(torch.float64)]).cpu().numpy()    # one copy
        D = self.input_dim
        sums = state[:3 * D].reshape(3, D)
        rows, skipped = (int(v) for v in state[3 * D:].view(np.int64))
        if rows == 0:
            raise ValueError(f"DatasetMoments: no row was kept ({skipped} skipped for NaN): the moments are undefined")
        total = rows * D
        asc = lambda v: float(np.cumsum(v)[-1])                # noqa: E731  (the ascending-d sum)
        s1, s2 = asc(sums[0]), asc(sums[1])
        mean = s1 / total
        variance = s2 / total - mean * mean
        mean_d = sums[0] / rows
        with np.errstate(invalid="ignore"):                    # an inf column: inf - inf
            var_d = sums[1] / rows - mean_d * mean_d
        out: Dict[str, Any] = {"mean": mean, "variance": variance, "baseline_mse_zeros": s2 / total, "baseline_mse_mean": variance,
                               "total_samples": total, "rows": rows, "skipped_rows": skipped,
                               "mean_per_dim": torch.from_numpy(mean_d.copy()), "variance_per_dim": torch.from_numpy(var_d.copy())}
        if self.with_recon:
            mse_d = sums[2] / rows
            mse = asc(sums[2]) / total
            with np.errstate(divide="ignore", invalid="ignore"):
                fvu_d = mse_d / var_d
            out.update({"mse": mse, "mse_per_dim": torch.from_numpy(mse_d.copy()),
                        "fvu": mse / variance if variance != 0 else float("nan"), "fvu_per_dim": torch.from_numpy(fvu_d)})
        return out


def _rows(batch: Any) -> torch.Tensor:
    x = _ensure_tensor(batch)
    return x.reshape(-1, x.shape[-1]) if x.dim() != 2 else x


def estimate_baseline_error(batches: Iterable[Any], group_rows: int = 1024, device=None) -> Dict[str, Any]:
    """``estimate_baseline_error.py`` over any iterable of batches ``[rows, D]``: mean, variance, predict-zero and
    predict-mean MSE.  Each batch's rows are grouped from its first row (feed DataLoader batches of ``group_rows`` rows
    to get the reference's NaN rule exactly)."""
    moments = None
    for batch in batches:
        x = _rows(batch)
        if moments is None:
            moments = DatasetMoments(x.shape[1], group_rows, device)
        moments.add(x.to(moments.device))
    if moments is None:
        raise ValueError("empty loader")
    return moments.finish()


def evaluate_dataset(sae: SAEWrapper, loader: Iterable[Any], group_rows: int = 1024) -> Dict[str, Any]:
    """One pass: the dataset's moments and the SAE's reconstruction error against them -- ``mse``, ``fvu`` = mse / variance
    (the fraction of variance left unexplained) and both per input dimension, next to the baseline keys."""
    sae.eval()
    moments = None
    with torch.no_grad():
        for batch in loader:
            x = _rows(batch).to(sae.device)
            if moments is None:
                moments = DatasetMoments(x.shape[1], group_rows, sae.device)
            moments.add(x, sae.reconstruct(x))
    if moments is None:
        raise ValueError("empty loader")
    return moments.finish()
