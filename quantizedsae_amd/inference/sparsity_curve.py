"""Sparsity-fidelity curve of a top-k SAE: reconstruction error as a function of the test-time k, from ONE top-k pass.

``evaluate_dataset`` gives one point of the curve (the k the model was built with), and sweeping ``model.k`` costs one
encoder contraction per point although all points share it.  The top-k list of a row is ordered by (value descending, unit
ascending), so the selection at k' is the first k' entries of the list at K = max(ks); ``SparsityCurve`` selects once at K
through the model's own ``_select`` and hands the list to ``qsaec_prefix_errors_*`` (csrc/sparsity_curve.hip), which gathers
a row's dictionary rows once per four points and sums their chains side by side.  Every point is bit for bit the
reconstruction of the model rebuilt with ``top_k = k'``; the sums are fp64 in a fixed order and are read once, in
``finish()``.  It is the test-time k sweep of Gao et al. 2024 ("Scaling and evaluating sparse autoencoders").
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .. import torch_ops as T
from ..sae.base import as_f32c
from ..sae.baseline import BaselineSparseAutoencoder
from ..sae.binary import BinarySAE
from .evaluation import DatasetMoments, _rows
from .framework import SAEWrapper

__all__ = ["default_ks", "SparsityCurve", "sparsity_curve"]

MAX_K = 256
MAX_POINTS = 16


def default_ks(top_k: int) -> List[int]:
    """The powers of two up to 256 plus ``top_k`` (when it is 1 .. 256), ascending and distinct."""
    ks = {1 << p for p in range(9)}
    if 1 <= int(top_k) <= MAX_K:
        ks.add(int(top_k))
    return sorted(ks)


class SparsityCurve:
    """Running squared reconstruction error of a ``BinarySAE`` or ``BaselineSparseAutoencoder`` (or an ``SAEWrapper`` around
    one) at every k' of ``ks`` (default ``default_ks(top-k of the model)``, cut at hidden_dim).

    ``add(x)``: one selection at K = max(ks) on the path ``resolved_latent_path`` gives for the batch (no dense latent is
    written), one call of ``prefix_errors`` with the decoder description ``forward()`` would resolve (BinarySAE: the packed
    dictionary or the soft table, the baseline: its table), and the batch's moments for the variance.  Rows are cut into
    groups of ``group_rows`` from the first row of every call and a group holding a NaN is skipped, as ``DatasetMoments``
    does.  ``finish()`` makes one host copy and returns ``ks``, ``sse``, ``mse`` (per element), ``fvu`` = mse / variance
    (``evaluate_dataset``'s definition), ``rows``, ``skipped_rows``, ``variance`` and ``model_k``."""

    def __init__(self, sae_or_model, ks: Optional[Sequence[int]] = None, group_rows: int = 1024) -> None:
        model = sae_or_model.model if isinstance(sae_or_model, SAEWrapper) else sae_or_model
        if not isinstance(model, (BinarySAE, BaselineSparseAutoencoder)):
            raise TypeError(f"SparsityCurve: expected a BinarySAE or a BaselineSparseAutoencoder, got {type(model).__name__}: "
                            "the sparsity of the other classes is not a k (a threshold or a set of levels decides what is "
                            "active); compute_reconstruction_error_by_level gives the matryoshka levels")
        self.model = model
        H, D = model.encoder.linear.weight.shape
        self.hidden_dim, self.input_dim = int(H), int(D)
        self.model_k = int(model.top_k if isinstance(model, BinarySAE) else model.topk)
        if ks is None:
            ks = [k for k in default_ks(self.model_k) if k <= H]
        ks = [int(k) for k in ks]
        if not 1 <= len(ks) <= MAX_POINTS:
            raise ValueError(f"SparsityCurve: {len(ks)} points; 1 .. {MAX_POINTS} are supported")
        if ks[0] < 0 or any(b <= a for a, b in zip(ks, ks[1:])):
            raise ValueError(f"SparsityCurve: ks = {ks} must be ascending, distinct and >= 0")
        if ks[-1] > min(MAX_K, H):
            raise ValueError(f"SparsityCurve: the largest k = {ks[-1]} exceeds {min(MAX_K, H)} (the kernels' limit of {MAX_K} "
                             f"and hidden_dim = {H})")
        self.ks = ks
        self.group_rows = int(group_rows)
        if self.group_rows < 1:
            raise ValueError(f"SparsityCurve: group_rows must be >= 1, got {group_rows}")
        self.device = model.encoder.linear.weight.device
        self._sums: Optional[torch.Tensor] = None
        self._counts: Optional[torch.Tensor] = None
        self._moments: Optional[DatasetMoments] = None

    def _state(self, device) -> None:
        if self._sums is None:
            self._sums = torch.zeros((len(self.ks),), dtype=torch.float64, device=device)
            self._counts = torch.zeros((2,), dtype=torch.int64, device=device)
            self._moments = DatasetMoments(self.input_dim, self.group_rows, device)

    def _decoder(self):
        """-> (decoder description, decoder bias): what forward() decodes from"""
        m = self.model
        if isinstance(m, BinarySAE):
            dec = m.decoder
            return m._fused_decoder(dec.resolved_decode_mode() == "hard"), dec.bias.detach()
        return ("table", m._table(), 1.0), m.decoder.bias.detach()

    def _path(self, rows: int, K: int) -> str:
        return self.model._select_path(rows, K, "SparsityCurve")

    def add(self, x: torch.Tensor, recon_out: Optional[torch.Tensor] = None) -> None:
        """Add the rows of ``x`` [rows, input_dim] (on the device).  ``recon_out``: an fp32 [len(ks), rows, input_dim] tensor
        that receives every point's reconstruction (tests and inspection; the curve itself never writes one)."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.input_dim:
            raise ValueError(f"x: expected a tensor [rows, {self.input_dim}], got {tuple(getattr(x, 'shape', ()))}")
        if not x.is_cuda:
            raise RuntimeError(f"x: quantizedsae_amd runs on MI355X only; tensor is on {x.device} (no CPU fallback exists)")
        if x.shape[0] == 0:
            return
        with torch.no_grad():
            xf = as_f32c(x.detach())
            self._state(xf.device)
            K = self.ks[-1]
            if K == 0:
                idx = torch.empty((xf.shape[0], 0), dtype=torch.int32, device=xf.device)
                val = torch.empty((xf.shape[0], 0), dtype=torch.float32, device=xf.device)
            else:
                idx, val, _ = self.model._select(xf, K, self._path(xf.shape[0], K), False)
            decoder, bias = self._decoder()
            T.prefix_errors(xf, idx, val, self.ks, decoder, bias, self.group_rows, self._sums, self._counts, recon_out)
            self._moments.add(xf)

    def finish(self) -> Dict[str, Any]:
        if self._sums is None:
            raise ValueError("SparsityCurve: no row was added")
        m = self._moments
        state = torch.cat([self._sums, self._counts.view(torch.float64), m.sums.reshape(-1),
                           m.counts.view(torch.float64)]).cpu().numpy()                         # the one host copy
        n, D = len(self.ks), self.input_dim
        sse = state[:n].copy()
        rows, skipped = (int(v) for v in state[n:n + 2].view(np.int64))
        msums = state[n + 2:n + 2 + 3 * D].reshape(3, D)
        mrows, mskipped = (int(v) for v in state[n + 2 + 3 * D:].view(np.int64))
        if (rows, skipped) != (mrows, mskipped):
            raise RuntimeError(f"SparsityCurve: the curve kept {rows} rows and skipped {skipped}, the moments {mrows} and {mskipped}")
        if rows == 0:
            raise ValueError(f"SparsityCurve: no row was kept ({skipped} skipped for NaN): the curve is undefined")
        total = rows * D
        asc = lambda v: float(np.cumsum(v)[-1])                # noqa: E731  (the ascending-d sum, as DatasetMoments.finish)
        mean = asc(msums[0]) / total
        variance = asc(msums[1]) / total - mean * mean
        mse = sse / total
        with np.errstate(divide="ignore", invalid="ignore"):
            fvu = mse / variance if variance != 0 else np.full_like(mse, np.nan)
        self._result = {"ks": list(self.ks), "sse": sse, "mse": mse, "fvu": fvu, "rows": rows, "skipped_rows": skipped,
                        "variance": variance, "model_k": self.model_k}
        return self._result

    def k_at(self, mse: Optional[float] = None, fvu: Optional[float] = None) -> Optional[int]:
        """The smallest listed k whose ``mse`` (or ``fvu``) is at or below the target, or None; exactly one target."""
        if (mse is None) == (fvu is None):
            raise ValueError("k_at: give exactly one of mse= and fvu=")
        r = self.finish()
        values, target = (r["mse"], mse) if mse is not None else (r["fvu"], fvu)
        for k, v in zip(r["ks"], values):
            if v <= target:
                return k
        return None


def sparsity_curve(sae, loader: Iterable[Any], ks: Optional[Sequence[int]] = None, group_rows: int = 1024) -> Dict[str, Any]:
    """One pass over a loader of batches ``[rows, D]``, the way ``evaluate_dataset`` does it: -> ``SparsityCurve.finish()``."""
    if isinstance(sae, SAEWrapper):
        sae.eval()
    curve = SparsityCurve(sae, ks, group_rows)
    seen = False
    for batch in loader:
        curve.add(_rows(batch).to(curve.device))
        seen = True
    if not seen:
        raise ValueError("empty loader")
    return curve.finish()
