"""Revive the dead units of a top-k dictionary from the rows it reconstructs worst (csrc/resample.hip; DESIGN.md section
4.28).  ``FeatureActivity.summary(window, dead_list=True)`` says which units are dead; a unit that has fallen out of every
row's top-k gets no gradient from the HIP backward, which visits selected entries only, and never comes back by itself.
The reference carries a ``dead_neuron_threshold`` that nothing reads.

``resample_dead`` is the published step (Bricken et al., "Towards Monosemanticity"): every dead unit draws one row of the
batch with probability proportional to the row's squared loss, its encoder row becomes the row's residual direction at
``encoder_scale`` times the alive units' mean norm, its decoder atom the unit direction (``BaselineSparseAutoencoder``) or
the direction quantized to the model's n-bit two's-complement integers, written as logits of the checkpoint's own magnitude
(``BinarySAE``), and the optimizer's moments are cleared where it wrote.  Five kernel calls chained on the device; nothing
is read back unless the caller looks at the report.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import torch_ops as ops
from ..sae import BaselineSparseAutoencoder, BinarySAE

__all__ = ["resample_dead", "ResampleReport"]

_WORDS = ("dead", "revived", "duplicate", "degenerate", "no_weight", "skipped")


class ResampleReport:
    """What one ``resample_dead`` call did.  ``block`` is the int64 [8] report on the device (None for an empty dead list)
    and ``rows`` the int32 [n] row of every dead unit (-1: the batch had no weight to draw from, -2: an earlier unit owns the
    row).  The counts are read from the device on first use, one host copy:

    ``dead`` units in the list; ``revived`` rewritten; ``duplicate`` drew a row that an earlier unit owns and stay dead until
    the next step; ``degenerate`` drew a row equal to the decoder bias (or of non-finite norm) and are left untouched;
    ``no_weight`` had nothing to draw from; ``skipped`` entries of the list were out of range or out of order."""

    def __init__(self, block: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
        self.block, self.rows = block, rows
        self._counts = None if block is not None else [0] * len(_WORDS)

    def counts(self) -> dict:
        if self._counts is None:
            self._counts = self.block.tolist()[:len(_WORDS)]
        return dict(zip(_WORDS, self._counts))

    def __getattr__(self, name):
        if name in _WORDS:
            return self.counts()[name]
        raise AttributeError(name)

    def metrics(self) -> dict:
        """The keys a Trainer step logs"""
        c = self.counts()
        return {"resample_dead": c["dead"], "resampled_features": c["revived"], "resample_duplicates": c["duplicate"],
                "resample_degenerate": c["degenerate"], "resample_no_weight": c["no_weight"], "resample_skipped": c["skipped"]}

    def __repr__(self):
        return "ResampleReport(" + ", ".join(f"{k}={v}" for k, v in self.counts().items()) + ")"


def resample_line(report: ResampleReport) -> str:
    """One printed line of a report"""
    c = report.counts()
    return (f"  resample: revived={c['revived']}/{c['dead']} dead, duplicates={c['duplicate']}, degenerate={c['degenerate']}, "
            f"no_weight={c['no_weight']}, skipped={c['skipped']}")


def _moments(optimizer, params):
    """(exp_avg, exp_avg_sq) of every parameter the optimizer holds state for, None otherwise; ``step`` is not touched.
    torch.optim.Adam and quantizedsae_amd.optim.Adam share the names."""
    out = []
    for p in params:
        state = optimizer.state.get(p) if optimizer is not None else None
        for name in ("exp_avg", "exp_avg_sq"):
            t = state.get(name) if state else None
            out.append(t if isinstance(t, torch.Tensor) else None)
    return tuple(out)


def resample_dead(model, dead_indices: torch.Tensor, x: torch.Tensor, *, optimizer=None, activity=None,
                  u: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, encoder_scale: float = 0.2,
                  logit_scale: Optional[float] = None, recon: Optional[torch.Tensor] = None) -> ResampleReport:
    """Rewrite the units ``dead_indices`` (int32, ascending, on the device: ``ActivitySummary.dead_indices``) of a
    ``BaselineSparseAutoencoder`` or ``BinarySAE`` in place from the candidate rows ``x`` fp32 [N, D].

    ``u``: one fp64 uniform in [0, 1) per dead unit; by default ``torch.rand`` from ``generator``, which must be a generator
    of the caller's own on the model's device -- the default generator is never touched, so a loader's shuffles stay what
    they were.  ``recon``: the model's reconstruction of ``x`` if the caller has it (``forward_compact`` under ``no_grad``
    otherwise).  ``optimizer``: its ``exp_avg`` / ``exp_avg_sq`` are zeroed at the written positions.  ``activity``: a
    ``FeatureActivity`` whose ``last`` of every revived unit becomes ``rows_seen``, so that the unit gets a full window before
    it can count as dead again.  ``logit_scale`` (BinarySAE): the magnitude of the written logits; default: the alive rows'
    mean |logit|, which follows the checkpoint's own polarisation -- a saturated +-16 would revive an atom whose sigmoid
    gradient is gone.  With ``n_bits == 1`` the format holds {0, -1} only, so a revived atom keeps the negative half of its
    direction.

    The kernels write through raw pointers; the derived copies of the weights are dropped at the end
    (``model.invalidate_packed()``).  An empty list is a no-op that launches nothing."""
    if not isinstance(model, (BaselineSparseAutoencoder, BinarySAE)):
        raise ValueError(f"resample_dead: resampling is built for BaselineSparseAutoencoder and BinarySAE, the two top-k models; "
                         f"got {type(model).__name__}")
    n = int(dead_indices.numel())
    if n == 0:
        return ResampleReport()
    lin, dec = model.encoder.linear, model.decoder
    if u is None:
        if generator is None:
            raise ValueError("resample_dead: pass the uniforms u or a private torch.Generator on the model's device (the "
                             "default generator is not used)")
        u = torch.rand((n,), dtype=torch.float64, device=lin.weight.device, generator=generator)
    if u.numel() != n:
        raise ValueError(f"resample_dead: {u.numel()} uniforms for {n} dead units")
    binary = isinstance(model, BinarySAE)
    with torch.no_grad():
        if recon is None:
            recon = model.forward_compact(x)[2]
        W, b, Wd, bd = lin.weight.detach(), lin.bias.detach(), dec.weight.detach(), dec.bias.detach()
        rows, block = ops.resample_draw(ops.resample_row_weights(x, recon), u)
        stats = ops.resample_alive_stats(W, Wd if binary else None, dead_indices, dec.n_bits if binary else 8)
        moments = _moments(optimizer, (lin.weight, lin.bias, dec.weight))
        last = activity.last if activity is not None else None
        seen = activity.rows_seen if activity is not None else 0
        if binary:
            ops.resample_write_binary(W, b, Wd, dead_indices, rows, x, bd, stats, block, dec.n_bits, moments, last, seen,
                                      encoder_scale, logit_scale)
        else:
            ops.resample_write_table(W, b, Wd, dead_indices, rows, x, bd, stats, block, moments, last, seen, encoder_scale)
        model.invalidate_packed()
    return ResampleReport(block, rows)
