"""JumpReLU for the two top-k models (Rajamanoharan et al. 2024, "Jumping Ahead: Improving Reconstruction Fidelity with JumpReLU
Sparse Autoencoders"): one learned threshold per dictionary unit, a unit fires where its pre-activation exceeds it, the
gradient passes straight through with a rectangle kernel of width ``bandwidth``, and an L0 penalty counts the firing units
(DESIGN.md section 4.36).

    jr = JumpReLU(model)                                      cap = min(256, hidden_dim) list places per row
    jr.calibrate(batch, k)                                    thresholds from what BatchTopK would select at k
    outputs = model.forward_train_jumprelu(batch, jr)         the tuple of forward_train with l0 appended
    idx, val, counts, recon = model.forward_jumprelu(x, jr)   evaluation
    ... = model.forward_train_jumprelu_dense(batch, jr)       the same two from the dense encoder: the thresholds applied to
    ... = model.forward_jumprelu_dense(x, jr)                 all pre-activations, no list and no certificate (section 4.37)

The selection runs over every row's top-``cap`` list (csrc/jumprelu.hip): the entries above their unit's threshold are moved to
the front of the row in list order, so every ragged row operation of BatchTopK takes the result unchanged.  It is JumpReLU
capped at ``cap`` per row and equals the uncapped one for every *certified* row -- a row whose last list entry lies below the
smallest threshold minus half the bandwidth; ``report[4]`` counts the rows that are not.

``bandwidth`` defaults to the paper's 0.001, which presumes inputs normalised as the paper's are (to a mean squared norm of
one per dimension, so that pre-activations are of order one); for inputs on another scale choose it in proportion.

The only parameter is ``log_threshold`` [H]; thresholds are its exponential, taken by torch, whose backward supplies the
factor theta.  Nothing is read back unless ``summary()`` is called.
"""
from __future__ import annotations

import math
import struct
from typing import Optional

import torch

from .. import torch_ops as ops
from ..sae.base import as_f32c, require_device_input
from ..sae.topk import TopKCore

__all__ = ["JumpReLU"]


class JumpReLU(torch.nn.Module):
    def __init__(self, model, cap: Optional[int] = None, bandwidth: float = 1e-3, init_threshold: Optional[float] = None) -> None:
        super().__init__()
        if not isinstance(model, TopKCore):
            raise TypeError(f"JumpReLU: expected one of the two top-k models (BinarySAE, BaselineSparseAutoencoder), got "
                            f"{type(model).__name__}: the sparsity of the other classes is not a k")
        H = int(model.encoder.linear.weight.shape[0])
        limit = min(ops.JUMP_MAX_K, H)
        cap = limit if cap is None else int(cap)
        if not 1 <= cap <= limit:
            raise ValueError(f"JumpReLU: cap = {cap}; expected 1 .. {limit} list places per row (the kernels' limit of "
                             f"{ops.JUMP_MAX_K} and hidden_dim = {H})")
        bandwidth = float(bandwidth)
        if not (bandwidth > 0.0 and math.isfinite(bandwidth)):
            raise ValueError(f"JumpReLU: bandwidth = {bandwidth}; expected a positive finite width")
        init_threshold = 1e-3 if init_threshold is None else float(init_threshold)       # the paper's initial threshold
        if not (init_threshold > 0.0 and math.isfinite(init_threshold)):
            raise ValueError(f"JumpReLU: init_threshold = {init_threshold}; expected a positive finite threshold")
        object.__setattr__(self, "model", model)               # not a submodule: the model's state dict stays its own
        self.cap, self.bandwidth = cap, bandwidth
        device = model.encoder.linear.weight.device
        self.log_threshold = torch.nn.Parameter(torch.full((H,), math.log(init_threshold), dtype=torch.float32, device=device))
        #: counts int32 [B] and report int64 [6] (selected, band entries, saturated rows, empty rows, uncertified rows, bits of the
        #: smallest threshold) of the last selection, on the device
        self.counts: Optional[torch.Tensor] = None
        self.report: Optional[torch.Tensor] = None
        #: the names of the report's words: REPORT_NAMES after a capped selection, REPORT_NAMES_DENSE after a dense one
        self.report_names = self.REPORT_NAMES

    #: what the six words of ``report`` count, on the capped path (csrc/jumprelu.hip) and on the dense one (csrc/jump_dense.hip)
    REPORT_NAMES = ("selected", "band_entries", "saturated_rows", "empty_rows", "uncertified_rows", "theta_min")
    REPORT_NAMES_DENSE = ("selected", "band_entries", "truncated_rows", "empty_rows", "band_truncated_rows", "firing")

    def record(self, counts: torch.Tensor, report: torch.Tensor, dense: bool = False) -> None:
        self.counts, self.report = counts, report
        self.report_names = self.REPORT_NAMES_DENSE if dense else self.REPORT_NAMES

    def thresholds(self) -> torch.Tensor:
        """theta = exp(log_threshold), fp32 [H] on the device, without a ``grad_fn``"""
        return self.log_threshold.detach().exp()

    def summary(self) -> dict:
        """The last selection's report as numbers (one host copy of six words)."""
        if self.report is None:
            raise ValueError("JumpReLU: no selection has run yet")
        rep = self.report.tolist()
        rows = int(self.counts.shape[0])
        if self.report_names is self.REPORT_NAMES_DENSE:       # the dense encoder: l0 from the uncapped count of firing units
            out = dict(zip(self.report_names, rep))
            out["l0"] = rep[5] / rows if rows else 0.0
            return out
        return {"selected": rep[0], "band_entries": rep[1], "saturated_rows": rep[2], "empty_rows": rep[3],
                "uncertified_rows": rep[4], "theta_min": struct.unpack("<f", struct.pack("<I", rep[5] & 0xFFFFFFFF))[0],
                "l0": rep[0] / rows if rows else 0.0}

    # -- thresholds from a BatchTopK selection ---------------------------------------------------------------------------------
    def _set_where_positive(self, value: torch.Tensor) -> None:
        """log_threshold <- log(value) everywhere when the one-element ``value`` is > 0 (false for NaN), else unchanged"""
        with torch.no_grad():
            value = value.reshape(1).to(self.log_threshold.device, torch.float32)
            self.log_threshold.copy_(torch.where(value > 0, value.log(), self.log_threshold))

    def calibrate(self, x, k: int) -> None:
        """Set every threshold to the smallest value BatchTopK would select at ``k`` per row on the batch ``x`` (from the top-
        ``cap`` lists, as ``forward_batch_topk`` selects).  On the device throughout; the thresholds stay as they are when
        that value is not > 0."""
        model = self.model
        k = int(k)
        if not 1 <= k <= self.cap:
            raise ValueError(f"JumpReLU.calibrate: k = {k}; expected 1 .. cap = {self.cap}")
        x = require_device_input(x, "x")
        H, D = model.encoder.linear.weight.shape
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"x is {tuple(x.shape)}, expected [batch, {D}]")
        with torch.no_grad():
            xf = as_f32c(x)
            _, val = model._select_cap(xf, self.cap, "JumpReLU.calibrate")
            _, _, report = ops.batch_select(val, xf.shape[0] * k, want_val=False)
            smallest = report[3:4].view(torch.float32)[0:1]    # the low 32 bits of the word, as the float they are
            smallest = torch.where(report[0:1] > 0, smallest, torch.zeros_like(smallest))
        self._set_where_positive(smallest)

    def load_from(self, batch_topk_ctl) -> None:
        """Set every threshold to the global inference threshold a ``BatchTopK`` controller has learned (``ctl.theta``; unchanged
        when that is not > 0).  On the device throughout."""
        if not hasattr(batch_topk_ctl, "theta"):
            raise TypeError(f"JumpReLU.load_from: expected a BatchTopK controller, got {type(batch_topk_ctl).__name__}")
        self._set_where_positive(batch_topk_ctl.theta.detach())

    # -- the state dict: the module's own, plus cap and bandwidth, which a loaded state must match ---------------------------
    def get_extra_state(self):
        return {"cap": self.cap, "bandwidth": self.bandwidth}

    def set_extra_state(self, state) -> None:
        if int(state["cap"]) != self.cap or float(state["bandwidth"]) != self.bandwidth:
            raise ValueError(f"JumpReLU: the state was saved with cap = {int(state['cap'])}, bandwidth = {float(state['bandwidth'])}; "
                             f"this controller has cap = {self.cap}, bandwidth = {self.bandwidth}")
