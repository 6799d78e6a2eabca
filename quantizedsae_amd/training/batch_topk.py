"""BatchTopK for the two top-k models (Bussmann et al., "BatchTopK Sparse Autoencoders"; the selection their Matryoshka SAEs
train with): keep the ``B * k`` largest pre-activations of the whole batch instead of k per row, so a row spends as many units
as it needs, and at inference one global threshold learned during training.

    ctl = BatchTopK(model, k=65)                              cap = min(256, hidden_dim, 4 k) list places per row
    outputs = model.forward_train_batch_topk(batch, ctl)      the tuple of forward_train; moves ctl's threshold
    idx, val, counts, recon = model.forward_threshold(x, ctl) evaluation: every entry at or above the threshold
    outputs = model.forward_train_nested_batch_topk(batch, ctl, bounds)    the same selection, one reconstruction per
                                                              dictionary prefix (the tuple of forward_train_nested)

Every row's top-``cap`` list is rank ordered, so the batch-wide selection (ties to the lowest row, then list position) is a
prefix of every row's list: the whole result is one count per row, and the decode and the backward walk ``counts[r]`` entries
of row r (csrc/batch_topk.hip, csrc/batch_topk_decode.hip).  The selection is BatchTopK capped at ``cap`` per row; it equals
the uncapped one whenever no row is saturated (``report[1] == 0``), because a unit outside a row's top-``cap`` can beat the
threshold only if the row's ``cap``-th entry does too.

The threshold state -- ``theta`` (fp32) and ``batches`` (int64) -- lives on the device and is moved by the selection's own
kernel chain: with m the smallest selected value of a batch, ``theta <- m`` on the first update and
``theta <- theta + lr * (m - theta)`` afterwards, when m > 0.  Nothing is read back unless ``threshold()`` or ``summary()`` is
called.  The models' state-dict keys stay the reference's; the controller has a ``state_dict()`` of its own.

``BatchTopK(model, dense=True)`` selects through the dense encoder (csrc/batch_dense.hip): the
``forward*_batch_topk_dense`` methods of the models collect the pre-activations above a *floor* in the encoder's contraction and
select among those.  The floor -- one fp32 word on the device, ``floor_ratio`` times the last batch's smallest selected value,
written by the kernel chain -- changes the time, never the result: a batch with too few candidates above it is selected again
without a floor, on the device.  A controller whose floor was never seeded runs one capped step and seeds it from that step's
report.  The default (``dense=False``) is the capped path and nothing above changes.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import torch_ops as ops
from ..sae.topk import TopKCore

__all__ = ["BatchTopK"]


class BatchTopK:
    #: the floor of a dense controller as a fraction of the last batch's smallest selected value, unless the caller says otherwise:
    #: the largest of the ratios tried at which no batch of the measured run needed the second attempt (DESIGN.md section 4.38,
    #: profiles/batch_dense.txt)
    DEFAULT_FLOOR_RATIO = 0.97
    #: what the eight words of the dense encoder's report count (``report_dense``); the first four are ``report``
    REPORT_NAMES_DENSE = ("selected", "saturated_rows", "empty_rows", "min_selected_bits", "candidates", "second_attempt",
                          "rows_over_cap", "floor_bits")

    def __init__(self, model, k: Optional[int] = None, cap: Optional[int] = None, threshold_lr: float = 0.01, dense: bool = False,
                 floor_ratio: Optional[float] = None) -> None:
        if not isinstance(model, TopKCore):
            raise TypeError(f"BatchTopK: expected one of the two top-k models (BinarySAE, BaselineSparseAutoencoder), got "
                            f"{type(model).__name__}: the sparsity of the other classes is not a k")
        H = int(model.encoder.linear.weight.shape[0])
        if k is None:
            k = model.top_k if hasattr(model, "top_k") else model.topk
        k, limit = int(k), min(ops.BATCH_TOPK_MAX_K, H)
        if not 1 <= k <= limit:
            raise ValueError(f"BatchTopK: k = {k}; expected 1 .. {limit} (the kernels' limit of {ops.BATCH_TOPK_MAX_K} and "
                             f"hidden_dim = {H})")
        cap = min(limit, 4 * k) if cap is None else int(cap)
        if not k <= cap <= limit:
            raise ValueError(f"BatchTopK: cap = {cap}; expected k = {k} .. {limit} list places per row")
        threshold_lr = float(threshold_lr)
        if not 0.0 <= threshold_lr <= 1.0:
            raise ValueError(f"BatchTopK: threshold_lr = {threshold_lr}; expected a rate in [0, 1]")
        if floor_ratio is not None and not dense:
            raise ValueError("BatchTopK: floor_ratio needs dense=True")
        floor_ratio = self.DEFAULT_FLOOR_RATIO if floor_ratio is None else float(floor_ratio)
        if not 0.0 < floor_ratio <= 1.0:
            raise ValueError(f"BatchTopK: floor_ratio = {floor_ratio}; expected a ratio in (0, 1]")
        self.model, self.k, self.cap, self.threshold_lr = model, k, cap, threshold_lr
        self.dense, self.floor_ratio = bool(dense), floor_ratio
        device = model.encoder.linear.weight.device
        #: the floor of the dense selection, on the device; NaN until a step has seeded it (a NaN floor admits no candidate)
        self.floor = torch.full((), float("nan"), dtype=torch.float32, device=device)
        self.floor_seeded = False
        #: the dense encoder's report int64 [8] of the last dense selection, the number of dense selections and how many of
        #: them needed the second attempt (int64, counted on the device)
        self.report_dense: Optional[torch.Tensor] = None
        self.dense_selections = 0
        self.second_attempts = torch.zeros((), dtype=torch.int64, device=device)
        #: the inference threshold and the number of batches that have moved it, on the device
        self.theta = torch.zeros((), dtype=torch.float32, device=device)
        self.batches = torch.zeros((), dtype=torch.int64, device=device)
        #: counts int32 [B] and report int64 [4] (selected, saturated rows, empty rows, bits of the smallest selected value) of
        #: the last selection, on the device
        self.counts: Optional[torch.Tensor] = None
        self.report: Optional[torch.Tensor] = None
        #: int32 [L, B]: every row's selected entries below each bound, left by the last nested selection
        #: (forward_nested_batch_topk, forward_nested_threshold, forward_train_nested_batch_topk), on the device
        self.level_counts: Optional[torch.Tensor] = None

    def state(self, device):
        """-> (theta, batches) on ``device`` (moved there once, when the model has moved since)"""
        if self.theta.device != device:
            self.theta, self.batches = self.theta.to(device), self.batches.to(device)
        return self.theta, self.batches

    def record(self, counts: torch.Tensor, report: torch.Tensor) -> None:
        """``report``: the four words of ``batch_select``, or the eight of ``encode_batch_topk`` (whose first four they are)"""
        if report.numel() == len(self.REPORT_NAMES_DENSE):
            self.report_dense, report = report, report[:4]
            self.dense_selections += 1
            if self.second_attempts.device != report.device:
                self.second_attempts = self.second_attempts.to(report.device)
            self.second_attempts += self.report_dense[5]
        self.counts, self.report = counts, report

    def floor_state(self, device) -> torch.Tensor:
        """-> the floor word on ``device`` (moved there once, when the model has moved since)"""
        if self.floor.device != device:
            self.floor = self.floor.to(device)
        return self.floor

    def seed_floor(self, report: torch.Tensor) -> None:
        """The floor from the report of a capped selection, on the device: fl32(floor_ratio * m) when something was selected
        and the smallest selected value m is > 0 -- what the dense chain writes at its own end.  No host read."""
        floor = self.floor_state(report.device)
        m = report[3:4].to(torch.int32).view(torch.float32).reshape(())
        ratio = torch.tensor(self.floor_ratio, dtype=torch.float32, device=report.device)
        floor.copy_(torch.where((report[0] > 0) & (m > 0), ratio * m, floor))
        self.floor_seeded = True

    def dense_summary(self) -> dict:
        """The last dense selection's extra report words as numbers (one host copy)."""
        if self.report_dense is None:
            raise ValueError("BatchTopK: no dense selection has run yet")
        words = torch.cat([self.report_dense, self.second_attempts.reshape(1)]).tolist()
        rows = int(self.counts.shape[0])
        return {"candidates": int(words[4]), "candidates_per_row": int(words[4]) / max(rows, 1), "second_attempt": int(words[5]),
                "rows_over_cap": int(words[6]), "second_attempts": int(words[8]), "dense_selections": self.dense_selections}

    def threshold(self) -> float:
        """The learned threshold (one host read)."""
        return float(self.theta)

    def summary(self) -> dict:
        """The last selection's report and the threshold as numbers (one host copy of five words)."""
        if self.report is None:
            raise ValueError("BatchTopK: no selection has run yet")
        both = torch.cat([self.report.to(torch.float64), self.theta.reshape(1).to(torch.float64)]).tolist()
        return {"selected": int(both[0]), "saturated_rows": int(both[1]), "empty_rows": int(both[2]), "threshold": both[4]}

    def state_dict(self) -> dict:
        state = {"theta": self.theta.detach().cpu().clone(), "batches": self.batches.detach().cpu().clone(), "k": self.k,
                 "cap": self.cap, "threshold_lr": self.threshold_lr}
        if self.dense:
            state["dense_floor"] = {"floor": self.floor.detach().cpu().clone(), "seeded": self.floor_seeded,
                                    "floor_ratio": self.floor_ratio}
        return state

    def load_state_dict(self, state: dict) -> None:
        if int(state["k"]) != self.k or int(state["cap"]) != self.cap:
            raise ValueError(f"BatchTopK: the state was saved with k = {int(state['k'])}, cap = {int(state['cap'])}; this "
                             f"controller has k = {self.k}, cap = {self.cap}")
        device = self.theta.device
        self.theta = torch.as_tensor(state["theta"], dtype=torch.float32).reshape(()).to(device).clone()
        self.batches = torch.as_tensor(state["batches"], dtype=torch.int64).reshape(()).to(device).clone()
        self.threshold_lr = float(state["threshold_lr"])
        saved = state.get("dense_floor")                      # absent in states saved by a capped controller: the floor is
        if saved is not None and self.dense:                   # then seeded again by the first step
            self.floor = torch.as_tensor(saved["floor"], dtype=torch.float32).reshape(()).to(device).clone()
            self.floor_seeded = bool(saved["seeded"])
