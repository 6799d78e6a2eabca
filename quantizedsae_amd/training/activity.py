"""Whether the dictionary is alive while it trains: per-unit firing counts and a "last fired" clock kept on the device
(csrc/activity.hip).  The reference's ``one_epoch`` takes a ``dead_neuron_threshold`` that nothing reads
and a ``latents`` list it never fills (training/trainer.py:66-78), and logs ``activated_neurons`` for ``b_sae`` alone.

A ``FeatureActivity`` is fed by ``forward_train`` from what it already holds -- ``(idx, val)`` of the top-k models, the packed
z bits of the threshold models, the dense latent of the ternary model -- once ``model.activity`` is set; ``summary(window)``
is one kernel call and one host copy of a few dozen integers.  "Active" is the reference's activation mask
(scripts/analysis/dynamic_analysis.py:30-73), the convention of ``inference/analysis.py``.

The clock ``rows_seen`` is a host integer, the rows added so far; a batch of B rows is stamped ``rows_seen + B``.  With a
window of W rows a unit is dead when ``rows_seen - last >= W`` (one that never fired once ``rows_seen >= W``), ``never`` fired
while ``last == 0``, and silent when it has not fired since the previous summary.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from .. import torch_ops as ops

__all__ = ["FeatureActivity", "ActivitySummary", "activity_line", "ACTIVITY_BINS"]

_HEAD = 8
ACTIVITY_BINS = 34
_MAX_SEGMENTS = 16


@dataclass
class ActivitySummary:
    """One block of a summary: all units, or one level.  ``octaves[0]`` counts the units with no firing in the interval,
    ``octaves[b]`` those with ``2^(b-1) <= count < 2^b`` (33 and above in the last bin).  ``interval_count`` is the sum of the
    interval's firing counts and ``mean_l0 = interval_count / interval_rows`` the active units per row over the interval (0.0
    for an empty one).  ``dead_indices``: the dead units in ascending order, an int32 tensor on the device, or None."""
    units: int
    never: int
    dead: int
    silent: int
    interval_rows: int
    interval_count: int
    total_count: int
    max_count: int
    mean_l0: float
    octaves: List[int]
    levels: List["ActivitySummary"] = field(default_factory=list)
    dead_indices: Optional[torch.Tensor] = None

    @property
    def dead_fraction(self) -> float:
        return self.dead / self.units if self.units else 0.0


def _parse(block: torch.Tensor, interval_rows: int) -> List[ActivitySummary]:
    """block: the int64 [1 + n_seg, 8 + 34] result of ops.activity_summary on the host"""
    out = []
    for row in block.tolist():
        units, never, dead, silent, interval, total, largest = row[:7]
        out.append(ActivitySummary(units, never, dead, silent, interval_rows, interval, total, largest,
                                   interval / interval_rows if interval_rows > 0 else 0.0, row[_HEAD:]))
    return out


class _ActivityView:
    """``fired`` / ``last`` of a run of units and the clock they are stamped by.  ``add_*`` of a segment never advance it."""

    def __init__(self, root: "FeatureActivity", fired: torch.Tensor, last: torch.Tensor):
        self._root, self.fired, self.last = root, fired, last

    @property
    def H(self) -> int:
        return int(self.fired.numel())

    def _done(self, rows: int, advance: bool) -> None:
        pass                                                   # a segment: the owner of the clock advances it

    def add_compact(self, idx: torch.Tensor, val: Optional[torch.Tensor], *, advance: bool = True) -> None:
        """(idx int32 [B, k], val fp32 [B, k] or None) of a top-k forward: entry active iff val > 0"""
        B = int(idx.shape[0])
        if B and idx.shape[1]:
            ops.activity_add_compact(idx, val, self._root.rows_seen + B, self.fired, self.last)
        self._done(B, advance)

    def add_bits(self, zbits: torch.Tensor, index: Optional[torch.Tensor] = None, *, advance: bool = True) -> None:
        """zbits int32 [B, words] packed bits; ``index`` maps a packed position to its unit (-1 = pad), None = identity"""
        B = int(zbits.shape[0])
        if B:
            ops.activity_add_bits(zbits, index, self._root.rows_seen + B, self.fired, self.last)
        self._done(B, advance)

    def add_dense(self, latent: torch.Tensor, *, advance: bool = True) -> None:
        """latent fp32 [B, H]: active iff latent > 0"""
        B = int(latent.shape[0])
        if B:
            ops.activity_add_dense(latent, self._root.rows_seen + B, self.fired, self.last)
        self._done(B, advance)


class FeatureActivity(_ActivityView):
    """``FeatureActivity(H, device, level_sizes=None)``: the state of H units on ``device`` (three int64 [H] arrays) and the
    host clock ``rows_seen``.  ``level_sizes``: consecutive slices of the units that ``summary`` also reports one by one (the
    matryoshka levels, the residual stages; at most 16, adding up to H)."""

    def __init__(self, H: int, device, level_sizes: Optional[Sequence[int]] = None):
        H = int(H)
        if H < 1:
            raise ValueError(f"FeatureActivity: H must be >= 1, got {H}")
        sizes = [int(s) for s in level_sizes] if level_sizes is not None else []
        if sizes and (len(sizes) > _MAX_SEGMENTS or min(sizes) < 0 or sum(sizes) != H):
            raise ValueError(f"FeatureActivity: level_sizes must be at most {_MAX_SEGMENTS} sizes >= 0 that add up to H = {H}, "
                             f"got {sizes}")
        self.device = torch.device(device)
        self.level_sizes = sizes
        fired, last, self.base = (torch.zeros((H,), dtype=torch.int64, device=self.device) for _ in range(3))
        super().__init__(self, fired, last)
        self.rows_seen = 0
        self._summary_rows = 0                                 # rows_seen at the previous advancing summary
        self._dead_out = None

    @classmethod
    def for_model(cls, model: torch.nn.Module) -> "FeatureActivity":
        """The tracker of a model: the levels of ``decoder.nested_dictionary_size`` for a QuantizedMatryoshkaSAE, the stages
        ``sae_hidden_dims`` side by side for a ResidualQuantizedSAE (H = their sum), no levels otherwise."""
        from ..sae import QuantizedMatryoshkaSAE, ResidualQuantizedSAE
        if isinstance(model, ResidualQuantizedSAE):
            sizes = [int(h) for h in model.sae_hidden_dims]
            return cls(sum(sizes), model.saes[0].encoder.linear.weight.device, sizes)
        weight = model.encoder.linear.weight
        if isinstance(model, QuantizedMatryoshkaSAE):
            return cls(weight.shape[0], weight.device, [int(s) for s in model.decoder.nested_dictionary_size])
        return cls(weight.shape[0], weight.device)

    def _done(self, rows: int, advance: bool) -> None:
        if advance:
            self.advance(rows)

    def advance(self, rows: int) -> None:
        """The clock moves on by ``rows`` rows"""
        rows = int(rows)
        if rows < 0:
            raise ValueError(f"FeatureActivity.advance: rows = {rows}")
        self.rows_seen += rows

    def segment(self, offset: int, size: int) -> _ActivityView:
        """A view on the units [offset, offset + size) of the same state, stamped by the same clock, whose ``add_*`` never
        advance it: the stages of a residual model feed one each and the model advances once per batch."""
        offset, size = int(offset), int(size)
        if offset < 0 or size < 1 or offset + size > self.H:
            raise ValueError(f"FeatureActivity.segment: [{offset}, {offset + size}) is not inside [0, {self.H})")
        return _ActivityView(self, self.fired[offset:offset + size], self.last[offset:offset + size])

    def summary(self, window: int, *, dead_list: bool = False, advance: bool = True) -> ActivitySummary:
        """One kernel call and one host copy of its result.  ``advance``: this summary ends the interval (base = fired).
        ``dead_list``: ``dead_indices`` holds the dead units in ascending order, on the device."""
        window = int(window)
        if window < 1:
            raise ValueError(f"FeatureActivity.summary: window must be >= 1 row, got {window}")
        dead_out = None
        if dead_list:
            if self._dead_out is None:
                self._dead_out = torch.empty((self.H,), dtype=torch.int32, device=self.device)
            dead_out = self._dead_out
        result = ops.activity_summary(self.fired, self.base, self.last, self.rows_seen, window, self.level_sizes, advance, dead_out)
        blocks = _parse(result.cpu(), self.rows_seen - self._summary_rows)
        out = blocks[0]
        out.levels = blocks[1:]
        if dead_list:
            out.dead_indices = dead_out[:out.dead].clone()
        if advance:
            self._summary_rows = self.rows_seen
        return out

    def state_dict(self) -> dict:
        return {"fired": self.fired.detach().cpu().clone(), "last": self.last.detach().cpu().clone(),
                "base": self.base.detach().cpu().clone(), "rows_seen": self.rows_seen, "summary_rows": self._summary_rows,
                "level_sizes": list(self.level_sizes)}

    def load_state_dict(self, state: dict) -> None:
        for name in ("fired", "last", "base"):
            t = torch.as_tensor(state[name])
            if t.dtype != torch.int64 or tuple(t.shape) != (self.H,):
                raise ValueError(f"FeatureActivity.load_state_dict: {name} must be int64 [{self.H}], got {t.dtype} {tuple(t.shape)}")
        if list(state.get("level_sizes", self.level_sizes)) != list(self.level_sizes):
            raise ValueError(f"FeatureActivity.load_state_dict: level_sizes {state['level_sizes']} != {self.level_sizes}")
        rows, summary_rows = int(state["rows_seen"]), int(state["summary_rows"])
        if not 0 <= summary_rows <= rows:
            raise ValueError(f"FeatureActivity.load_state_dict: rows_seen = {rows}, summary_rows = {summary_rows}")
        for name in ("fired", "last", "base"):
            getattr(self, name).copy_(torch.as_tensor(state[name]))
        self.rows_seen, self._summary_rows = rows, summary_rows


def activity_line(s: ActivitySummary) -> str:
    """One printed line of a summary: dead, never fired, silent, the mean L0 of the interval and the octave bins up to the last
    non-empty one; the dead units per level where there are levels"""
    top = max((b for b, n in enumerate(s.octaves) if n), default=0)
    line = (f"  activity: dead={s.dead}/{s.units} ({100.0 * s.dead_fraction:.2f}%), never_fired={s.never}, silent={s.silent}, "
            f"mean_l0={s.mean_l0:.4f} over {s.interval_rows} rows, count_octaves={s.octaves[:top + 1]}")
    if s.levels:
        line += ", dead_per_level=[" + ", ".join(f"{lv.dead}/{lv.units}" for lv in s.levels) + "]"
    return line
