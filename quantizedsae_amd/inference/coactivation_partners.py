"""Co-activation partner sets: which features ever fired together, as one bit per pair on the device.

Reference: scripts/analysis/summarize_stats.py:37-70 -- ``average_coactivating_features`` reads ``coactivation > 0``
and nothing else of the [H, H] int32 matrix.  That bit is OR-accumulated here over the batches of a dataset
(``qsae_coactivation_partners_*``, csrc/coactivation_partners.hip) from the compact ``(idx, val)`` of the top-k models
or the packed bits of the threshold models: 128 MiB of state at H = 32768 instead of 4 GiB, and no copy of it to the
host -- ``counts()`` is all the summary needs.  Two states of the same model merge with a bitwise OR of ``bits``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import torch_ops as T

__all__ = ["CoactivationPartners"]


class CoactivationPartners:
    """Accumulates the partner sets of H features on ``device``.

    ``add_compact`` / ``add_bits`` take one batch each.  The first call fixes the number of packed positions P and the
    packed-position -> unit map; a later call with another P or another map raises ValueError.  ``bits`` is the raw
    state, int32 [P, P / 32]: bit q & 31 of word q >> 5 of row p = positions p and q were active in the same row at least
    once (the diagonal: p was active at all); ``index`` is the map (int32 [P], -1 = no unit) or None for the identity.
    Both are None before the first batch."""

    def __init__(self, H: int, device) -> None:
        if int(H) <= 0:
            raise ValueError("H must be positive")
        self.H = int(H)
        self.device = torch.device(device)
        self.bits: Optional[torch.Tensor] = None
        self.index: Optional[torch.Tensor] = None

    def _state(self, P: int, index: Optional[torch.Tensor]) -> torch.Tensor:
        if self.bits is None:
            if index is None and P != (self.H + 31) // 32 * 32:
                raise ValueError(f"{P} packed positions without a map do not stand for {self.H} units")
            self.bits = torch.zeros((P, P // 32), dtype=torch.int32, device=self.device)
            self.index = None if index is None else index.to(device=self.device, dtype=torch.int32).contiguous()
            return self.bits
        if P != self.bits.shape[0]:
            raise ValueError(f"expected {self.bits.shape[0]} packed positions as in the first batch, got {P}")
        same = (index is None) == (self.index is None) and (
            index is None or index is self.index or (index.numel() == P and torch.equal(index.to(self.index), self.index)))
        if not same:
            raise ValueError("the packed-position -> unit map differs from the first batch's")
        return self.bits

    def add_compact(self, idx: torch.Tensor, val: Optional[torch.Tensor]) -> None:
        """One batch of a top-k model: ``idx`` int32 [B, k], ``val`` fp32 [B, k] (active = val > 0) or None."""
        T.coactivation_partners_sparse(idx, val, self.H, self._state((self.H + 31) // 32 * 32, None))

    def add_bits(self, zbits: torch.Tensor, index: Optional[torch.Tensor]) -> None:
        """One batch of a threshold model: ``zbits`` int32 [B, words] and the packed-position -> unit map ``index`` (None =
        identity), the pair that goes to ``coactivation_bits``."""
        if index is not None and index.numel() != 32 * zbits.shape[1]:
            raise ValueError(f"index: expected {32 * zbits.shape[1]} entries, got {index.numel()}")
        bits = self._state(32 * zbits.shape[1], index)
        T.coactivation_partners_bits(zbits, self.index, bits)

    def counts(self) -> torch.Tensor:
        """int64 [H] on the device, in unit order: the number of other features each feature ever fired with."""
        if self.bits is None:
            return torch.zeros((self.H,), dtype=torch.int64, device=self.device)
        return T.coactivation_partner_counts(self.bits, self.H, self.index)

    def to_dense(self) -> torch.Tensor:
        """bool [H, H] in unit order, diagonal included (``coactivation > 0``).  Unpacks the state and applies the map
        with torch ops: H^2 bytes and more in flight, for small H and for tests."""
        H = self.H
        out = torch.zeros((H, H), dtype=torch.bool, device=self.device)
        if self.bits is None:
            return out
        P = self.bits.shape[0]
        shifts = torch.arange(32, device=self.device, dtype=torch.int32)
        full = ((self.bits.unsqueeze(-1) >> shifts) & 1).to(torch.bool).reshape(P, P)
        if self.index is None:
            return full[:H, :H].clone()
        index = self.index.long()
        pos = ((index >= 0) & (index < H)).nonzero(as_tuple=True)[0]
        unit = index[pos]
        out[unit.unsqueeze(1), unit.unsqueeze(0)] = full[pos.unsqueeze(1), pos.unsqueeze(0)]
        return out
