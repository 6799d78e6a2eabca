"""Batch supply of the epoch loop: the reference's ``DataLoader(dataset, batch_size, shuffle=True, num_workers=0)`` over a
``HiddenStatesTorchDataset`` (training/trainer.py:73-86), with the chunk resident on the device.

The order of the rows is the DataLoader's (``epoch_permutation``); the batches are gathered and widened by one HIP kernel
(``qsae_gather_rows``) instead of ``batch_size`` ``__getitem__`` calls and a collate on the host; which batches the
reference's ``if torch.isnan(batch).any(): continue`` would skip is known before the epoch starts, from a bitmap of the
chunk's NaN rows built once (``qsae_rows_nan_bitmap``) and the permutation (``plan_epoch``, host arithmetic): no host read
happens per step.
"""
from __future__ import annotations

import os
from typing import Iterator, List, NamedTuple, Tuple

import numpy as np
import torch

from .. import torch_ops as ops

__all__ = ["epoch_permutation", "plan_epoch", "EpochPlan", "ShuffledChunk"]

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def epoch_permutation(n: int) -> torch.Tensor:
    """The order in which ``DataLoader(dataset, shuffle=True, num_workers=0)`` yields the ``n`` samples of one epoch under
    the current state of torch's default RNG (host only; int64 [n]).

    The loader's iterator draws one int64 from the default generator as its base seed (used by worker processes only);
    its ``RandomSampler`` then draws a second one, seeds a generator of its own with it and takes ``torch.randperm(n)``
    from that.  The default RNG is left where one epoch of the loader leaves it."""
    n = int(n)
    if n < 0:
        raise ValueError(f"epoch_permutation: n = {n}")
    torch.empty((), dtype=torch.int64).random_()                  # the loader's base seed: drawn and not used
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


class EpochPlan(NamedTuple):
    """``batches``: (batch_idx, start, stop) of every batch that is trained on, ``perm[start:stop]`` being its rows and
    batch_idx counting from 1 over ALL batches, as the reference's loop does; ``skipped``: the batch_idx of the others."""
    batches: List[Tuple[int, int, int]]
    skipped: List[int]


def plan_epoch(perm, nan_bits, batch_size: int) -> EpochPlan:
    """Which batches of an epoch hold a NaN row: ``perm`` int64 [n] (the epoch's order), ``nan_bits`` the words of
    ``rows_nan_bitmap`` (bit r % 32 of word r // 32: row r holds a NaN).  Pure host arithmetic.  The last batch may be
    short."""
    perm = np.asarray(perm, dtype=np.int64).reshape(-1)
    n, batch_size = perm.size, int(batch_size)
    if batch_size < 1:
        raise ValueError(f"plan_epoch: batch_size = {batch_size}")
    words = np.ascontiguousarray(np.asarray(nan_bits)).view(np.uint32).reshape(-1)
    if words.size * 32 < n or (n and (perm.min() < 0 or perm.max() >= n)):
        raise ValueError(f"plan_epoch: {words.size} bitmap words / an order outside [0, {n}) for {n} rows")
    bad = ((words[perm >> 5] >> (perm & 31).astype(np.uint32)) & 1).astype(bool)
    batches, skipped = [], []
    for i, start in enumerate(range(0, n, batch_size), 1):
        stop = min(start + batch_size, n)
        if bad[start:stop].any():
            skipped.append(i)
        else:
            batches.append((i, start, stop))
    return EpochPlan(batches, skipped)


def _chunk_tensor(source) -> torch.Tensor:
    if isinstance(source, (str, os.PathLike)):
        from ..data import _load_chunk
        return _load_chunk(source)
    data = getattr(source, "data", source)                       # a HiddenStatesTorchDataset, or the tensor itself
    if not isinstance(data, torch.Tensor) or data.dim() not in (2, 3):
        raise TypeError("ShuffledChunk takes a chunk file, a HiddenStatesTorchDataset or a tensor [contexts, tokens, D] / "
                        f"[rows, D], got {type(source).__name__}")
    return data


class ShuffledChunk:
    """One chunk of hidden states resident on the device in its stored dtype (fp32, fp16 or bf16), handed out in the
    DataLoader's shuffled batches.

    ``ValueError`` (with the byte counts) when the chunk does not fit in the device's free memory; chunks that stay on the
    host are out of scope.  One host read happens here (the NaN bitmap, a bit per row) and none in ``epoch()``."""

    def __init__(self, dataset_or_path, batch_size: int, device=None):
        data = _chunk_tensor(dataset_or_path)
        if data.dtype not in _DTYPES:
            raise TypeError(f"ShuffledChunk: the chunk is {data.dtype}; fp32, fp16 and bf16 are stored as they are")
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"ShuffledChunk: batch_size = {batch_size}")
        if device is None and data.is_cuda:
            device = data.device
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError(f"ShuffledChunk: quantizedsae_amd runs on MI355X only; device is {dev} (no CPU fallback exists)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.feature_dim = data.shape[-1]
        self.n_rows = data.numel() // max(self.feature_dim, 1)
        if self.feature_dim < 1:
            raise ValueError(f"ShuffledChunk: the chunk is {tuple(data.shape)}")
        if not data.is_cuda:
            need = data.numel() * data.element_size()
            free, _total = torch.cuda.mem_get_info(dev)
            if need > free:
                raise ValueError(f"ShuffledChunk: the chunk takes {need} bytes and {dev} has {free} bytes free; "
                                 "host-resident chunks are not supported")
        self.data = data.to(dev).contiguous().reshape(self.n_rows, self.feature_dim)
        self.nan_bits = ops.rows_nan_bitmap(self.data).cpu().numpy() if self.n_rows else np.zeros((0,), np.int32)
        self._flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._perm_host = None
        self.last_plan = None

    def __len__(self) -> int:
        return self.n_rows

    @property
    def nan_rows(self) -> int:
        return int(sum(bin(int(w)).count("1") for w in self.nan_bits.view(np.uint32)))

    def epoch(self) -> Iterator[Tuple[int, torch.Tensor]]:
        """Yields ``(batch_idx, batch fp32 [rows, D])`` for one epoch in the DataLoader's order under the current default
        RNG.  Batches holding a NaN row are not produced; batch_idx counts them, as in the reference.  The permutation is
        uploaded once; the plan of the epoch is left in ``last_plan``."""
        perm = epoch_permutation(self.n_rows)
        plan = self.last_plan = plan_epoch(perm.numpy(), self.nan_bits, self.batch_size)
        self._perm_host = perm.pin_memory()                       # kept alive while the copy is in flight
        perm_dev = self._perm_host.to(self.device, non_blocking=True)
        for batch_idx, start, stop in plan.batches:
            yield batch_idx, ops.gather_rows(self.data, perm_dev[start:stop], self._flag)

    def check(self) -> None:
        """One host read: raises if any gather since the last check met an index outside the chunk."""
        if int(self._flag.item()) != 0:
            self._flag.zero_()
            raise RuntimeError("ShuffledChunk: a batch index was outside the chunk (its rows were filled with zeros)")
