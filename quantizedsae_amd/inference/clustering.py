"""k-means over the atoms of a dictionary on the GPU.

Reference: src/quantized_sae/utils/inspector.py:137-165 (``k_means_analysis``) hands the [H, D] dictionary to
``kmeans_pytorch.kmeans(..., device=cpu)``: Lloyd's algorithm with broadcast [N, C, D] distances.  Here an iteration is
two library calls: ``qsae_kmeans_assign_f32`` (csrc/kmeans.hip) contracts atoms and centers on the exact-fp32 matrix pipe
and keeps one key per atom, so no [N, C] matrix exists, and ``qsae_kmeans_update_f32`` forms the means in fp64 in a fixed
order.  Every step is reproducible bit for bit: the arithmetic is spelled out in DESIGN.md 4.20.

Deliberate differences from ``kmeans_pytorch``: an all-zero atom has cosine 0 with every center (there: NaN) and goes to
center 0; an empty cluster keeps its center (there: it is reseeded from a random atom); equal scores go to the lowest
center index; the random initial rows are drawn by torch's seeded generator, not numpy's global one.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from .. import torch_ops as T
from .dictionary import _decode_keys
from .inspector import _fp32_atoms, _pad4

__all__ = ["kmeans_atoms"]

DISTANCES = ("cosine", "euclidean")


def _inertia(atoms: torch.Tensor, centers: torch.Tensor, labels: torch.Tensor, score: torch.Tensor, distance: str) -> float:
    """fp64: the sum of 1 - cos (from the assign scores), or of the squared distances to the assigned centers."""
    ok = labels >= 0
    if distance == "cosine":
        return float((1.0 - score[ok].double()).sum().item())
    total = 0.0
    for r0 in range(0, atoms.shape[0], 8192):               # bounded fp64 temporaries
        rows = ok[r0:r0 + 8192]
        diff = atoms[r0:r0 + 8192][rows].double() - centers[labels[r0:r0 + 8192][rows]].double()
        total += float((diff * diff).sum().item())
    return total


def kmeans_atoms(atoms_or_sae, num_clusters: int, *, distance: str = "cosine", tol: float = 1e-4, max_iter: int = 300,
                 init: str = "random", seed: int = 0, init_indices=None, init_centers: Optional[torch.Tensor] = None,
                 check_every: int = 1) -> Dict[str, Any]:
    """Lloyd's k-means of the atoms of an SAE (or of atoms ``[N, D]``, fp32 or int8) into ``num_clusters`` clusters.

    Initial centers: ``atoms[init_indices]``, or ``init_centers`` ``[C, D]``, or (``init="random"``)
    ``atoms[torch.randperm(N, generator seeded with seed)[:C]]`` -- C distinct rows, as ``kmeans_pytorch`` draws them.
    An iteration assigns (``distance``: "cosine", or "euclidean" on the raw vectors) and updates on the device, with two
    alternating center buffers; ``center_shift`` is read on the host every ``check_every`` iterations and the loop stops
    when ``center_shift ** 2 < tol`` (``kmeans_pytorch``'s rule and default) or after ``max_iter`` iterations.  One more
    assign against the final centers gives the labels.

    Result: ``labels`` int64 [N] (-1 for an atom whose every score is NaN), ``centers`` fp32 [C, D], ``counts`` int64 [C]
    of the final labels, ``score`` fp32 [N] (the cosine, or ``a . c - |c|^2 / 2``), ``inertia`` (fp64 sum of ``1 - cos``
    or of squared distances), ``n_iter``, ``converged``, ``n_empty`` and ``center_shift`` of the last update.  ValueError:
    more clusters than atoms with index initialisation, an unknown ``distance`` or ``init``, a different D or device."""
    if distance not in DISTANCES:
        raise ValueError(f"distance must be 'cosine' or 'euclidean', got {distance!r}")
    if init != "random":
        raise ValueError(f"init must be 'random' (or pass init_indices / init_centers), got {init!r}")
    C = int(num_clusters)
    if C < 1:
        raise ValueError(f"num_clusters must be >= 1, got {num_clusters}")
    if int(max_iter) < 0 or int(check_every) < 1:
        raise ValueError("max_iter >= 0 and check_every >= 1 required")
    a = _fp32_atoms(atoms_or_sae)
    N, D = a.shape
    a = _pad4(a)                                             # a zero column changes no chain, no norm and no mean
    if init_centers is not None:
        if init_indices is not None:
            raise ValueError("pass init_indices or init_centers, not both")
        if not isinstance(init_centers, torch.Tensor) or init_centers.dim() != 2 or init_centers.shape != (C, D):
            raise ValueError(f"init_centers must be [{C}, {D}] (num_clusters, D of the atoms)")
        if init_centers.device != a.device:
            raise ValueError(f"atoms and init_centers live on different devices ({a.device} vs {init_centers.device})")
        centers = _pad4(init_centers.to(torch.float32)).clone()
    else:
        if C > N:
            raise ValueError(f"num_clusters = {C} exceeds the {N} atoms: initial centers are distinct atoms")
        if init_indices is not None:
            idx = torch.as_tensor(init_indices, dtype=torch.int64, device=a.device).reshape(-1)
            if idx.numel() != C or (C and (int(idx.min()) < 0 or int(idx.max()) >= N)):
                raise ValueError(f"init_indices must be {C} atom indices in [0, {N})")
        else:
            gen = torch.Generator(device="cpu")
            gen.manual_seed(int(seed))
            idx = torch.randperm(N, generator=gen)[:C].to(a.device)
        centers = a[idx].clone()

    n_iter, converged, shift, n_empty = 0, False, float("nan"), 0
    stats = None
    while n_iter < int(max_iter):
        labels = _decode_keys(T.kmeans_assign(a, centers, distance))[1]
        centers, _, stats = T.kmeans_update(a, labels, centers)          # a new buffer; the old one is released
        n_iter += 1
        if n_iter % int(check_every) == 0 or n_iter == int(max_iter):
            shift, n_empty = (float(v) for v in stats.tolist())          # the host reads two doubles
            if shift ** 2 < tol:
                converged = True
                break
    score, labels = _decode_keys(T.kmeans_assign(a, centers, distance))
    counts = torch.bincount(labels[labels >= 0], minlength=C)
    out_centers = centers[:, :D].contiguous()
    return {"labels": labels, "centers": out_centers, "counts": counts, "score": score,
            "inertia": _inertia(a, centers, labels, score, distance), "n_iter": n_iter, "converged": converged,
            "n_empty": int(n_empty), "center_shift": shift}
