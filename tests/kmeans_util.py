"""Shared helpers of the k-means tests: the numpy restatement of the arithmetic contract -- the assign
keys of both metrics, the chunked fp64 update with its two summation orders, Lloyd's loop with kmeans_pytorch's stopping
rule -- the post-processing of the reference's ``k_means_analysis`` (groups, center features), atom recipes from the
portable PRNG of quantizedsae_amd/synthetic.py, and the recipe of the fixture tests/golden/kmeans_inspector_ternary.npz."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

import dictionary_neighbors_util as NU
import neighbors_f32_util as FU
from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"
GOLDEN_NAME = "kmeans_inspector_ternary"
GOLDEN_N, GOLDEN_D, GOLDEN_C, GOLDEN_SEED, GOLDEN_EMPTY = 300, 64, 7, 61, 4
KMEANS_CHUNK = 64                       # kKmeansChunk of csrc/kmeans.hip: consecutive members summed by one workgroup
METRICS = {"cosine": 0, "euclidean": 1}

mono, decode_keys, chain = FU.mono, FU.decode_keys, FU.chain


# ---- the contract, restated ------------------------------------------------------------------------------------------
def nsq64(a: np.ndarray) -> np.ndarray:
    """fp64 [N]: the sum of squares in atom_inv_norms_kernel's order.  Lane l of 64 adds the fp64 squares of d = l,
    l + 64, ... in order from 0.0, then the xor butterfly m = 32, 16, ..., 1."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    N, D = a.shape
    T = (D + 63) // 64
    sq = np.zeros((N, T * 64), dtype=np.float64)
    v = a.astype(np.float64)
    sq[:, :D] = v * v
    sq = sq.reshape(N, T, 64)
    s = np.zeros((N, 64), dtype=np.float64)
    for t in range(T):
        s = s + sq[:, t, :]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ m]
    return s[:, 0]


def half_sq(c: np.ndarray) -> np.ndarray:
    """h[j] = fp32(0.5 * nsq64[j])."""
    return (0.5 * nsq64(c)).astype(np.float32)


def scores(a: np.ndarray, c: np.ndarray, metric) -> np.ndarray:
    """fp32 [N, C]: cosine acc * (inv_a * inv_c); euclidean acc - h, one separately rounded fp32 subtraction."""
    if METRICS.get(metric, metric) == 0:
        return FU.cosines(a, c)
    return chain(a, c) - half_sq(c)[None, :]


def assign_keys(a: np.ndarray, c: np.ndarray, metric) -> np.ndarray:
    """int64 [N]: the largest mono(s) << 32 | ~j over the centers; 0 where every score is NaN."""
    if METRICS.get(metric, metric) == 0:
        return FU.reference_keys(a, c, 1)[:, 0].copy()
    s = scores(a, c, 1)
    key = (mono(s).astype(np.uint64) << np.uint64(32)) | (~np.arange(c.shape[0], dtype=np.uint32)).astype(np.uint64)[None, :]
    key[np.isnan(s)] = 0
    return key.max(axis=1).view(np.int64)


def labels_of(keys: np.ndarray) -> np.ndarray:
    return decode_keys(np.ascontiguousarray(keys))[1]


def _tree256(s: np.ndarray) -> float:
    """ls[t] += ls[t + w] for w = 128, 64, ..., 1 over 256 slots."""
    s = s.copy()
    w = 128
    while w >= 1:
        s[:w] = s[:w] + s[w:2 * w]
        w >>= 1
    return float(s[0])


def cluster_shift(new_row: np.ndarray, old_row: np.ndarray) -> float:
    """sqrt(sum_d (double(new) - double(old))^2): slot t of 256 adds d = t, t + 256, ... in order, then the tree."""
    diff = new_row.astype(np.float64) - old_row.astype(np.float64)
    D = diff.size
    T = (D + 255) // 256
    sq = np.zeros((T * 256,), dtype=np.float64)
    sq[:D] = diff * diff
    return float(np.sqrt(_tree256(np.cumsum(sq.reshape(T, 256), axis=0)[-1])))


def total_shift(shifts: np.ndarray) -> float:
    """Slot t of 256 adds the contiguous run c = t per .. t per + per - 1 (per = ceil(C / 256)) in order, then the tree."""
    C = shifts.size
    per = (C + 255) // 256
    s = np.zeros((256 * per,), dtype=np.float64)
    s[:C] = shifts
    return _tree256(np.cumsum(s.reshape(256, per), axis=1)[:, -1])


def update(a: np.ndarray, labels: np.ndarray, old: np.ndarray):
    """-> (centers fp32 [C, D], counts int32 [C], stats fp64 [2] = {center_shift, n_empty}).  Members in ascending atom
    index; chunks of KMEANS_CHUNK members, each an fp64 chain from 0.0 (np.cumsum is that chain), the chunk partials
    added in chunk order from 0.0; fp32(sum / count); an empty cluster keeps its old center."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    old = np.ascontiguousarray(old, dtype=np.float32)
    C, D = old.shape
    new = old.copy()
    counts = np.zeros((C,), dtype=np.int32)
    order = np.argsort(labels, kind="stable")
    sl = np.asarray(labels)[order]
    for c in range(C):
        idx = order[np.searchsorted(sl, c, "left"):np.searchsorted(sl, c, "right")]
        counts[c] = idx.size
        if idx.size == 0:
            continue
        s = np.zeros((D,), dtype=np.float64)
        for g in range(0, idx.size, KMEANS_CHUNK):
            s = s + np.cumsum(a[idx[g:g + KMEANS_CHUNK]].astype(np.float64), axis=0)[-1]
        new[c] = (s / float(idx.size)).astype(np.float32)
    shifts = np.array([cluster_shift(new[c], old[c]) for c in range(C)], dtype=np.float64)
    return new, counts, np.array([total_shift(shifts), float((counts == 0).sum())], dtype=np.float64)


def lloyd(a: np.ndarray, init: np.ndarray, metric="cosine", tol: float = 1e-4, max_iter: int = 300) -> dict:
    """Lloyd's loop as kmeans_atoms runs it with check_every = 1: assign, update, stop when center_shift ** 2 < tol
    (kmeans_pytorch's rule) or at max_iter; then one more assign against the final centers."""
    centers = np.ascontiguousarray(init, dtype=np.float32).copy()
    history, centers_history, n_iter, converged, stats = [], [], 0, False, np.zeros(2)
    for _ in range(max_iter):
        labels = labels_of(assign_keys(a, centers, metric))
        centers, counts, stats = update(a, labels, centers)
        history.append(labels)
        centers_history.append(centers)
        n_iter += 1
        if stats[0] ** 2 < tol:
            converged = True
            break
    keys = assign_keys(a, centers, metric)
    labels = labels_of(keys)
    return {"labels": labels, "centers": centers, "counts": np.bincount(labels[labels >= 0], minlength=centers.shape[0]),
            "keys": keys, "history": history, "centers_history": centers_history, "n_iter": n_iter, "converged": converged, "center_shift": float(stats[0]),
            "n_empty": int(stats[1])}


# ---- what the reference's k_means_analysis does around the kmeans call (inspector.py:143-165) ------------------------
def groups(labels: np.ndarray, C: int):
    return [np.nonzero(labels == c)[0].tolist() for c in range(C)]


def center_features(a: np.ndarray, labels: np.ndarray, centers: np.ndarray, metric="cosine"):
    """Per cluster the member with the smallest 1 - atom . center (cosine, raw vectors) or |atom - center| (euclidean),
    in fp64; the lowest index among equals; -1 for an empty cluster."""
    a64 = np.asarray(a, dtype=np.float64)
    c64 = np.asarray(centers, dtype=np.float64)
    out = []
    for c, members in enumerate(groups(labels, centers.shape[0])):
        if not members:
            out.append(-1)
            continue
        dot = (a64[members] * c64[c][None, :]).sum(1)
        if METRICS.get(metric, metric) == 0:
            rank = dist = 1.0 - dot
        else:                                               # |a|^2 / 2 - a . c orders the members as |a - c| does
            rank = 0.5 * (a64[members] * a64[members]).sum(1) - dot
            dist = np.sqrt(np.maximum(2.0 * rank + (c64[c] * c64[c]).sum(), 0.0))
        # the reference starts its search at min_distance = 99999: a member at or beyond that is never chosen
        rank = np.where(dist < 99999.0, rank, np.inf)
        out.append(int(members[int(np.argmin(rank))]) if np.isfinite(rank.min()) else -1)
    return out


# ---- bounds against real arithmetic ----------------------------------------------------------------------------------
def euclid_f64(a: np.ndarray, c: np.ndarray):
    """(s64, bound): s64 = a . c - |c|^2 / 2 in fp64 and the derived bound on |s - s64| of the restatement (DESIGN.md
    4.20), with u = 2^-24, H = |c|^2 / 2 and no underflow:
      E_chain = g sum_d |a_d c_d|, g = D u / (1 - D u)       the D roundings of the fma chain
      E_h     = (u + D 2^-52) H                              h = fp32 of an fp64 sum of D exact squares, halved exactly
      E_sub   = u (|a . c| + E_chain + H + E_h)              one rounding of acc - h, whose operands are at most that large
    bound = E_chain + E_h + E_sub."""
    u = 2.0 ** -24
    a64, c64 = a.astype(np.float64), c.astype(np.float64)
    dot = a64 @ c64.T
    D = a.shape[1]
    H = 0.5 * (c64 * c64).sum(1)[None, :]
    e_chain = D * u / (1.0 - D * u) * (np.abs(a64) @ np.abs(c64).T)
    e_h = (u + D * 2.0 ** -52) * H
    e_sub = u * (np.abs(dot) + e_chain + H + e_h)
    return dot - H, e_chain + e_h + e_sub


# ---- atoms -----------------------------------------------------------------------------------------------------------
def gaussian(seed: int, N: int, D: int) -> np.ndarray:
    return S.normal(seed, (N, D), stream=43)


def ternary(seed: int, N: int, D: int) -> np.ndarray:
    return NU.ternary(seed, N, D).astype(np.float32)


def planted(seed: int, N: int, D: int, C: int = 6, noise: float = 0.05):
    """(atoms, truth): C well-separated prototypes (Gaussian directions of norm about sqrt(D)) plus Gaussian noise of
    standard deviation `noise`; atom i belongs to prototype i % C, so atoms 0 .. C - 1 are one per cluster."""
    proto = S.normal(seed, (C, D), stream=44)
    truth = np.arange(N) % C
    return (proto[truth] + np.float32(noise) * S.normal(seed, (N, D), stream=45)).astype(np.float32), truth


RECIPES = {"gaussian": gaussian, "ternary": ternary, "planted": lambda seed, N, D: planted(seed, N, D)[0]}


def same_partition(labels: np.ndarray, truth: np.ndarray) -> bool:
    """Whether two labelings are the same partition up to the names of the clusters."""
    pairs = set(zip(labels.tolist(), truth.tolist()))
    return len(pairs) == len(set(labels.tolist())) == len(set(truth.tolist()))


# ---- the fixture -----------------------------------------------------------------------------------------------------
def golden_atoms() -> np.ndarray:
    """Ternary atoms [300, 64] of uneven sparsity: row i keeps a share 0.15 + 0.6 (i % 10) / 9 of its columns."""
    N, D = GOLDEN_N, GOLDEN_D
    u = S.uniform01(GOLDEN_SEED, N * D, stream=21).reshape(N, D)
    dens = (0.15 + 0.6 * (np.arange(N) % 10) / 9.0)[:, None]
    return np.where(u < dens / 2, -1, np.where(u < dens, 1, 0)).astype(np.float32)


def golden_lloyd(a: np.ndarray):
    """(labels, centers) the generator hands to the reference in place of kmeans_pytorch: one Lloyd run of the
    restatement into C - 1 clusters from atoms 0 .. C - 2, then an empty cluster (all-zero center, no member) is
    inserted at index GOLDEN_EMPTY, the labels at or above it moving up by one."""
    r = lloyd(a, a[:GOLDEN_C - 1].copy(), "cosine", 1e-4, 50)
    labels = r["labels"].copy()
    labels[labels >= GOLDEN_EMPTY] += 1
    return labels, np.insert(r["centers"], GOLDEN_EMPTY, 0.0, axis=0).astype(np.float32)


def load_golden() -> dict:
    z = np.load(GOLDEN / f"{GOLDEN_NAME}.npz")
    out = {k: z[k] for k in z.files}
    out["meta"] = json.loads(bytes(out["meta"]).decode())
    return out


def golden_groups(g: dict):
    """The recorded ragged cluster_ids_by_group as lists."""
    off = g["group_offsets"]
    return [g["group_members"][off[c]:off[c + 1]].tolist() for c in range(len(off) - 1)]
