"""Recipes of the token-overlap fixtures (tests/golden/token_overlap_*.npz) and a plain numpy integer formulation of the
(intersection, union) histogram.

Token lists come from the portable counter hash of quantizedsae_amd/synthetic.py (no library RNG stream): list lengths
from ``hash_u64``, token ids as floor(V * u ** power) with ``uniform01`` -- power 3 is Zipf-like (a few tokens in most
lists), power near 1 flat.  The first features of each side are planted so that every rule of the reference's set
construction decides something (see ``token_lists``)."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"

# (Na, Nb, V, k) as in the issue; power / max_len chosen so that the coverage conditions of the generator hold
RECIPES = {
    "token_overlap_k10": dict(Na=300, Nb=260, V=1030, k=10, seed=71, power=3.0, max_len=60),
    "token_overlap_k100": dict(Na=97, Nb=130, V=300, k=100, seed=72, power=3.0, max_len=900),
    "token_overlap_k3": dict(Na=64, Nb=70, V=40, k=3, seed=73, power=3.0, max_len=12),
    "token_overlap_k128": dict(Na=260, Nb=33, V=513, k=128, seed=74, power=3.0, max_len=1500),
    "token_overlap_flat": dict(Na=150, Nb=170, V=4099, k=20, seed=75, power=1.2, max_len=120),
}


def _side(recipe: dict, side: int):
    N = recipe["Nb"] if side else recipe["Na"]
    V, k, seed = recipe["V"], recipe["k"], recipe["seed"]
    lengths = (S.hash_u64(seed, N, stream=10 + side) % np.uint64(recipe["max_len"] + 1)).astype(np.int64)
    lengths[lengths % 7 == 3] = 0                                  # a share of empty lists
    u = S.uniform01(seed, int(lengths.sum()), stream=20 + side)
    flat = np.minimum((V * u ** recipe["power"]).astype(np.int64), V - 1)
    ends = np.cumsum(lengths)
    lists = [flat[e - n:e].tolist() for e, n in zip(ends, lengths)]
    # planted features
    lists[0] = []                                                   # never active, empty
    lists[2] = [V - 1, 7 % V, V - 1] if k > 2 else [V - 1]          # a set smaller than k, with the last token id
    # k + 1 distinct tokens, once each, in descending id order: all tie, the first k by occurrence are the set
    lists[3] = [V - 1 - 2 * j if V > 2 * (k + 1) else V - 1 - j for j in range(k + 1)]
    act = np.array([len(t) for t in lists], dtype=np.int64)
    act[1] = 0                                                      # a list, but activation_counts == 0
    if not lists[1]:
        lists[1] = [3 % V, 5 % V]
    return lists, act


def token_lists(recipe: dict):
    """-> (lists_a, act_a, lists_b, act_b).  Features 0..3 of each side: never active; inactive with a list; a small
    set holding token V - 1; the k-th / (k + 1)-th tie.  B's feature 5 is a copy of A's feature 4 (score 1.0)."""
    la, aa = _side(recipe, 0)
    lb, ab = _side(recipe, 1)
    if not la[4]:
        la[4] = [1 % recipe["V"], 0, 1 % recipe["V"]]
        aa[4] = 3
    lb[5] = list(la[4])
    ab[5] = len(lb[5])
    return la, aa, lb, ab


def csr(lists):
    lengths = np.array([len(t) for t in lists], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    tokens = np.array([t for lst in lists for t in lst], dtype=np.int64)
    return offsets, tokens


def load(name: str):
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {key: z[key] for key in z.files if key != "meta"}


def membership(sets: np.ndarray, V: int) -> np.ndarray:
    """uint8 [N, V] from padded sets [N, k] (-1 = nothing)."""
    M = np.zeros((sets.shape[0], V), dtype=np.uint8)
    rows, cols = np.nonzero(sets >= 0)
    M[rows, sets[rows, cols]] = 1
    return M


def pack(M: np.ndarray, words: int = None) -> np.ndarray:
    """int32 [N, words] from a 0/1 matrix [N, V]: bit t & 31 of word t >> 5 is column t."""
    N, V = M.shape
    words = (V + 31) // 32 if words is None else words
    padded = np.zeros((N, words * 32), dtype=np.uint64)
    padded[:, :V] = M
    shifted = padded.reshape(N, words, 32) << np.arange(32, dtype=np.uint64)
    return shifted.sum(axis=2).astype(np.uint32).view(np.int32)


def hist_numpy(Ma: np.ndarray, asize: np.ndarray, Mb: np.ndarray, bsize: np.ndarray, k: int) -> np.ndarray:
    """int64 [k + 1, 2k + 1]: the integer product of the membership matrices, then a bincount of (inter, union) over
    the pairs the kernel counts: both sizes in 1..k and an intersection no larger than either size."""
    assert Ma.shape[1] < 1 << 24                                    # counts below 2^24 are exact in fp32 (and use BLAS)
    inter = (Ma.astype(np.float32) @ Mb.astype(np.float32).T).astype(np.int64)
    sa, sb = np.asarray(asize, dtype=np.int64)[:, None], np.asarray(bsize, dtype=np.int64)[None, :]
    ok = (sa > 0) & (sa <= k) & (sb > 0) & (sb <= k) & (inter <= np.minimum(sa, sb))
    union = sa + sb - inter
    flat = (inter * (2 * k + 1) + union)[ok]
    return np.bincount(flat, minlength=(k + 1) * (2 * k + 1)).reshape(k + 1, 2 * k + 1).astype(np.int64)


def hist_from_triples(triples: np.ndarray, k: int) -> np.ndarray:
    h = np.zeros((k + 1, 2 * k + 1), dtype=np.int64)
    h[triples[:, 0], triples[:, 1]] = triples[:, 2]
    return h


def random_sets(seed: int, N: int, V: int, k: int, density: float, stream: int):
    """0/1 matrix [N, V] with row sizes spread over 0..k, and its sizes: each column is a candidate with probability
    ``density``; a row keeps its first size[i] candidates (fewer when it has fewer)."""
    cand = S.uniform01(seed, N * V, stream=stream).reshape(N, V) < density
    want = (S.hash_u64(seed, N, stream=stream + 1) % np.uint64(k + 1)).astype(np.int64)
    M = (cand & (np.cumsum(cand, axis=1) <= want[:, None])).astype(np.uint8)
    return M, M.sum(axis=1).astype(np.int32)
