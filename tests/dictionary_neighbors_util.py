"""Shared helpers of the nearest-atom tests: the numpy restatement of the arithmetic contract, int8
dictionary recipes from the portable PRNG of quantizedsae_amd/synthetic.py, and the model recipes of the fixtures
tests/golden/nearest_atoms_*.npz."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"
GOLDEN_D, GOLDEN_H, GOLDEN_K, N_BITS, GAMMA = 64, 512, 10, 4, 1.5
GOLDEN_CASES = {
    "nearest_atoms_ternary": {"variant": "ternary", "seed": 51},
    "nearest_atoms_binary4": {"variant": "binary", "seed": 52},
    # ternary with planted all-zero atoms and duplicates (a pair, a triple and the zeros themselves)
    "nearest_atoms_zero_dup": {"variant": "ternary", "seed": 53, "zero": [0, 7, 300], "copy": [[5, 400], [9, 130], [9, 511]]},
}


# ---- the contract, restated ------------------------------------------------------------------------------------------
def norms(a: np.ndarray):
    """nsq int32 [N] exact; inv = fp32(1 / sqrt(fp64(nsq))), 1.0 for an all-zero atom."""
    a64 = a.astype(np.int64)
    nsq = (a64 * a64).sum(1)
    with np.errstate(divide="ignore"):
        inv = np.where(nsq > 0, (1.0 / np.sqrt(nsq.astype(np.float64))).astype(np.float32), np.float32(1.0))
    return nsq.astype(np.int32), inv.astype(np.float32)


def dots(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Exact int32 products (fp64 BLAS: every partial sum is an integer below 2^53)."""
    return (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int32)


def cosines(a: np.ndarray, b: np.ndarray = None) -> np.ndarray:
    """c[i, j] = fp32(dot) * (inva[i] * invb[j]), every operation in fp32 with one rounding."""
    b = a if b is None else b
    _, ia = norms(a)
    _, ib = norms(b)
    scale = ia[:, None] * ib[None, :]                       # fp32 * fp32 -> fp32
    return dots(a, b).astype(np.float32) * scale


def mono(c: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(c, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def reference_keys(a: np.ndarray, b: np.ndarray = None, k: int = 10, exclude_self: bool = False) -> np.ndarray:
    """int64 [Na, k]: the k largest keys mono(c) << 32 | ~j of every row, descending, 0 past the candidates."""
    c = cosines(a, b)
    Na, Nb = c.shape
    key = (mono(c).astype(np.uint64) << np.uint64(32)) | (~np.arange(Nb, dtype=np.uint32)).astype(np.uint64)[None, :]
    if exclude_self:
        assert b is None
        key[np.arange(Na), np.arange(Na)] = 0
    if k < Nb:
        key = np.partition(key, Nb - k, axis=1)[:, Nb - k:]
    key = np.sort(key, axis=1)[:, ::-1]
    out = np.zeros((Na, k), dtype=np.uint64)
    out[:, :key.shape[1]] = key[:, :k]
    return out.view(np.int64)


def decode_keys(keys: np.ndarray):
    """-> (similarity fp32, index int64); none -> (-inf, -1)."""
    u = keys.view(np.uint64)
    hi = (u >> np.uint64(32)).astype(np.uint32)
    bits = np.where(hi & 0x80000000, hi ^ np.uint32(0x80000000), ~hi).astype(np.uint32)
    sim = bits.view(np.float32).copy()
    idx = (~(u & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64)
    none = u == 0
    sim[none] = -np.inf
    idx[none] = -1
    return sim, idx


def reference_duplicate_of(a: np.ndarray) -> np.ndarray:
    """The lowest index holding an identical row (by bytes, as the reference's Counter over tuples)."""
    first, out = {}, np.empty((a.shape[0],), dtype=np.int32)
    for i, row in enumerate(np.ascontiguousarray(a)):
        out[i] = first.setdefault(row.tobytes(), i)
    return out


def n_duplicate_groups(dup: np.ndarray) -> int:
    return int(np.unique(dup[dup != np.arange(dup.size)]).size)


def cosines_f64(a: np.ndarray, b: np.ndarray = None) -> np.ndarray:
    """Real arithmetic, to fp64: dot / sqrt(nsq_a nsq_b), 0 where an atom is all-zero."""
    b = a if b is None else b
    na = np.sqrt((a.astype(np.float64) ** 2).sum(1))
    nb = np.sqrt((b.astype(np.float64) ** 2).sum(1))
    na[na == 0] = 1.0
    nb[nb == 0] = 1.0
    return (a.astype(np.float64) @ b.astype(np.float64).T) / na[:, None] / nb[None, :]


# ---- dictionaries ----------------------------------------------------------------------------------------------------
def ternary(seed: int, N: int, D: int, density: float = 0.4) -> np.ndarray:
    u = S.uniform01(seed, N * D, stream=21).reshape(N, D)
    return np.where(u < density / 2, -1, np.where(u < density, 1, 0)).astype(np.int8)


def nbit(seed: int, N: int, D: int, bits: int = 4) -> np.ndarray:
    h = S.hash_u64(seed, N * D, stream=22) >> np.uint64(40)
    return ((h % np.uint64(1 << bits)).astype(np.int64) - (1 << (bits - 1))).astype(np.int8).reshape(N, D)


def full_int8(seed: int, N: int, D: int) -> np.ndarray:
    """Every int8 value, -128 included."""
    return nbit(seed, N, D, 8)


RECIPES = {"ternary": ternary, "nbit4": nbit, "int8": full_int8}


# ---- fixtures --------------------------------------------------------------------------------------------------------
def golden_state_dict(spec: dict, D: int = GOLDEN_D, H: int = GOLDEN_H) -> dict:
    if spec["variant"] == "binary":
        return S.binary_sae_params(spec["seed"], D, H, N_BITS)
    # Atoms of uneven sparsity (a per-atom scale spread over a factor 8 around w_std = 1.5: 17 to 60 non-zeros of 64).
    # With one density for all atoms, dot / sqrt(n_i n_j) of a ternary dictionary at D = 64 takes so few values that a
    # quarter of the rows tie exactly at the k-th neighbour and could not be compared with the reference's indices.
    sd = S.ternary_sae_params(spec["seed"], D, H, w_std=1.5)
    scale = np.exp((S.uniform01(spec["seed"], H, stream=31) - 0.5) * np.log(8.0)).astype(np.float32)
    w = sd["decoder.weight"] * scale[None, :]               # [D, H]: atom h is column h
    for z in spec.get("zero", ()):
        w[:, z] = 0.0
    for src, dst in spec.get("copy", ()):
        w[:, dst] = w[:, src]
    sd["decoder.weight"] = w
    return sd


def golden_model(classes, spec: dict, D: int = GOLDEN_D, H: int = GOLDEN_H):
    """classes: namespace with BinarySAE and TernarySparseAutoencoder (this package's or the reference's)."""
    import torch
    if spec["variant"] == "binary":
        m = classes.BinarySAE(D, H, gamma=GAMMA, n_bits=N_BITS)
    else:
        m = classes.TernarySparseAutoencoder(D, H)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in golden_state_dict(spec, D, H).items()},
                      strict=False)
    return m.eval()


def golden_atoms(spec: dict, D: int = GOLDEN_D, H: int = GOLDEN_H) -> np.ndarray:
    """The int8 atoms [H, D] of a fixture's model, restated in numpy."""
    sd = golden_state_dict(spec, D, H)
    if spec["variant"] == "binary":
        w = sd["decoder.weight"].reshape(H, D, N_BITS) > 0          # saturated logits: bit = w > 0
        ints = sum(w[..., j].astype(np.int64) << j for j in range(N_BITS))
        return np.where(ints >= 1 << (N_BITS - 1), ints - (1 << N_BITS), ints).astype(np.int8)
    w = sd["decoder.weight"]
    return np.ascontiguousarray((np.sign(w) * (np.abs(w) >= 0.5)).T).astype(np.int8)


def load_golden(name: str) -> dict:
    z = np.load(GOLDEN / f"{name}.npz")
    out = {k: z[k] for k in z.files}
    out["meta"] = json.loads(bytes(out["meta"]).decode())
    return out


def check_against_golden(g: dict, dist: np.ndarray, idx: np.ndarray) -> float:
    """dist / idx [N, k] (ours, k = the fixture's) against the reference's k + 1 recorded neighbours.  Distances within
    ref_fp64_maxdev + 3e-7; index sets equal on the rows whose recorded k-th and (k+1)-th distances are further apart
    than twice that.  Returns the share of such rows."""
    k = int(g["meta"]["k"])
    tol = float(g["ref_fp64_maxdev"]) + 3e-7
    rd, ri = g["nn_dist"], g["nn_index"]                   # [N, k + 1] ascending
    assert dist.shape == (rd.shape[0], k)
    assert np.abs(dist.astype(np.float64) - rd[:, :k].astype(np.float64)).max() <= tol
    clear = (rd[:, k].astype(np.float64) - rd[:, k - 1].astype(np.float64)) > 2 * tol
    # inside the k columns equal distances may be ordered differently (sklearn's order is unspecified): compare sets
    same = np.array([set(idx[i].tolist()) == set(ri[i, :k].tolist()) for i in np.nonzero(clear)[0]])
    assert same.all(), f"{(~same).sum()} rows differ"
    return float(clear.mean())
