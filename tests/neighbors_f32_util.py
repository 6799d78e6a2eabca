"""Shared helpers of the fp32 nearest-atom tests: the numpy restatement of the arithmetic contract --
inverse norms in the kernel's fp64 order, the exact fmaf chain through ``oracle.encode``, the scaling in fp32, keys and
their decode -- atom recipes from the portable PRNG of quantizedsae_amd/synthetic.py, and the cases of the fixtures
tests/golden/neighbors_f32_*.npz."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

import dictionary_neighbors_util as NU
import dictionary_util as DU
import oracle
from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"
GOLDEN_D, GOLDEN_H, GOLDEN_K = 64, 320, 10
VALUE_ATOL, CLEAR_GAP = 1e-5, 2e-5
# lhs / rhs: recipes of tests/dictionary_util.py; rhs None = self mode; rhs_H: the right side's H when it differs
GOLDEN_CASES = {
    "neighbors_f32_baseline": dict(lhs={"variant": "baseline", "seed": 42}, rhs=None),
    "neighbors_f32_matryoshka": dict(lhs={"variant": "matryoshka", "seed": 43}, rhs=None),
    "neighbors_f32_residual": dict(lhs={"variant": "residual", "seed": 44}, rhs=None),
    "neighbors_f32_binary_baseline": dict(lhs={"variant": "binary", "seed": 41}, rhs={"variant": "baseline", "seed": 42}),
    "neighbors_f32_binary_baseline_wide": dict(lhs={"variant": "binary", "seed": 41}, rhs={"variant": "baseline", "seed": 48},
                                               rhs_H=GOLDEN_H + 37),
}

mono, decode_keys = NU.mono, NU.decode_keys


# ---- the contract, restated ------------------------------------------------------------------------------------------
def inv_norms(a: np.ndarray) -> np.ndarray:
    """fp32 [N]: atom_inv_norms_kernel's order.  Lane l of 64 adds the fp64 squares of d = l, l + 64, ... in order from
    0.0, then the xor butterfly m = 32, 16, ..., 1; inv = fp32(1 / max(sqrt(s), 1e-12))."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    N, D = a.shape
    T = (D + 63) // 64
    sq = np.zeros((N, T * 64), dtype=np.float64)            # + 0.0 past D changes no partial sum
    v = a.astype(np.float64)
    sq[:, :D] = v * v
    sq = sq.reshape(N, T, 64)
    s = np.zeros((N, 64), dtype=np.float64)
    for t in range(T):
        s = s + sq[:, t, :]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ m]
    n = np.sqrt(s[:, 0])
    return (1.0 / np.where(n > 1e-12, n, 1e-12)).astype(np.float32)


def chain(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """acc[i, j]: fmaf over d ascending from +0 (the library's exact chain)."""
    return oracle.encode(np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32))


def cosines(a: np.ndarray, b: np.ndarray = None) -> np.ndarray:
    """c[i, j] = acc * (inv_a[i] * inv_b[j]): the inverse norms multiplied first, every operation rounded to fp32."""
    b = a if b is None else b
    scale = inv_norms(a)[:, None] * inv_norms(b)[None, :]
    return chain(a, b) * scale


def keys_of(c: np.ndarray, k: int, exclude_self: bool = False) -> np.ndarray:
    """int64 [Na, k]: the k largest keys mono(c) << 32 | ~j of every row, descending, 0 past the candidates."""
    Na, Nb = c.shape
    key = (mono(c).astype(np.uint64) << np.uint64(32)) | (~np.arange(Nb, dtype=np.uint32)).astype(np.uint64)[None, :]
    if exclude_self:
        assert Na == Nb
        key[np.arange(Na), np.arange(Na)] = 0
    if k < Nb:
        key = np.partition(key, Nb - k, axis=1)[:, Nb - k:]
    key = np.sort(key, axis=1)[:, ::-1]
    out = np.zeros((Na, k), dtype=np.uint64)
    out[:, :key.shape[1]] = key[:, :k]
    return out.view(np.int64)


def reference_keys(a: np.ndarray, b: np.ndarray = None, k: int = 10, exclude_self: bool = False) -> np.ndarray:
    assert not (exclude_self and b is not None)
    return keys_of(cosines(a, b), k, exclude_self)


def cosines_f64(a: np.ndarray, b: np.ndarray = None):
    """(c64, bound): the cosine in fp64 and the derived bound on |c - c64| of the restatement,
    (D + 5) * 2^-24 * sum_d |a_d b_d| / (|a| |b|): the forward error of a D-term fma chain plus the five roundings of
    the scaling (two inverse norms, their product, the final product, and the chain's own last rounding)."""
    b = a if b is None else b
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    na = np.maximum(np.sqrt((a64 * a64).sum(1)), 1e-12)
    nb = np.maximum(np.sqrt((b64 * b64).sum(1)), 1e-12)
    den = na[:, None] * nb[None, :]
    return (a64 @ b64.T) / den, (a.shape[1] + 5) * 2.0 ** -24 * (np.abs(a64) @ np.abs(b64).T) / den


# ---- atoms -----------------------------------------------------------------------------------------------------------
def baseline_like(seed: int, N: int, D: int) -> np.ndarray:
    """decoder.weight of a baseline SAE: U(+-1 / sqrt(N)), atoms as rows."""
    return DU.atoms_np({"variant": "baseline", "seed": seed}, D, N)


def matryoshka_like(seed: int, N: int, D: int) -> np.ndarray:
    """weight + weight_mirror of a matryoshka decoder."""
    return DU.atoms_np({"variant": "matryoshka", "seed": seed}, D, N)


def integer_valued(seed: int, N: int, D: int) -> np.ndarray:
    """4-bit two's complement integers as fp32: every dot product is exact in the chain."""
    return NU.nbit(seed, N, D).astype(np.float32)


def gaussian(seed: int, N: int, D: int) -> np.ndarray:
    return S.normal(seed, (N, D), stream=41)


RECIPES = {"baseline": baseline_like, "matryoshka": matryoshka_like, "integer": integer_valued}


# ---- fixtures --------------------------------------------------------------------------------------------------------
def case_sizes(case: dict):
    return GOLDEN_D, GOLDEN_H, int(case.get("rhs_H", GOLDEN_H))


def golden_atoms(case: dict):
    """(a, b or None): the fp32 atoms of a fixture's two sides, restated in numpy."""
    D, H, Hr = case_sizes(case)
    a = DU.atoms_np(case["lhs"], D, H)
    return a, (None if case["rhs"] is None else DU.atoms_np(case["rhs"], D, Hr))


def golden_models(classes, case: dict):
    """(lhs, rhs or None) built with ``classes`` (this package or the reference: same constructors)."""
    D, H, Hr = case_sizes(case)
    lhs = DU.build(classes, case["lhs"], D, H)
    return lhs, (None if case["rhs"] is None else DU.build(classes, case["rhs"], D, Hr))


def load_golden(name: str) -> dict:
    z = np.load(GOLDEN / f"{name}.npz")
    out = {k: z[k] for k in z.files}
    out["meta"] = json.loads(bytes(out["meta"]).decode())
    return out


def clear_rows(values: np.ndarray) -> np.ndarray:
    """Rows of the recorded [N, k + 1] descending values whose consecutive gaps all exceed CLEAR_GAP."""
    v = values.astype(np.float64)
    return ((v[:, :-1] - v[:, 1:]) > CLEAR_GAP).all(axis=1)


def check_against_golden(g: dict, sim: np.ndarray, idx: np.ndarray) -> float:
    """sim / idx [N, k] (ours) against the reference's recorded torch.topk(k + 1): values at VALUE_ATOL, indices equal
    in the rows whose recorded consecutive gaps all exceed CLEAR_GAP.  Returns the share of such rows."""
    k = int(g["meta"]["k"])
    rv, ri = g["values"], g["indices"]
    assert sim.shape == idx.shape == (rv.shape[0], k)
    np.testing.assert_allclose(sim, rv[:, :k], rtol=0, atol=VALUE_ATOL)
    clear = clear_rows(rv)
    assert np.array_equal(idx[clear], ri[clear][:, :k])
    return float(clear.mean())
