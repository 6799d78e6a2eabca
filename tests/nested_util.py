"""Shared helpers of the nested-dictionary tests: the numpy restatement of the contract of include/qsae_nested.h.

``nested_recons``: for every level the CPU oracle's sparse decode (the fmaf chain in ascending unit index, ``* step`` /
``* scale``, ``+ bias``) of each row's list with the entries of units ``>= bounds[l]`` -- and the entries whose id lies outside
[0, H) -- removed.  ``suffix_sums``: G[l] = fl32(g[l] + G[l + 1]) over the levels that have a gradient.  ``grads64``: the
gradient table of tests/train_util.py::grads64 in fp64 with g_recon replaced per entry by G[level(unit)]."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from quantizedsae_amd import synthetic as S
from sparsity_curve_util import gaussian, packed_dictionary, ranked_lists
from train_util import _t, soft_table64

__all__ = ["nested_recons", "levels_of", "suffix_sums", "grads64", "build_case", "CASES", "EMU_CASES"]


def _decode(idx, val, decoder, bias):
    if decoder[0] == "packed":
        _, packed, D, n_bits, step = decoder
        return oracle.decode_binary(idx, val, packed, D, n_bits, step, bias)
    _, table, scale = decoder
    return oracle.decode_table(idx, val, table, scale, bias)


def levels_of(idx, bounds) -> np.ndarray:
    """level(h) = the smallest l with h < bounds[l] = the number of bounds <= h (ids are taken as they are)"""
    return np.searchsorted(np.asarray(bounds, dtype=np.int64), np.asarray(idx, dtype=np.int64), side="right")


def nested_recons(idx, val, bounds, decoder, bias) -> np.ndarray:
    """-> fp32 [L, B, D].  ``decoder`` = ("packed", packed uint8 [H, row_bytes], D, n_bits, step) or ("table", fp32 [H, D],
    scale), on the host."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float32)
    H = decoder[1].shape[0]
    assert list(bounds) == sorted(set(bounds)) and bounds[0] > 0 and bounds[-1] == H
    B = idx.shape[0]
    inside = idx >= 0
    out = []
    for b in bounds:
        keep = inside & (idx < b)
        if B and (keep == keep[:1]).all():                    # every row keeps the same positions: one call
            out.append(_decode(np.ascontiguousarray(idx[:, keep[0]]), np.ascontiguousarray(val[:, keep[0]]), decoder, bias))
            continue
        rows = [_decode(idx[r:r + 1][:, keep[r]], val[r:r + 1][:, keep[r]], decoder, bias)[0] for r in range(B)]
        out.append(np.stack(rows))
    return np.stack(out).astype(np.float32)


def suffix_sums(g_levels, B: int, D: int) -> np.ndarray:
    """-> fp32 [L, B, D]: the last level that has a gradient is copied, every one before it adds its own (fp32) or, absent,
    copies its successor; the levels after the last gradient are +0."""
    L = len(g_levels)
    G = np.zeros((L, B, D), dtype=np.float32)
    acc = None
    for l in range(L - 1, -1, -1):
        if g_levels[l] is not None:
            g = np.asarray(g_levels[l], dtype=np.float32)
            acc = g.copy() if acc is None else (g + acc).astype(np.float32)
        if acc is not None:
            G[l] = acc
    return G


def grads64(x, W, table, step: float, idx, val, G, bounds, g_latent_sel=None, want_dx: bool = False):
    """The table of DESIGN.md section 4.10 in fp64 with the reconstruction gradient of entry (r, j) = G[level(idx[r, j])][r]:
    -> dict of gv [B, k], encoder.0.weight [H, D], encoder.0.bias [H], rows [H, D] (= sum val G[level(h)][r]: the baseline's
    decoder.weight gradient transposed; times step it is BinarySAE's dInt), decoder.bias [D], x (if want_dx)."""
    x, W, T, val = _t(x), _t(W), _t(table), _t(val)
    G = _t(G)
    idx = torch.as_tensor(np.asarray(idx)).long()
    B, D = x.shape
    H = W.shape[0]
    lev = torch.from_numpy(levels_of(idx.numpy(), bounds)).long()                 # [B, k]
    rows = torch.arange(B)[:, None].expand_as(idx)
    Ge = G[lev, rows]                                                               # [B, k, D]
    gv = _t(g_latent_sel).clone() if g_latent_sel is not None else torch.zeros(idx.shape, dtype=torch.float64)
    gv = gv + step * torch.einsum("rjd,rjd->rj", Ge, T[idx])
    flat = idx.reshape(-1)
    dW = torch.zeros((H, D), dtype=torch.float64).index_add_(0, flat, (gv[:, :, None] * x[:, None, :]).reshape(-1, D))
    db = torch.zeros((H,), dtype=torch.float64).index_add_(0, flat, gv.reshape(-1))
    Sg = torch.zeros((H, D), dtype=torch.float64).index_add_(0, flat, (val[:, :, None] * Ge).reshape(-1, D))
    out = {"gv": gv, "encoder.0.weight": dW, "encoder.0.bias": db, "rows": Sg, "decoder.bias": G[0].sum(0)}
    if want_dx:
        out["x"] = torch.einsum("rj,rjd->rd", gv, W[idx])
    return out


def logit_grads64(rows, logits, D: int, n_bits: int, step: float, g_pol=None):
    """BinarySAE's logit gradient from ``rows`` of grads64 (dInt = step * rows), with the polarize term"""
    _, p = soft_table64(logits, D, n_bits)
    H = p.shape[0]
    bw = 2.0 ** torch.arange(n_bits, dtype=torch.float64)
    pw = bw.clone()
    bw[-1] = -bw[-1]
    gp = float(g_pol) if g_pol is not None else 0.0
    dl = ((step * _t(rows))[:, :, None] * bw + gp * pw * (1 - 2 * p) / (H * D * n_bits)) * p * (1 - p)
    return dl.reshape(H, D * n_bits)


# ---- inputs -----------------------------------------------------------------------------------------------------------
#: the issue's op-level shapes: B = 7, H = 512, k = 6, bounds = [1, 33, 64, 512]; D in {4, 48, 520}; n_bits in {1, 4, 8} and the
#: table form; and one case with B = 3, k = 256, H = 300, bounds = [7, 300]
BOUNDS = [1, 33, 64, 512]


def cases():
    out = {}
    for D in (4, 48, 520):
        for n in (1, 4, 8):
            out[f"packed_D{D}_n{n}"] = ("packed", D, n, True, 7, 6, 512, BOUNDS)
        out[f"table_D{D}_s1.0"] = ("table", D, 1.0, True, 7, 6, 512, BOUNDS)
        out[f"table_D{D}_s0.5_nobias"] = ("table", D, 0.5, False, 7, 6, 512, BOUNDS)
    out["packed_k256"] = ("packed", 48, 4, True, 3, 256, 300, [7, 300])
    out["table_k256"] = ("table", 48, 0.5, True, 3, 256, 300, [7, 300])
    out["packed_last_level_only"] = ("packed", 48, 4, True, 7, 6, 512, BOUNDS)
    out["table_last_level_only"] = ("table", 48, 0.5, True, 7, 6, 512, BOUNDS)
    out["table_one_level"] = ("table", 48, 0.5, True, 7, 6, 512, [512])
    out["packed_eight_levels"] = ("packed", 36, 3, True, 5, 9, 64, [1, 2, 3, 8, 9, 32, 63, 64])
    return out


CASES = cases()
#: the subset the host emulation runs (one thread per lane)
EMU_CASES = ["packed_D4_n1", "packed_D48_n4", "packed_D520_n8", "table_D4_s1.0", "table_D520_s0.5_nobias", "packed_k256",
             "table_k256", "table_last_level_only", "packed_eight_levels", "table_one_level"]


def build_case(name: str):
    """-> (idx, val, bounds, decoder (host form), bias or None).  The first rows carry what the levels are there to separate:
    row 0 selects unit 0 (a bound of one unit), row 1 nothing below bounds[1] (levels without an entry) -- unless the case is
    *_last_level_only, where every entry of every row lies in the last level."""
    kind, D, par, with_bias, B, k, H, bounds = CASES[name]
    seed = 3000 + sorted(CASES).index(name)
    idx, val = ranked_lists(seed + 1, B, k, H)
    if k < H and len(bounds) > 1:
        lo = bounds[-2]
        if name.endswith("last_level_only"):
            idx = (lo + (idx.astype(np.int64) * 7 + np.arange(k)[None, :] * 61) % (H - lo)).astype(np.int32)
            for r in range(B):                                # keep a row's ids distinct
                seen = set()
                for j in range(k):
                    h = int(idx[r, j])
                    while h in seen:
                        h = lo + (h - lo + 1) % (H - lo)
                    seen.add(h)
                    idx[r, j] = h
        else:
            if 0 not in idx[0]:
                idx[0, k // 2] = 0
            moved = idx[1] < bounds[min(1, len(bounds) - 2)]
            free = [h for h in range(H - 1, 0, -1) if h not in set(idx[1].tolist())]
            idx[1, moved] = np.array(free[:int(moved.sum())], dtype=np.int32)
    bias = gaussian(seed + 2, 1, D)[0] if with_bias else None
    if kind == "packed":
        decoder = ("packed", packed_dictionary(seed + 3, H, D, par), D, par, 0.25)
    else:
        decoder = ("table", gaussian(seed + 3, H, D), par)
    return np.ascontiguousarray(idx), val, list(bounds), decoder, bias


# ---- special values ---------------------------------------------------------------------------------------------------
SPECIAL_CASES = ("inf_behind_a_bound", "minus_zero", "packed_ids_outside", "table_ids_outside")
SPECIAL_BOUNDS = [8, 32, 64]
INF_UNIT, INF_COLUMN = 40, 7


def special_case(name: str):
    """-> (idx, val, bounds, decoder (host form), bias).  inf_behind_a_bound: unit 40 (last level) of every row's list has an
    inf column; minus_zero: the values of row 0 are all +-0 under a negative scale and no bias; *_ids_outside: an id below 0
    and ids at or above H in every row."""
    B, D, H, k = 4, 36, 64, 8
    seed = 4000 + SPECIAL_CASES.index(name)
    idx, val = ranked_lists(seed + 1, B, k, H)
    bias = gaussian(seed + 2, 1, D)[0]
    if name.startswith("packed"):
        decoder = ("packed", packed_dictionary(seed + 3, H, D, 4), D, 4, 0.25)
    else:
        decoder = ("table", gaussian(seed + 3, H, D), 0.5)
    if name == "inf_behind_a_bound":
        table = decoder[1].copy()
        for r in range(B):
            if INF_UNIT not in idx[r]:
                idx[r, 3] = INF_UNIT
        table[INF_UNIT, INF_COLUMN] = np.inf
        decoder = ("table", table, 0.5)
    elif name == "minus_zero":
        val[0, 0::2] = -0.0
        val[0, 1::2] = 0.0
        decoder, bias = ("table", decoder[1], -0.5), None
    elif name.endswith("ids_outside"):
        idx[:, 2] = -3
        idx[:, 6] = H + 5
        idx[0, 0] = H
    return idx, val, list(SPECIAL_BOUNDS), decoder, bias


def check_special(name: str, recons: np.ndarray) -> None:
    """What the case is there to show, on the levels [L, B, D] a run produced."""
    if name == "inf_behind_a_bound":
        assert np.isfinite(recons[:2]).all()                 # unit 40 takes no part below its bound
        assert (~np.isfinite(recons[2][:, INF_COLUMN])).all()
    elif name == "minus_zero":
        assert not recons[:, 0].view(np.uint32).any()        # +0 at every level, never -0
