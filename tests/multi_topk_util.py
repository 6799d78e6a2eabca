"""Shared helpers of the Multi-TopK tests: the numpy restatement of the contract of include/qsae_multik.h and the case table.

``recons``: for every point the CPU oracle's sparse decode of each row's list cut at ``ks[p]`` (tests/sparsity_curve_util.py
states the same contract for the curve).  ``points_of``: point(j) = the smallest p with j < ks[p].  ``row_grad``: the suffix
sums G (tests/nested_util.py), then gv and dx in the operation order of the row kernel -- per lane an fmaf chain over its column
quads, the xor butterfly over the 64 lanes, ``step *``, ``g_latent +``; dx one fmaf chain per column in list order -- every fmaf
through the oracle's ``dot_chain``, so the result is fp32 bit for bit.  ``unit_grads``: the unit sums over the lists of
qsae_train_csr (entries of a unit in ascending row), chunked at 256 entries, partials added in chunk order, with
g_recon = G[point(e % K)] per entry: dW_enc, db_enc and ``rows`` = sum val G (the table form's decoder gradient, transposed;
``step * rows`` is BinarySAE's dInt).  The logit gradient goes through a sigmoid and is not restated in bits; ``grads64`` gives
every gradient in fp64."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from nested_util import logit_grads64, suffix_sums
from sparsity_curve_util import gaussian, packed_dictionary, prefix_recons, ranked_lists
from train_util import _t

__all__ = ["recons", "points_of", "row_grad", "unit_grads", "grads64", "build_case", "CASES", "EMU_CASES", "suffix_sums",
           "logit_grads64"]

CHUNK = 256                                                  # entries of a unit list that one workgroup sums (kTrainChunk)


def points_of(K: int, ks) -> np.ndarray:
    """point(j) for j = 0 .. K - 1: the number of ks[p] <= j"""
    return np.searchsorted(np.asarray(ks, dtype=np.int64), np.arange(K, dtype=np.int64), side="right")


def recons(idx, val, ks, decoder, bias) -> np.ndarray:
    """-> fp32 [P, B, D]; ``decoder`` = ("packed", packed uint8 [H, row_bytes], D, n_bits, step) or ("table", fp32 [H, D], scale)"""
    assert list(ks) == sorted(set(ks)) and ks[0] > 0 and ks[-1] == np.asarray(idx).shape[1]
    return prefix_recons(idx, val, ks, decoder, bias)


def _chain(a, b) -> np.float32:
    return oracle.dot_chain(np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32), 0.0)


def row_grad(idx, table, step, g_points, ks, g_latent, W):
    """-> (G [P, B, D], gv [B, K], dx [B, D] or None), fp32 bit for bit.  Ids are clamped into [0, H) as the kernel does."""
    idx = np.asarray(idx)
    B, K = idx.shape
    H, D = table.shape
    G = suffix_sums(g_points, B, D)
    pt = points_of(K, ks)
    h = np.clip(idx, 0, H - 1)
    D4 = D // 4
    step = np.float32(step)
    gv = np.zeros((B, K), dtype=np.float32)
    for r in range(B):
        for j in range(K):
            g, t = G[pt[j], r], table[h[r, j]]
            part = np.zeros(64, dtype=np.float32)
            for lane in range(min(64, D4)):
                cols = np.concatenate([np.arange(4 * q, 4 * q + 4) for q in range(lane, D4, 64)])
                part[lane] = _chain(g[cols], t[cols])
            for off in (32, 16, 8, 4, 2, 1):
                part = (part + part[np.arange(64) ^ off]).astype(np.float32)
            v = np.float32(step * part[0])
            if g_latent is not None:
                v = np.float32(g_latent[r, h[r, j]] + v)
            gv[r, j] = v
    dx = None
    if W is not None:
        dx = np.zeros((B, D), dtype=np.float32)
        for r in range(B):
            Wr = np.ascontiguousarray(W[h[r]].T)                 # [D, K]
            for d in range(D):
                dx[r, d] = _chain(gv[r], Wr[d])
    return G, gv, dx


def csr(idx, H: int):
    """-> (offsets int32 [H + 1], entries int32 [B K]) as qsae_train_csr writes them for ids inside [0, H)"""
    idx = np.asarray(idx)
    B, K = idx.shape
    flat = idx.reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind="stable")                  # flat index r K + j ascending within a unit = ascending row
    counts = np.bincount(flat, minlength=H)
    offsets = np.zeros(H + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    return offsets, order.astype(np.int32)


def unit_grads(idx, val, gv, x, G, ks, H: int):
    """-> dict of dW [H, D], db [H], rows [H, D], fp32 bit for bit (G None: rows are +0).  Ids inside [0, H), distinct per row."""
    idx = np.asarray(idx)
    B, K = idx.shape
    D = x.shape[1]
    pt = points_of(K, ks)
    offsets, entries = csr(idx, H)
    vflat, gflat = np.asarray(val, np.float32).reshape(-1), np.asarray(gv, np.float32).reshape(-1)
    dW = np.zeros((H, D), dtype=np.float32)
    db = np.zeros((H,), dtype=np.float32)
    rows = np.zeros((H, D), dtype=np.float32)
    for h in range(H):
        lo, hi = int(offsets[h]), int(offsets[h + 1])
        if hi == lo:
            continue
        parts = []
        for c0 in range(lo, hi, CHUNK):
            e = entries[c0:min(c0 + CHUNK, hi)].astype(np.int64)
            r, j = e // K, e % K
            X = np.ascontiguousarray(x[r].T)                                    # [D, len]
            Gm = np.ascontiguousarray(G[pt[j], r].T) if G is not None else None
            w = np.array([_chain(gflat[e], X[d]) for d in range(D)], dtype=np.float32)
            s = np.array([_chain(vflat[e], Gm[d]) for d in range(D)], dtype=np.float32) if Gm is not None else np.zeros(D, np.float32)
            b = np.float32(0.0)
            for v in gflat[e]:
                b = np.float32(b + v)
            parts.append((w, s, b))
        if len(parts) == 1:
            dW[h], rows[h], db[h] = parts[0]
        else:                                                # a split list: the chunk partials are added to +0 in chunk order
            w, s, b = np.zeros(D, np.float32), np.zeros(D, np.float32), np.float32(0.0)
            for pw, ps, pb in parts:
                w, s, b = (w + pw).astype(np.float32), (s + ps).astype(np.float32), np.float32(b + pb)
            dW[h], rows[h], db[h] = w, s, b
    return {"dW": dW, "db": db, "rows": rows}


def grads64(x, W, table, step: float, idx, val, G, ks, g_latent_sel=None, want_dx: bool = False):
    """Every gradient in fp64 with the reconstruction gradient of entry (r, j) = G[point(j)][r] (tests/nested_util.py::grads64
    with the level of the unit replaced by the point of the rank)."""
    x, W, T, val = _t(x), _t(W), _t(table), _t(val)
    G = _t(G)
    idx = torch.as_tensor(np.asarray(idx)).long()
    B, D = x.shape
    H = W.shape[0]
    pt = torch.from_numpy(points_of(idx.shape[1], ks)).long()[None, :].expand_as(idx)
    rows = torch.arange(B)[:, None].expand_as(idx)
    Ge = G[pt, rows]                                                                # [B, K, D]
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


# ---- inputs -----------------------------------------------------------------------------------------------------------
#: name -> (kind, D, n_bits or scale, with bias, B, K, H, ks).  B in {1, 5, 9}, K in {1, 7, 12, 65, 256}, D in {4, 48, 516, 520},
#: H <= 600, n_ks in {1, 2, 4, 5, 8} (5: the second gather trip), n_bits in {1, 4, 8}, scale in {1, 0.5}
def cases():
    out = {
        "packed_K1_D4_n1": ("packed", 4, 1, True, 1, 1, 8, [1]),
        "table_K1_D4": ("table", 4, 1.0, False, 1, 1, 8, [1]),
        "packed_K7_D48_n4": ("packed", 48, 4, True, 5, 7, 600, [1, 7]),
        "table_K7_D48": ("table", 48, 1.0, True, 5, 7, 600, [1, 7]),
        "packed_K12_D516_n8": ("packed", 516, 8, False, 5, 12, 300, [3, 12]),
        "table_K12_D516_s0.5": ("table", 516, 0.5, True, 5, 12, 300, [3, 12]),
        "packed_K12_D520_n4": ("packed", 520, 4, True, 5, 12, 300, [1, 2, 3, 12]),
        "table_K12_D520_nobias": ("table", 520, 1.0, False, 5, 12, 300, [1, 2, 3, 12]),
        "packed_K65_D48_n1_five": ("packed", 48, 1, True, 9, 65, 600, [1, 16, 63, 64, 65]),
        "table_K65_D48_five": ("table", 48, 0.5, True, 9, 65, 600, [1, 16, 63, 64, 65]),
        "packed_K256_D48_n4": ("packed", 48, 4, True, 9, 256, 600, [63, 64, 65, 256]),
        "table_K256_D48": ("table", 48, 1.0, True, 9, 256, 600, [63, 64, 65, 256]),
        "table_K256_D48_k_4k": ("table", 48, 0.5, False, 9, 256, 600, [64, 256]),
        "packed_K12_D48_n8_eight": ("packed", 48, 8, True, 5, 12, 300, [5, 6, 7, 8, 9, 10, 11, 12]),
        "table_K12_D48_eight": ("table", 48, 1.0, True, 5, 12, 300, [5, 6, 7, 8, 9, 10, 11, 12]),
        "table_K256_D48_one": ("table", 48, 0.5, True, 9, 256, 600, [256]),
        "table_split_lists": ("table", 48, 1.0, True, 300, 4, 8, [1, 4]),     # a unit's list passes 256 entries, chunks mix points
    }
    return out


CASES = cases()
#: the subset the host emulation runs (one thread per lane)
EMU_CASES = ["packed_K1_D4_n1", "table_K1_D4", "packed_K7_D48_n4", "table_K12_D516_s0.5", "packed_K12_D520_n4",
             "packed_K65_D48_n1_five", "table_K65_D48_five", "packed_K256_D48_n4", "table_K256_D48_k_4k",
             "packed_K12_D48_n8_eight", "table_K256_D48_one"]
#: the cases whose gradients are driven (table form: the gradient kernels read an fp32 table)
GRAD_CASES = ["table_K1_D4", "table_K7_D48", "table_K12_D516_s0.5", "table_K12_D520_nobias", "table_K65_D48_five",
              "table_K256_D48", "table_K12_D48_eight", "table_K256_D48_one", "table_split_lists"]


def build_case(name: str, outside: bool = False):
    """-> (idx, val, ks, decoder (host form), bias or None).  ``outside``: every row carries an id below 0 and ids at or above
    H (never in the gradient cases of the unit sums, whose lists come from the model's own top-k)."""
    kind, D, par, with_bias, B, K, H, ks = CASES[name]
    seed = 5000 + sorted(CASES).index(name)
    idx, val = ranked_lists(seed + 1, B, K, H)
    if name == "table_split_lists":                         # unit 0 in every row, at a rank that moves: its list holds B entries
        for r in range(B):
            if 0 not in idx[r]:
                idx[r, r % K] = 0
    if outside and K >= 3:
        idx[:, 0] = -3
        idx[:, K // 2] = H + 5
        idx[0, K - 1] = H
    bias = gaussian(seed + 2, 1, D)[0] if with_bias else None
    if kind == "packed":
        decoder = ("packed", packed_dictionary(seed + 3, H, D, par), D, par, 0.25)
    else:
        decoder = ("table", gaussian(seed + 3, H, D), par)
    return np.ascontiguousarray(idx), val, list(ks), decoder, bias


def grad_inputs(name: str):
    """-> dict of the operands of the gradient calls for a table case: idx, val, ks, table, step, g (P x [B, D]), g_latent
    [B, H], W [H, D], x [B, D]"""
    idx, val, ks, decoder, _ = build_case(name)
    B, K = idx.shape
    H, D = decoder[1].shape
    seed = 6000 + sorted(CASES).index(name)
    return {"idx": idx, "val": val, "ks": ks, "table": decoder[1], "step": float(decoder[2]), "B": B, "K": K, "H": H, "D": D,
            "g": [gaussian(seed + 10 + p, B, D) for p in range(len(ks))], "g_latent": gaussian(seed + 1, B, H),
            "W": gaussian(seed + 2, H, D), "x": gaussian(seed + 3, B, D)}
