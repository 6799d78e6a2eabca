"""Shared helpers of the sparsity-curve tests: the numpy restatement of the contract of include/qsae_curve.h.

``prefix_recons``: for every listed k' the CPU oracle's sparse decode (the fmaf chain in ascending unit index, ``* step`` /
``* scale``, ``+ bias``) of the truncated lists ``idx[:, :k']``, ``val[:, :k']``; entries whose id lies outside [0, H) are
dropped from the row's list first (they take part in no chain).  ``prefix_errors``: the fp32 error terms summed in fp64 in the
header's order -- 64 slots of column octets, a butterfly, the rows of a group, the unflagged groups in ascending order onto
the running state."""
from __future__ import annotations

import numpy as np

import oracle
from quantizedsae_amd import synthetic as S

LANES = np.arange(64)


def _decode(idx, val, decoder, bias):
    if decoder[0] == "packed":
        _, packed, D, n_bits, step = decoder
        return oracle.decode_binary(idx, val, packed, D, n_bits, step, bias)
    _, table, scale = decoder
    return oracle.decode_table(idx, val, table, scale, bias)


def dictionary_rows(decoder) -> int:
    return decoder[1].shape[0]


def prefix_recons(idx, val, ks, decoder, bias) -> np.ndarray:
    """-> fp32 [n_ks, B, D].  ``decoder`` = ("packed", packed uint8 [H, row_bytes], D, n_bits, step) or ("table", fp32 [H, D],
    scale), on the host."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float32)
    H = dictionary_rows(decoder)
    B = idx.shape[0]
    inside = (idx >= 0) & (idx < H)
    out = []
    for k in ks:
        if inside[:, :k].all():
            out.append(_decode(idx[:, :k], val[:, :k], decoder, bias))
            continue
        rows = []
        for r in range(B):                                   # ragged: a row at a time, its outside entries dropped
            keep = inside[r, :k]
            rows.append(_decode(idx[r:r + 1, :k][:, keep], val[r:r + 1, :k][:, keep], decoder, bias)[0])
        out.append(np.stack(rows))
    return np.stack(out).astype(np.float32)


def row_sums(recons: np.ndarray, x: np.ndarray) -> np.ndarray:
    """-> fp64 [B, n_ks]: slot s = (d // 8) % 64 adds its terms to 0.0 in ascending d; butterfly xor 32 .. 1; element 0"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, B, D = recons.shape
    with np.errstate(all="ignore"):
        e = (recons - x[None]).astype(np.float32)
        t = (e * e).astype(np.float32).astype(np.float64)            # [n, B, D]
        slots = np.zeros((n, B, 64), dtype=np.float64)
        for d in range(D):
            s = (d // 8) % 64
            slots[:, :, s] = slots[:, :, s] + t[:, :, d]
        for m in (32, 16, 8, 4, 2, 1):
            slots = slots + slots[:, :, LANES ^ m]
    return slots[:, :, 0].T.copy()


def prefix_errors(x, idx, val, ks, decoder, bias, group_rows: int, sums=None, counts=None):
    """-> (sums fp64 [n_ks], counts int64 [2], recons fp32 [n_ks, B, D]); ``sums`` / ``counts``: the running state to continue"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B = x.shape[0]
    sums = np.zeros(len(ks), dtype=np.float64) if sums is None else np.array(sums, dtype=np.float64)
    counts = np.zeros(2, dtype=np.int64) if counts is None else np.array(counts, dtype=np.int64)
    recons = prefix_recons(idx, val, ks, decoder, bias)
    rs = row_sums(recons, x)
    flagged = np.isnan(x).any(axis=1)
    with np.errstate(all="ignore"):
        for r0 in range(0, B, group_rows):
            r1 = min(B, r0 + group_rows)
            if flagged[r0:r1].any():
                counts[1] += r1 - r0
                continue
            counts[0] += r1 - r0
            g = np.zeros(len(ks), dtype=np.float64)
            for r in range(r0, r1):
                g = g + rs[r]
            sums = sums + g
    return sums, counts, recons


# ---- inputs -----------------------------------------------------------------------------------------------------------
def gaussian(seed: int, rows: int, cols: int) -> np.ndarray:
    return S.normal(seed, (rows, cols), stream=53)


def ranked_lists(seed: int, B: int, K: int, H: int):
    """-> (idx int32 [B, K] of distinct ids per row, val fp32 [B, K] descending): a list as the top-k kernels write it"""
    score = S.normal(seed, (B, H), stream=59)
    idx = np.argsort(-score, axis=1, kind="stable")[:, :K].astype(np.int32)
    val = np.take_along_axis(score, idx.astype(np.int64), axis=1).astype(np.float32)
    return np.ascontiguousarray(idx), np.ascontiguousarray(val)


def packed_dictionary(seed: int, H: int, D: int, n_bits: int) -> np.ndarray:
    """packed uint8 [H, row_bytes] of polarised logits"""
    logits = np.where(S.normal(seed, (H, D * n_bits), stream=61) > 0, np.float32(20.0), np.float32(-20.0)).astype(np.float32)
    return oracle.pack_binary(logits, D, n_bits)


def sixteen_points(K: int):
    """up to 16 ascending distinct points in 0 .. K that contain 0 and K"""
    return sorted({int(round(i * K / 15)) for i in range(16)})


#: name -> (kind, D, n_bits or scale, bias?, K, H, ks, B, group_rows): the shapes the emulation and the GPU both run
def cases():
    out = {}
    for D, n in ((48, 4), (4, 1), (36, 3), (512, 4), (512, 8), (1028, 2)):
        out[f"packed_D{D}_n{n}"] = ("packed", D, n, True, 8, 64, [1, 3, 8], 3, 4)
    for D in (4, 36, 512, 1028):
        for scale in (1.0, 0.5):
            for with_bias in (True, False):
                out[f"table_D{D}_s{scale}_b{int(with_bias)}"] = ("table", D, scale, with_bias, 8, 64, [1, 3, 8], 3, 4)
    for K in (1, 64, 65, 256):
        for H in (64, 4096):
            if K <= H:                                       # a row's ids are distinct: no list is longer than the dictionary
                out[f"packed_K{K}_H{H}"] = ("packed", 36, 4, True, K, H, sixteen_points(K), 2, 4)
                out[f"table_K{K}_H{H}"] = ("table", 36, 0.5, True, K, H, sixteen_points(K), 2, 4)
    for kind in ("packed", "table"):
        par = 4 if kind == "packed" else 0.5
        out[f"{kind}_one_point_K"] = (kind, 36, par, True, 8, 64, [8], 3, 4)
        out[f"{kind}_one_point_0"] = (kind, 36, par, True, 8, 64, [0], 3, 4)
        out[f"{kind}_one_point_0_no_bias"] = (kind, 36, par, False, 8, 64, [0], 3, 4)
        out[f"{kind}_B1"] = (kind, 36, par, True, 8, 64, [1, 3, 8], 1, 4)
        out[f"{kind}_B10_nan"] = (kind, 36, par, True, 8, 64, [1, 3, 8], 10, 4)
    return out


CASES = cases()
#: the subset the host emulation runs (one thread per lane: the big shapes take minutes there)
EMU_CASES = ["packed_D48_n4", "packed_D4_n1", "packed_D36_n3", "packed_D1028_n2", "table_D4_s1.0_b1", "table_D36_s0.5_b0",
             "table_D1028_s1.0_b0", "packed_K64_H64", "table_K256_H4096", "packed_one_point_0",
             "table_one_point_0_no_bias", "packed_B10_nan", "table_B10_nan", "packed_D512_n8"]


def build_case(name: str):
    """-> (x, idx, val, ks, decoder (host form), bias or None, group_rows)"""
    kind, D, par, with_bias, K, H, ks, B, group_rows = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    x = gaussian(seed, B, D)
    if name.endswith("_nan"):
        x[B // 2, D // 2] = np.nan                       # one NaN row in the middle group
    idx, val = ranked_lists(seed + 1, B, K, H)
    bias = gaussian(seed + 2, 1, D)[0] if with_bias else None
    if kind == "packed":
        decoder = ("packed", packed_dictionary(seed + 3, H, D, par), D, par, 0.25)
    else:
        decoder = ("table", gaussian(seed + 3, H, D), par)
    return x, idx, val, list(ks), decoder, bias, group_rows


# ---- special values ---------------------------------------------------------------------------------------------------
SPECIAL_CASES = ("values_packed", "values_table", "inf_atom", "packed_ids_outside", "table_ids_outside")


def special_case(name: str):
    """-> (x, idx, val, ks, decoder (host form), bias, group_rows).  values_*: negative, tied and -0.0 values (the list
    position stays the rank); inf_atom: the unit at rank 5 of every row has an inf column; *_ids_outside: an id below 0 and
    one at or above H in every row."""
    B, D, H, K = 6, 36, 64, 8
    seed = 2000 + SPECIAL_CASES.index(name)
    x = gaussian(seed, B, D)
    idx, val = ranked_lists(seed + 1, B, K, H)
    bias = gaussian(seed + 2, 1, D)[0]
    ks = [1, 2, 3, 5, 6, 8]
    if name.endswith("packed") or name.startswith("packed"):
        decoder = ("packed", packed_dictionary(seed + 3, H, D, 4), D, 4, 0.25)
    else:
        decoder = ("table", gaussian(seed + 3, H, D), 0.5)
    if name.startswith("values"):
        val[:, 1] = val[:, 0]                                # tied
        val[:, 2] = -0.0
        val[:, 3] = 0.0
        val[:, 4:] = -np.abs(val[:, 4:]) - 1                 # negative, not ordered
        bias = None
    elif name == "inf_atom":
        table = decoder[1].copy()
        atom = H - 1                                         # the one atom with an inf column: at rank 5 of every row
        for r in range(B):
            idx[r, idx[r] == atom] = idx[r, 5]               # (the ids of a row stay distinct)
            idx[r, 5] = atom
        table[atom, 7] = np.inf
        decoder = ("table", table, 0.5)
    else:
        idx[:, 2] = -3
        idx[:, 6] = H + 5
        idx[0, 0] = H                                        # the first id outside
    return x, idx, val, ks, decoder, bias, 4


def check_special(name: str, case, recons: np.ndarray) -> None:
    """What the case is there to show, on the reconstructions [n_ks, B, D] a run produced."""
    ks = case[3]
    if name == "inf_atom":
        for i, k in enumerate(ks):
            if k <= 5:
                assert np.isfinite(recons[i]).all(), k       # rank 5 takes no part in the chains of k' <= 5
            else:
                assert (~np.isfinite(recons[i])).any(axis=1).all(), k
