"""Shared helpers of the tests of the nested levels over ragged rows: the numpy restatement of the contract of
include/qsae_nested_batch.h, put together from the two restatements it joins.

``nested_recons``: ``nested_util.nested_recons`` per group of rows of equal ``c(r)`` on the lists truncated to ``c(r)`` entries.
``counts_below``: the kept entries (in the prefix, id in [0, H)) of every row below every bound, from the ids.  ``row_grad``:
``nested_util.suffix_sums`` and, per entry of a prefix, the arithmetic of ``batch_topk_util.row_grad_ragged`` with
``g_recon = G[level(unit)]``.  The inputs are those of ``batch_topk_util`` (``ragged_case`` where it has the shape, the same
generators where it has not, ``count_patterns``) with bounds over H = 512 and ids planted so that what the levels and the
prefixes are there to separate is in the inputs, not left to luck."""
from __future__ import annotations

import numpy as np

import nested_util as N
import oracle
from batch_topk_util import RAGGED_CASES, _lane_columns, clamp_counts, count_patterns, ragged_case
from sparsity_curve_util import gaussian, packed_dictionary, ranked_lists

__all__ = ["nested_recons", "counts_below", "row_grad", "BOUNDS", "EIGHT", "CASES", "EMU_CASES", "build_case", "patterns",
           "planted_facts", "special_case", "SPECIAL_CASES"]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def nested_recons(idx, val, counts, bounds, decoder, bias) -> np.ndarray:
    """-> fp32 [L, B, D]: level l of row r is the oracle's sparse decode of the row's first c(r) entries with the entries of
    units >= bounds[l], and those whose id lies outside [0, H), removed.  ``decoder`` as in nested_util.nested_recons."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float32)
    B, K = idx.shape
    D = decoder[2] if decoder[0] == "packed" else decoder[1].shape[1]
    c = clamp_counts(counts, K)
    out = np.empty((len(bounds), B, D), dtype=np.float32)
    for n in np.unique(c):
        rows = np.nonzero(c == n)[0]
        if n == 0:                                           # a chain of +0 through the two roundings: the bias, or +0
            out[:, rows] = np.float32(0) + (bias if bias is not None else np.zeros(D, np.float32))
            continue
        out[:, rows] = N.nested_recons(idx[rows, :n], val[rows, :n], bounds, decoder, bias)
    return out


def counts_below(idx, counts, bounds, H: int) -> np.ndarray:
    """-> int32 [L, B]"""
    idx = np.asarray(idx, dtype=np.int64)
    B, K = idx.shape
    c = clamp_counts(counts, K)
    kept = (np.arange(K)[None, :] < c[:, None]) & (idx >= 0) & (idx < H)
    return np.stack([(kept & (idx < b)).sum(axis=1) for b in bounds]).astype(np.int32)


def row_grad(idx, counts, table, step, g_levels, bounds, g_latent, W_enc):
    """-> (G fp32 [L, B, D], gv fp32 [B, K], dx fp32 [B, D] or None) in the kernels' order of operations: G as suffix_sums; per
    entry of a prefix (id clamped into [0, H)) the 64 lanes' fmaf chains over their own columns of G[level(h)][r] and
    table[h], a butterfly of fp32 adds, ``step *`` and ``g_latent +`` rounded one by one; dx per column one fmaf chain over the
    prefix in list order.  gv behind the prefix is +0."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.float32)
    B, K = idx.shape
    H, D = table.shape
    G = N.suffix_sums(g_levels, B, D)
    c = clamp_counts(counts, K)
    hh = np.clip(idx, 0, H - 1)
    lev = np.minimum(N.levels_of(hh, bounds), len(bounds) - 1)
    cols = _lane_columns(D)
    width = max(1, max(len(x) for x in cols))
    lanes = np.arange(64)
    gv = np.zeros((B, K), dtype=np.float32)
    dx = np.zeros((B, D), dtype=np.float32) if W_enc is not None else None
    step = np.float32(step)
    for r in range(B):
        for j in range(int(c[r])):
            h = int(hh[r, j])
            a = np.zeros((64, width), dtype=np.float32)       # padding: fmaf(0, 0, acc) leaves acc (never -0) as it is
            t = np.zeros((64, width), dtype=np.float32)
            for l in range(64):
                a[l, :len(cols[l])] = G[lev[r, j], r, cols[l]]
                t[l, :len(cols[l])] = table[h, cols[l]]
            part = np.diagonal(oracle.encode(a, t)).astype(np.float32)
            for off in (32, 16, 8, 4, 2, 1):
                part = (part + part[lanes ^ off]).astype(np.float32)
            v = np.float32(step * part[0])
            if g_latent is not None:
                v = np.float32(np.float32(g_latent[r, h]) + v)
            gv[r, j] = v
        if dx is not None and c[r] > 0:
            n = int(c[r])
            dx[r] = oracle.encode(gv[r:r + 1, :n], np.ascontiguousarray(np.asarray(W_enc, dtype=np.float32)[hh[r, :n]].T))[0]
    return G, gv, dx


# ---- inputs -------------------------------------------------------------------------------------------------------------
H = 512
BOUNDS = [1, 33, 64, 512]
EIGHT = [1, 2, 5, 33, 64, 100, 256, 512]
ONE = [512]

#: name -> (decoder kind, D, n_bits or scale, bias, B, K, bounds).  The first block is batch_topk_util.RAGGED_CASES at H = 512;
#: the second adds what that table has not: B = 1, K in {1, 7, 65}, D = 520, one and eight levels.
CASES = {name: RAGGED_CASES[name][:6] + (BOUNDS,) for name in sorted(RAGGED_CASES) if RAGGED_CASES[name][6] == H}
CASES.update({
    "table_D520_s0.5_nobias_B5_K65": ("table", 520, 0.5, False, 5, 65, BOUNDS),
    "packed_D520_n4_B1_K7_one_level": ("packed", 520, 4, True, 1, 7, ONE),
    "table_D48_B1_K1_eight_levels": ("table", 48, 1.0, True, 1, 1, EIGHT),
    "packed_D48_n8_nobias_B9_K12_eight_levels": ("packed", 48, 8, False, 9, 12, EIGHT),
    "table_D4_s0.5_B5_K7_one_level": ("table", 4, 0.5, True, 5, 7, ONE),
    "packed_D516_n1_B5_K65_eight_levels": ("packed", 516, 1, True, 5, 65, EIGHT),
    "table_D516_s0.5_B5_K7": ("table", 516, 0.5, True, 5, 7, BOUNDS),
})
#: the subset the host emulation runs (one thread per lane)
EMU_CASES = ["packed_D4_n1", "packed_D48_n4", "packed_D516_n8", "table_D516", "table_D48_K256", "packed_D48_n4_K256",
             "table_D520_s0.5_nobias_B5_K65", "packed_D520_n4_B1_K7_one_level", "table_D48_B1_K1_eight_levels",
             "packed_D48_n8_nobias_B9_K12_eight_levels"]

#: the planted rows of a case with B = 9, K = 12, and their prefix lengths under the pattern "mixed"
ROW_UNIT0_INSIDE, ROW_UNIT0_BEHIND, ROW_EMPTY_LEVEL, ROW_ALL_OUTSIDE = 2, 3, 4, 6
EMPTY_LEVEL = 1                                              # [bounds[0], bounds[1]) of the planted row holds no prefix entry


def _free(row, lo: int, n: int):
    taken = set(int(h) for h in row)
    return [h for h in range(H - 1, lo - 1, -1) if h not in taken][:n]


def _plant(idx, bounds):
    """B = 9, K = 12 under "mixed" = [0, 1, 11, 3, 8, 0, 5, 10, 12]: unit 0 inside the prefix of row 2 and just behind that of
    row 3; no prefix entry of row 4 in the second level; every prefix id of row 6 outside [0, H)."""
    mixed = clamp_counts(count_patterns(9, 12)["mixed"], 12)
    for r in (ROW_UNIT0_INSIDE, ROW_UNIT0_BEHIND):           # unit 0 nowhere else in these rows
        zero = idx[r] == 0
        idx[r, zero] = _free(idx[r], 64, int(zero.sum()))
    idx[ROW_UNIT0_INSIDE, 0] = 0
    idx[ROW_UNIT0_BEHIND, mixed[ROW_UNIT0_BEHIND]] = 0
    if len(bounds) > 2:
        r, n = ROW_EMPTY_LEVEL, int(mixed[ROW_EMPTY_LEVEL])
        inside = np.zeros(12, dtype=bool)
        inside[:n] = (idx[r, :n] >= bounds[EMPTY_LEVEL - 1]) & (idx[r, :n] < bounds[EMPTY_LEVEL])
        idx[r, inside] = _free(idx[r], bounds[-2], int(inside.sum()))
        twin = idx[r] == bounds[EMPTY_LEVEL]
        idx[r, twin] = _free(idx[r], bounds[-2], int(twin.sum()))
        idx[r, 0] = bounds[EMPTY_LEVEL]                       # ... and the level after it is not empty
    n = int(mixed[ROW_ALL_OUTSIDE])
    idx[ROW_ALL_OUTSIDE, :n] = [(-1 - j) if j % 2 == 0 else (H + j) for j in range(n)]
    return idx


def build_case(name: str):
    """-> (idx, val, bounds, decoder (host form), bias or None).  Row 0 holds an id below 0 and one at H (K >= 4); the cases
    with B = 9, K = 12 carry the planted rows."""
    kind, D, par, with_bias, B, K, bounds = CASES[name]
    if name in RAGGED_CASES:
        idx, val, decoder, bias, _ = ragged_case(name)
    else:
        seed = 7000 + sorted(CASES).index(name)
        idx, val = ranked_lists(seed + 1, B, K, H)
        if K >= 4:
            idx[0, 1], idx[0, 2] = -2, H
        bias = gaussian(seed + 2, 1, D)[0] if with_bias else None
        decoder = ("packed", packed_dictionary(seed + 3, H, D, par), D, par, 0.25) if kind == "packed" \
            else ("table", gaussian(seed + 3, H, D), par)
    idx = np.ascontiguousarray(idx).copy()
    if (B, K) == (9, 12):
        idx = _plant(idx, bounds)
    return idx, np.ascontiguousarray(val), list(bounds), decoder, bias


def patterns(B: int, K: int):
    """count_patterns, and at K = 256 one more: prefixes of 63, 64 and 65 entries (one, one and two rounds of the rank pass)"""
    out = dict(count_patterns(B, K))
    if K == 256 and B >= 3:
        c = out["mixed"].copy()
        c[:3] = (63, 64, 65)
        out["around_64"] = c
    return out


def planted_facts(name: str):
    """The coverage the planted rows give, from the inputs alone -> dict of bools"""
    idx, _, bounds, _, _ = build_case(name)
    B, K = idx.shape
    c = clamp_counts(count_patterns(B, K)["mixed"], K)
    below = counts_below(idx, c, bounds, H)
    r_in, r_out, r_mid, r_all = ROW_UNIT0_INSIDE, ROW_UNIT0_BEHIND, ROW_EMPTY_LEVEL, ROW_ALL_OUTSIDE
    facts = {
        "unit 0 inside a prefix": 0 in idx[r_in, :c[r_in]] and below[0, r_in] == 1,
        "unit 0 just behind a prefix": idx[r_out, c[r_out]] == 0 and 0 not in idx[r_out, :c[r_out]] and below[0, r_out] == 0,
        "a prefix with ids all outside": c[r_all] > 0 and bool(((idx[r_all, :c[r_all]] < 0) | (idx[r_all, :c[r_all]] >= H)).all())
        and below[-1, r_all] == 0,
        "ids of a row are distinct": all(len(set(idx[r].tolist())) == K for r in (r_in, r_out, r_mid)),
    }
    if len(bounds) > 2:
        facts["a middle level without a prefix entry"] = (below[EMPTY_LEVEL, r_mid] == below[EMPTY_LEVEL - 1, r_mid]
                                                          and below[EMPTY_LEVEL + 1, r_mid] > below[EMPTY_LEVEL, r_mid])
    return facts


# ---- special values -------------------------------------------------------------------------------------------------------
SPECIAL_CASES = ("behind_a_prefix", "behind_a_bound", "minus_zero")
SPECIAL_BOUNDS = [8, 32, 64]
SPECIAL_COUNTS = np.array([3, 5, 0, 8], dtype=np.int32)


def special_case(name: str):
    """-> (idx, val, counts, bounds, decoder (host form), bias, check).  B = 4, K = 8, H = 64, D = 36, a table at scale 0.5.
    behind_a_prefix: every unit no prefix holds has an inf row with a NaN column, and val behind the prefixes is inf / NaN;
    behind_a_bound: within the prefixes, the units of the last level have such rows and values -- no earlier level may show
    them; minus_zero: the values of row 0 are all +-0 under a negative scale and no bias -- +0 at every level, never -0.
    ``check(levels)`` asserts what the case is there to show."""
    B, D, Hs, K = 4, 36, 64, 8
    seed = 8000 + SPECIAL_CASES.index(name)
    idx, val = ranked_lists(seed + 1, B, K, Hs)
    val = val.copy()
    bias = gaussian(seed + 2, 1, D)[0]
    table = gaussian(seed + 3, Hs, D)
    counts, bounds, scale = SPECIAL_COUNTS.copy(), list(SPECIAL_BOUNDS), 0.5
    pre = np.arange(K)[None, :] < counts[:, None]
    if name == "behind_a_prefix":
        front = np.zeros(Hs, dtype=bool)
        front[idx[pre]] = True
        table[~front] = np.inf
        table[~front, 5] = np.nan
        val[~pre] = np.resize(np.array([np.inf, np.nan, -np.inf], np.float32), int((~pre).sum()))

        def check(levels):
            assert np.isfinite(levels).all()
    elif name == "behind_a_bound":
        last = pre & (idx >= bounds[-2])
        for r in (0, 1, 3):                                   # every prefix reaches into the last level
            if not last[r].any():
                idx[r, 0] = bounds[-2] + r
        last = pre & (idx >= bounds[-2])
        units = np.unique(idx[last])
        for r in range(B):                                    # those units stay in the last level's entries only
            assert not np.isin(idx[r][idx[r] < bounds[-2]], units).any()
        table[units] = np.inf
        table[units, 5] = np.nan
        val[last] = np.inf

        def check(levels):
            assert np.isfinite(levels[:-1]).all()
            assert (~np.isfinite(levels[-1][[0, 1, 3]])).any(axis=1).all() and np.isfinite(levels[-1][2]).all()
    elif name == "minus_zero":
        counts[0] = 6
        val[0, 0::2], val[0, 1::2] = -0.0, 0.0
        scale, bias = -0.5, None

        def check(levels):
            assert not levels[:, 0].view(np.uint32).any()
            assert not levels[:, 2].view(np.uint32).any()     # the empty row
    else:
        raise ValueError(name)
    return np.ascontiguousarray(idx), val, counts, bounds, ("table", table, scale), bias, check
