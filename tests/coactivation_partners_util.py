"""Shared by the co-activation partner tests and tools/gen_golden_coactivation_summary.py: inputs, expectations and the
portable recipes of the summary goldens.

Inputs: AND of s independent fair streams (density 2^-s) with s = max(1, round(log2(B) / 2)), so that a pair of
positions co-activates somewhere in a batch of B rows with probability 1 - (1 - 4^-s)^B: between 0.25 (B = 1) and 0.76
(B = 5), about 0.63 when B is a power of four.  Fair bits would make every pair co-active, and a kernel that writes all
ones would pass; every kernel test therefore asserts ``check_density``.
"""
import math

import numpy as np

import oracle
from quantizedsae_amd import synthetic as S

GOLDEN_PREFIX = "coactivation_summary_"


def streams(B):
    return max(1, round(math.log2(B) / 2)) if B > 1 else 1


def make_bits(seed, B, n, s=None):
    """uint8 0/1 [B, n] of density 2^-s"""
    s = streams(B) if s is None else s
    bits = S.fair_bits(seed, (B, n))
    for i in range(1, s):
        bits = bits & S.fair_bits(seed, (B, n), stream=i)
    return bits


def pack(bits):
    """uint8 0/1 [B, 32 * words] -> int32 [B, words], bit j of word w = position 32 w + j"""
    return np.packbits(bits, axis=1, bitorder="little").view(np.int32)


def unit_mask(bits, index, H):
    """the [B, H] mask the packed bits stand for: position p is unit index[p], -1 = pad slot (dropped)"""
    if index is None:
        return bits[:, :H].astype(bool)
    mask = np.zeros((bits.shape[0], H), bool)
    valid = index >= 0
    mask[:, index[valid]] = bits[:, valid].astype(bool)
    return mask


def expected_dense(mask):
    """bool [H, H]: the pair was active in the same row at least once (diagonal: the unit was active at all)"""
    mask = np.asarray(mask, bool)
    if mask.shape[0] * mask.shape[1] ** 2 <= 1 << 27:
        return oracle.activation_stats(mask)[1] > 0
    assert mask.shape[0] < 1 << 24                              # fp32 counts <= B are exact
    m = mask.astype(np.float32)
    return (m.T @ m) > 0


def expected_counts(dense):
    """int64 [H]: partners of each unit, itself excluded"""
    dense = np.asarray(dense, bool)
    return dense.sum(axis=1).astype(np.int64) - np.diagonal(dense).astype(np.int64)


def check_density(dense):
    """between 10 % and 90 % of the off-diagonal pairs are set: neither all zeros nor all ones can pass"""
    dense = np.asarray(dense, bool)
    H = dense.shape[0]
    if H < 2:
        return
    share = (dense.sum() - np.diagonal(dense).sum()) / (H * (H - 1))
    assert 0.1 <= share <= 0.9, f"off-diagonal share {share:.3f} outside [0.1, 0.9]"


# ---- summary goldens --------------------------------------------------------------------------------------------------
# B <= 256, H <= 192.  dead: features that never fire; lonely: a feature that fires only in rows where nothing else
# does (active, no partner); row_mask: a selection of rows for one extra average.
RECIPES = {
    "levels3": dict(seed=41, B=200, H=192, s=4, sizes=[32, 64, 96], threshold=9, lonely=70, lonely_rows=5,
                    dead=list(range(3, 32)) + [40, 41, 100, 191], row_mask=list(range(20, 120, 3))),
    "single": dict(seed=43, B=100, H=96, s=3, sizes=[96], threshold=1, lonely=None, lonely_rows=0,
                   dead=[0, 17, 95], row_mask=list(range(0, 96, 2))),
    "nothing_active": dict(seed=47, B=16, H=64, s=0, sizes=[32, 32], threshold=1, lonely=None, lonely_rows=0,
                           dead=list(range(64)), row_mask=list(range(10, 30))),
    "dead_selection": dict(seed=53, B=64, H=64, s=3, sizes=[16, 48], threshold=2, lonely=None, lonely_rows=0,
                           dead=list(range(16)) + [33], row_mask=list(range(16))),
}


def summary_mask(recipe):
    """bool [B, H] of a recipe"""
    B, H = recipe["B"], recipe["H"]
    mask = make_bits(recipe["seed"], B, H, recipe["s"]).astype(bool) if recipe["s"] else np.zeros((B, H), bool)
    if recipe["lonely"] is not None:
        rows = np.arange(recipe["lonely_rows"]) * 7 + 1
        mask[:, recipe["lonely"]] = False
        mask[rows, :] = False
        mask[rows, recipe["lonely"]] = True
    mask[:, recipe["dead"]] = False
    return mask


def level_slices(sizes):
    start = 0
    for size in sizes:
        yield slice(start, start + int(size))
        start += int(size)


# ---- compact rows of the top-k models --------------------------------------------------------------------------------
def compact_rows(seed, B, k, H):
    """(idx int32 [B, k], val fp32 [B, k], mask bool [B, H]) with k <= H: every row lists k minus a few distinct active
    units (val > 0) in shuffled slots; the other slots hold what must not count -- val 0.0, -0.0, NaN or negative on
    a valid unit, indices -1, H and H + 1000 with a positive val -- or, counting once, an active unit a second time."""
    assert k <= H
    rng = np.random.default_rng(seed)
    idx = np.empty((B, k), np.int32)
    val = np.empty((B, k), np.float32)
    mask = np.zeros((B, H), bool)
    dead_val = np.array([0.0, -0.0, np.nan, -1.5], np.float32)
    for b in range(B):
        junk = int(rng.integers(0, min(k, 8) + (k == 1)))
        act = rng.choice(H, size=k - junk, replace=False)
        mask[b, act] = True
        row_i = np.concatenate([act, np.zeros(junk, np.int64)])
        row_v = np.concatenate([rng.uniform(0.1, 2.0, k - junk), np.zeros(junk)]).astype(np.float32)
        for j in range(junk):
            kind = (b + j) % 8
            s = k - junk + j
            if kind < 4:
                row_i[s], row_v[s] = rng.integers(0, H), dead_val[kind]
            elif kind < 7:
                row_i[s], row_v[s] = (-1, H, H + 1000)[kind - 4], 1.0
            elif len(act):
                row_i[s], row_v[s] = act[j % len(act)], 0.5
            else:
                row_i[s], row_v[s] = -1, 1.0
        order = rng.permutation(k)
        idx[b], val[b] = row_i[order], row_v[order]
    return idx, val, mask
