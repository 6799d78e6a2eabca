"""What the tests of the slab selection (include/qsae_wide.h) share: the plan of qsaew_slab_plan restated, the order of the
top-k kernels as a numpy key, part lists with the awkward values in them, and the merge restated as one lexsort."""
import numpy as np

MAX_SLABS, MAX_H, MAX_SLAB = 32, 1 << 20, 32768
SENTINEL = np.float32(7.0)                                   # what the dense latent holds where no entry of a part list points
KINDS = ("equal", "straddle", "zeros", "inf", "nan")


def plan(H, k, slab):
    """The starts qsaew_slab_plan documents: walking upwards, a slab takes the remaining units divided by the remaining slabs,
    rounded up to a multiple of 256; the last one the rest.  -> S + 1 starts, or None where it refuses."""
    if H > MAX_H or k > 256 or H % 4 or slab > MAX_SLAB or slab % 256:
        return None
    S = -(-H // slab)
    if S > MAX_SLABS:
        return None
    starts, h0 = [], 0
    for s in range(S):
        rem, parts = H - h0, S - s
        w = rem if parts == 1 else -(-(-(-rem // parts)) // 256) * 256
        if w < k or w > rem:
            return None
        starts.append(h0)
        h0 += w
    return starts + [H]


def mono_key(v):
    """common.h's mono_key: larger value -> larger key, NaN above +inf, -0 equal to +0"""
    v = np.asarray(v, np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    key = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(v), 0xFFFFFFFF, key).astype(np.uint64)


def sort_lists(units, vals):
    """rows of (unit, value) pairs -> both in the kernels' order: key descending, unit ascending"""
    order = np.lexsort((units, -mono_key(vals).astype(np.int64)), axis=-1)
    return np.take_along_axis(units, order, -1), np.take_along_axis(vals, order, -1)


def row_values(kind, rng, S, k):
    """[S, k] values of one row's part lists (before sorting)"""
    if kind == "equal":                                      # all values equal across all parts: the units alone decide
        return np.full((S, k), 1.5, np.float32)
    if kind == "straddle":                                   # few distinct values, so duplicates sit on both sides of every boundary
        return rng.integers(-2, 3, (S, k)).astype(np.float32)
    if kind == "zeros":                                      # +0 and -0 tie; the output keeps each entry's own bits
        v = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), (S, k))
        return v.astype(np.float32)
    if kind == "inf":
        return rng.choice(np.array([np.inf, -np.inf, 3.0, -3.0, 0.0], np.float32), (S, k)).astype(np.float32)
    if kind == "nan":                                        # a NaN row: every value NaN, payloads differ, all keys tie
        bits = (0x7FC00000 + rng.integers(0, 16, (S, k))).astype(np.uint32)
        bits[rng.random((S, k)) < 0.5] |= 0x80000000
        return bits.view(np.float32)
    raise ValueError(kind)


def part_lists(seed, S, B, k, kinds, widths):
    """-> pidx int32, pval fp32 [S, B, k]: row r of kind kinds[r % len(kinds)], k distinct units of every slab, lists sorted"""
    rng = np.random.default_rng(seed)
    pidx = np.empty((S, B, k), np.int32)
    pval = np.empty((S, B, k), np.float32)
    for r in range(B):
        vals = row_values(kinds[r % len(kinds)], rng, S, k)
        for s in range(S):
            units = np.sort(rng.choice(widths[s], k, replace=False)).astype(np.int32)
            pidx[s, r], pval[s, r] = sort_lists(units, vals[s])
    return pidx, pval


def dense_before(pidx, pval, starts, ld):
    """the latent as the slabs' calls leave it for this test: every listed entry's bits in place, SENTINEL everywhere else"""
    S, B, k = pidx.shape
    dense = np.full((B, ld), SENTINEL, np.float32)
    for s in range(S):
        for r in range(B):
            dense[r, starts[s] + pidx[s, r]] = pval[s, r]
    return dense


def merge_ref(pidx, pval, starts, dense=None):
    """-> (idx, val [B, k], dense after or None): lexsort by key descending, global unit ascending; the losers' elements +0"""
    S, B, k = pidx.shape
    units = np.concatenate([pidx[s].astype(np.int64) + starts[s] for s in range(S)], axis=1)         # [B, S k]
    vals = np.concatenate([pval[s] for s in range(S)], axis=1)
    su, sv = sort_lists(units, vals)
    out = None
    if dense is not None:
        out = dense.copy()
        for r in range(B):
            out[r, su[r, k:]] = np.float32(0.0)
    return su[:, :k].astype(np.int32), sv[:, :k], out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
