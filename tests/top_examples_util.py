"""numpy restatement of the streaming top-n lists per feature (csrc/top_examples.hip) and the planted test data that the
host, emulator and GPU tests share.

State: keys uint64 [H, n], every row descending and 0-padded.  A candidate of feature h is (value, position) with
value > floor; its key is full_key(value, position): the order-preserving bits of the fp32 value << 32 | ~position.
After any number of updates keys[h] is the n largest keys among all candidates of h: collect them, lexsort by (feature,
key descending), take the first n per feature.  Every comparison against this is exact."""
import numpy as np

MAX_N = 64


def mono_key(v):
    """float32 -> uint32, larger float -> larger key; -0 as +0 (common.h mono_key; NaN never reaches it here)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def full_key(values, positions):
    pos = np.asarray(positions, np.uint64)
    assert (pos < (1 << 32)).all()
    return (mono_key(values).astype(np.uint64) << np.uint64(32)) | (~pos & np.uint64(0xFFFFFFFF))


def key_value(keys):
    m = (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.where(m & 0x80000000, m ^ np.uint32(0x80000000), ~m).astype(np.uint32).view(np.float32)


def key_position(keys):
    return (~np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def candidates_compact(idx, val, H, base=0, floor=0.0):
    """-> (features int64, keys uint64) of every candidate of a compact batch; val None = every entry at 1.0."""
    idx = np.asarray(idx, np.int64)
    B, k = idx.shape
    v = np.ones((B, k), np.float32) if val is None else np.asarray(val, np.float32)
    rows = np.broadcast_to(np.arange(B, dtype=np.int64)[:, None], (B, k))
    with np.errstate(invalid="ignore"):
        ok = (idx >= 0) & (idx < H) & (v > np.float32(floor))
    return idx[ok], full_key(v[ok], rows[ok] + int(base))


def candidates_dense(latent, H, base=0, floor=0.0):
    lat = np.asarray(latent, np.float32)[:, :H]
    with np.errstate(invalid="ignore"):
        r, f = np.nonzero(lat > np.float32(floor))
    return f.astype(np.int64), full_key(lat[r, f], r.astype(np.int64) + int(base))


def restate(H, n, feats, keys, old=None):
    """The n largest keys per feature of the candidates (feats, keys), joined with a previous state `old` [H, n]."""
    feats, keys = np.asarray(feats, np.int64), np.asarray(keys, np.uint64)
    if old is not None:
        f, j = np.nonzero(np.asarray(old, np.uint64) != 0)
        feats, keys = np.concatenate([feats, f]), np.concatenate([keys, np.asarray(old, np.uint64)[f, j]])
    out = np.zeros((H, n), np.uint64)
    if feats.size == 0:
        return out
    order = np.lexsort((~keys, feats))                         # feature ascending, key descending
    feats, keys = feats[order], keys[order]
    start = np.searchsorted(feats, feats, side="left")         # index of the first entry of this entry's feature
    rank = np.arange(feats.size) - start
    keep = rank < n
    out[feats[keep], rank[keep]] = keys[keep]
    return out


def restate_loop(H, n, triples, floor=0.0):
    """Brute force over (feature, value, position) triples, for tiny inputs: python sort per feature."""
    out = np.zeros((H, n), np.uint64)
    for h in range(H):
        mine = [(np.float32(v), int(p)) for f, v, p in triples if f == h and np.float32(v) > np.float32(floor)]
        mine.sort(key=lambda vp: (-float(vp[0]), vp[1]))
        for j, (v, p) in enumerate(mine[:n]):
            out[h, j] = full_key(np.array([v], np.float32), np.array([p]))[0]
    return out


def decode(keys):
    keys = np.asarray(keys, np.uint64)
    none = keys == 0
    return (np.where(none, np.float32(0), key_value(keys)).astype(np.float32), np.where(none, -1, key_position(keys)),
            (~none).sum(1).astype(np.int32))


# (B, k, H, n) of the compact cases and (B, H, ld, n) of the dense cases
COMPACT_CASES = [(1, 1, 32, 1), (37, 5, 33, 3), (130, 2, 4, 64), (300, 65, 1024, 16), (2100, 3, 64, 64)]
DENSE_CASES = [(1, 1, 4, 1), (65, 129, 132, 4), (193, 128, 128, 10), (200, 300, 304, 64)]


def compact_case(seed, B, k, H):
    """idx int32 [B, k], val float32 [B, k] with distinct units per row and, as far as the shape has room:
    unit 0 in every row with values ascending in the row (every candidate passes a threshold filter); unit 1 in every
    third row with descending values; unit 2 in every third row always at 0.5 (equal values: the lower position wins);
    unit H - 1 in no row; random units of 3 .. H - 2 elsewhere; 0.0, -0.0, NaN and a negative value planted in columns
    >= 1; indices outside [0, H) planted in columns >= 1 and wherever a random draw repeated a unit of its row."""
    rng = np.random.default_rng(seed)
    idx = np.full((B, k), -1, np.int64)
    val = (np.abs(rng.standard_normal((B, k))) + 1e-3).astype(np.float32)
    r = np.arange(B)
    idx[:, 0] = 0
    val[:, 0] = np.float32(1.0) + r.astype(np.float32) * np.float32(2.0 ** -10)
    if k >= 2 and H >= 3:
        idx[r % 3 == 0, 1] = 1
        val[:, 1] = np.float32(100.0) - r.astype(np.float32) * np.float32(2.0 ** -10)
        if H >= 4:
            idx[r % 3 == 1, 1] = 2
            val[r % 3 == 1, 1] = 0.5
    if k >= 3 and H >= 6:
        draw = np.sort(rng.integers(3, H - 1, size=(B, k - 2)), axis=1)
        draw[:, 1:][draw[:, 1:] == draw[:, :-1]] = H + 7        # a repeated unit becomes an out-of-range index
        idx[:, 2:] = draw
    if k >= 2:
        def spots(m):
            return rng.integers(0, B, size=m), rng.integers(1, k, size=m)
        m = max(1, B // 16)
        for special in (0.0, -0.0, np.nan, -1.5):
            val[spots(m)] = np.float32(special)
        for bad in (-1, H, H + 5, 2 ** 31 - 1, -2 ** 31):
            idx[spots(m)] = bad
    return idx.astype(np.int32), val


def dense_case(seed, B, H, ld):
    """latent float32 [B, ld]: ReLU of a Gaussian (about half zeros) with NaN at and past H in every row; column 0 ascends
    with the row, column 1 descends, column 2 is constant, column H - 1 is entirely <= 0; NaN, -0.0 and negatives planted."""
    rng = np.random.default_rng(seed)
    lat = np.maximum(rng.standard_normal((B, ld)), 0).astype(np.float32)
    r = np.arange(B, dtype=np.float32)
    lat[:, 0] = np.float32(1.0) + r * np.float32(2.0 ** -10)
    if H >= 2:
        lat[:, H - 1] = -np.abs(lat[:, H - 1])
    if H >= 4:
        lat[:, 1] = np.float32(100.0) - r * np.float32(2.0 ** -10)
        lat[:, 2] = 0.75
        m = max(1, B // 8)
        for special in (-0.0, np.nan, -2.0):
            lat[rng.integers(0, B, size=m), rng.integers(3, H, size=m)] = np.float32(special)
    lat[:, H:] = np.nan
    return lat


def splits(B, parts):
    """`parts` uneven batch boundaries over B rows that include a batch of one row: [0, ..., B]."""
    if B < parts:
        return list(range(B + 1))
    cuts = {0, B, 1}                                            # the first batch has one row
    step = B / (parts - 1)
    for i in range(1, parts - 1):
        cuts.add(min(B, max(1, int(round(i * step * (0.8 if i % 2 else 1.15))))))
    return sorted(cuts)
