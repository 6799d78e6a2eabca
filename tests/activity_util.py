"""What the activity tests share: the numpy restatement of the four entry points of csrc/activity.hip, written from the
definitions of include/qsae.h (not from the kernels), and the builders of the cases the GPU tests run.  Everything is
integer: every comparison with these is exact.

Active: compact entry (r, idx[r][j]) iff val[r][j] > 0 (NaN, 0.0, -0.0 are not; val None: every entry; indices outside
[0, H) dropped; a unit listed twice in a row counts twice); bit form: bit set, through index (-1 = pad, ignored); dense:
latent > 0.  fired[u] += active rows, last[u] = max(last[u], stamp) where the batch has an active row for u.  With clock and
window W: dead = clock - last >= W, never = last == 0, silent = fired == base, interval count c = fired - base, octave bin =
bit length of c with bins above 33 folded into 33.

Importing this module touches no GPU."""
import numpy as np

HEAD, BINS, WORDS, MAX_SEGMENTS = 8, 34, 42, 16
UNITS, NEVER, DEAD, SILENT, SUM_INTERVAL, SUM_FIRED, MAX_INTERVAL = range(7)
SUMMARY_CHUNK = 1024                                   # units of one workgroup of the summary: the workspace holds 4 bytes each
DEAD_POISON = 0x5A5A5A5A


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _mark(fired, last, units, stamp):
    """units: one entry per active (row, unit) pair, repeats included"""
    fired, last = fired.copy(), last.copy()
    if units.size:
        np.add.at(fired, units, 1)
        hit = np.unique(units)
        last[hit] = np.maximum(last[hit], np.int64(stamp))
    return fired, last


def add_compact(idx, val, H, stamp, fired, last):
    idx = np.asarray(idx, np.int64)
    with np.errstate(invalid="ignore"):
        on = np.ones(idx.shape, bool) if val is None else (np.asarray(val, np.float32) > 0)
    on &= (idx >= 0) & (idx < H)
    return _mark(fired, last, idx[on], stamp)


def bits_mask(zbits, nbits):
    """uint32 [B, >= nbits / 32] -> bool [B, nbits]: bit j of word w = position 32 w + j"""
    z = np.asarray(zbits).view(np.uint32)[:, :nbits // 32]
    return ((z[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(z.shape[0], nbits)


def add_bits(zbits, nbits, index, H, stamp, fired, last):
    mask = bits_mask(zbits, nbits)
    unit = np.arange(nbits, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    ok = (unit >= 0) & (unit < H)
    rows, pos = np.nonzero(mask[:, ok])
    return _mark(fired, last, unit[ok][pos], stamp)


def add_dense(latent, H, stamp, fired, last):
    with np.errstate(invalid="ignore"):
        mask = np.asarray(latent, np.float32)[:, :H] > 0
    return _mark(fired, last, np.nonzero(mask)[1].astype(np.int64), stamp)


def octave_bin(c) -> int:
    return min(int(c).bit_length(), BINS - 1)


def summary(fired, base, last, clock, window, seg_sizes=()):
    """-> (result int64 [1 + n_seg, 42], the dead units in ascending order int32)"""
    fired, last = np.asarray(fired, np.int64), np.asarray(last, np.int64)
    base = np.zeros_like(fired) if base is None else np.asarray(base, np.int64)
    H = fired.size
    dead = (np.int64(clock) - last) >= np.int64(window)
    c = fired - base
    bins = np.array([octave_bin(v) for v in c.tolist()], np.int64)
    bounds = [(0, H)]
    at = 0
    for s in seg_sizes:
        bounds.append((at, at + int(s)))
        at += int(s)
    assert not seg_sizes or at == H
    out = np.zeros((len(bounds), WORDS), np.int64)
    for r, (a, b) in enumerate(bounds):
        sl = slice(a, b)
        out[r, UNITS] = b - a
        out[r, NEVER] = int((last[sl] == 0).sum())
        out[r, DEAD] = int(dead[sl].sum())
        out[r, SILENT] = int((c[sl] == 0).sum())
        out[r, SUM_INTERVAL] = int(c[sl].sum())
        out[r, SUM_FIRED] = int(fired[sl].sum())
        out[r, MAX_INTERVAL] = int(c[sl].max()) if b > a else 0
        out[r, HEAD:] = np.bincount(bins[sl], minlength=BINS)
    return out, np.flatnonzero(dead).astype(np.int32)


def workspace_bytes(H: int) -> int:
    if H <= 0:
        return 0
    chunks = (H + SUMMARY_CHUNK - 1) // SUMMARY_CHUNK
    return (chunks * 4 + 255) // 256 * 256


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def compact_case(B, k, H, seed=1, specials=True):
    """idx int32 [B, k], val fp32 [B, k].  With ``specials`` (needs B >= 8, k >= 4): indices -1 and H, val with NaN, +-0.0 and
    negatives, and a unit repeated within a row (both entries active)."""
    g = _rng(seed)
    idx = g.integers(0, H, size=(B, k)).astype(np.int32)
    val = g.standard_normal((B, k)).astype(np.float32)           # about half negative
    if specials:
        idx[0, 0], idx[1, 1], idx[B - 1, k - 1] = -1, H, H
        val[0, 0] = val[1, 1] = val[B - 1, k - 1] = 1.0           # active values on indices that must be dropped
        val[2, 0], val[2, 1], val[2, 2] = np.nan, 0.0, -0.0
        idx[3, 0] = idx[3, 1] = idx[3, 2] = 7 % H
        val[3, 0] = val[3, 1] = 2.0
        val[3, 2] = -1.0
        idx[4, :] = 5 % H                                          # one unit in every slot of a row
        val[4, :] = 1.0
    return idx, val


def bits_case(B, words, words_ld, seed=2, density=0.3):
    """uint32 [B, words_ld] as int32; the columns past ``words`` hold set bits that must not be read as units"""
    g = _rng(seed)
    z = np.zeros((B, words_ld), np.uint32)
    for j in range(32):
        z |= (g.random((B, words_ld)) < density).astype(np.uint32) << np.uint32(j)
    return z.view(np.int32)


def padded_index(nbits, H, seed=3):
    """A permutation of the H units over nbits > H packed positions, -1 on the pad slots"""
    g = _rng(seed)
    index = np.full(nbits, -1, np.int32)
    index[g.permutation(nbits)[:H]] = g.permutation(H).astype(np.int32)
    return index


def dense_case(B, H, ld, seed=4, specials=True):
    """fp32 [B, ld]; the columns past H hold positive values that must not be read.  With ``specials`` (B >= 4, H >= 8): NaN,
    -0.0, +inf, -inf and a positive denormal planted in row 1"""
    g = _rng(seed)
    x = g.standard_normal((B, ld)).astype(np.float32)
    x[:, H:] = 1.0
    if specials:
        x[1, 0], x[1, 1], x[1, 2], x[1, 3] = np.nan, -0.0, np.inf, -np.inf
        x[1, 4] = np.float32(1e-45)
        x[:, 5] = -1.0                                              # a column that never fires
        x[:, H - 1] = 1.0                                           # the last column always does
    return x


def state_case(H, seed=5, clock=5000):
    """(fired, base, last): a third of the units never fired, base <= fired, counts spread over many octaves"""
    g = _rng(seed)
    never = g.random(H) < 0.33
    last = np.where(never, 0, g.integers(1, clock + 1, size=H)).astype(np.int64)
    fired = np.where(never, 0, (2.0 ** g.uniform(0, 20, size=H)).astype(np.int64) + 1).astype(np.int64)
    base = (fired * (g.random(H) < 0.5) * g.random(H)).astype(np.int64)
    silent = g.random(H) < 0.2
    base[silent] = fired[silent]
    return fired, base, last
