"""The numpy restatement of include/qsae_jump.h, written from the header: the two predicates, the two stable partitions, the
report, l0, theta_min, the certificate of a row, and the thresholds' pseudo-gradient.  Shared by tests/test_jumprelu_host.py and
tests/test_jumprelu_gpu.py; no GPU, no library."""
import numpy as np

REPORT_WORDS = 6
QUIET_NAN_BITS = 0x7FC00000


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def half_eps(eps):
    """fl32(0.5f * eps)"""
    return np.float32(np.float32(0.5) * np.float32(eps))


def theta_min(theta):
    """The smallest threshold under a float <, NaN skipped; of -0 and +0 the -0; the quiet NaN when all are NaN"""
    theta = np.asarray(theta, dtype=np.float32)
    best = None
    for t in theta:
        if np.isnan(t):
            continue
        if best is None or t < best or (t == best and np.signbit(t) and not np.signbit(best)):
            best = t
    return np.uint32(QUIET_NAN_BITS).view(np.float32) if best is None else np.float32(best)


def predicates(idx, val, theta, eps):
    """-> (selected, in the band), two bool [B, K]"""
    idx, val, theta = np.asarray(idx, np.int32), np.asarray(val, np.float32), np.asarray(theta, np.float32)
    H = theta.shape[0]
    ok = (idx >= 0) & (idx < H)
    th = theta[np.where(ok, idx, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        sel = ok & (val > th)                                  # NaN on either side: False
        d = (val - th).astype(np.float32)                      # one fp32 subtraction
        band = ok & (np.abs(d) < half_eps(eps))
    return sel, band


def stable_partition(idx, val, keep):
    """-> (idx_p, val_p or None, counts): the kept entries of every row first, in list order, then the others, in list order;
    val_p is +0 behind the kept ones"""
    B, K = idx.shape
    idx_p = np.empty_like(idx)
    val_p = None if val is None else np.zeros((B, K), np.float32)
    counts = keep.sum(axis=1).astype(np.int32)
    for r in range(B):
        order = np.concatenate([np.flatnonzero(keep[r]), np.flatnonzero(~keep[r])])
        idx_p[r] = idx[r, order]
        if val is not None:
            val_p[r, :counts[r]] = val[r, order[:counts[r]]]
    return idx_p, val_p, counts


def jump_select(idx, val, theta, eps):
    """-> (idx_sel, val_sel, counts, idx_band, counts_band, l0 fp32, report int64 [6]) of qsaej_jump_select"""
    idx, val, theta = np.asarray(idx, np.int32), np.asarray(val, np.float32), np.asarray(theta, np.float32)
    B, K = idx.shape
    H = theta.shape[0]
    sel, band = predicates(idx, val, theta, eps)
    idx_sel, val_sel, counts = stable_partition(idx, val, sel)
    idx_band, _, counts_band = stable_partition(idx, None, band)
    tmin = theta_min(theta)
    with np.errstate(invalid="ignore", over="ignore"):
        bound = np.float32(tmin - half_eps(eps))
        certified = val[:, K - 1] < bound
    uncertified = int((~certified).sum()) if K < H else 0
    selected = int(counts.sum())
    report = np.array([selected, int(counts_band.sum()), int((counts == K).sum()), int((counts == 0).sum()), uncertified,
                       int(bits(np.array([tmin], np.float32))[0])], dtype=np.int64)
    l0 = np.float32(np.float64(selected) / np.float64(B))
    return idx_sel, val_sel, counts, idx_band, counts_band, l0, report


def threshold_grad(offsets, entries, gv_band, theta, g_l0, B, eps):
    """-> dtheta fp32 [H] of qsaej_threshold_grad: fp64, left to right, one rounding"""
    theta = np.asarray(theta, np.float32)
    H = theta.shape[0]
    gv = None if gv_band is None else np.asarray(gv_band, np.float32).reshape(-1)
    out = np.zeros((H,), np.float32)
    with np.errstate(all="ignore"):
        for h in range(H):
            beg, end = int(offsets[h]), int(offsets[h + 1])
            n = end - beg
            if n == 0:
                continue
            S = np.float64(0.0)
            if gv is not None:
                for e in entries[beg:end]:
                    S = S + np.float64(gv[e])
            a = np.float64(theta[h]) * S
            g = np.float64(0.0) if g_l0 is None else np.float64(np.float32(g_l0))
            b = g * np.float64(n) / np.float64(B)
            t = -(a + b)
            out[h] = np.float32(t / np.float64(np.float32(eps)))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def lists(B, K, H, seed):
    """Top-K-like lists: distinct ids per row where H allows (ids repeat when K > H), values non-increasing"""
    rng = np.random.default_rng(seed)
    idx = np.empty((B, K), np.int32)
    for r in range(B):
        idx[r] = rng.permutation(H)[:K] if K <= H else rng.integers(0, H, K)
    val = -np.sort(-rng.standard_normal((B, K)).astype(np.float32), axis=1)
    return idx, np.ascontiguousarray(val)


def case(kind, B, K, H, seed=0, eps=0.25):
    """-> (idx, val, theta, eps) of a named value pattern"""
    idx, val = lists(B, K, H, seed + 17 * B + K)
    rng = np.random.default_rng(seed + 1000)
    theta = np.abs(rng.standard_normal(H)).astype(np.float32) * np.float32(0.5) + np.float32(0.05)
    if kind == "all":
        theta = np.full(H, -np.inf, np.float32)
    elif kind == "none":
        theta = np.full(H, np.inf, np.float32)
    elif kind == "mixed":
        pass
    elif kind == "special":
        theta, val, idx = theta.copy(), val.copy(), idx.copy()
        flat_v, flat_i = val.reshape(-1), idx.reshape(-1)
        n = flat_v.size
        he = half_eps(eps)
        for t, e in enumerate(rng.permutation(n)[:max(1, n // 2)]):
            h = flat_i[e]
            th = theta[h]
            m = t % 9
            if m == 0:
                flat_v[e] = th                                 # equal: not selected, in the band
            elif m == 1:
                flat_v[e] = np.nan
            elif m == 2:
                flat_v[e] = np.float32(th + he)                # on the band's edge (as rounding leaves it)
            elif m == 3:
                flat_v[e] = np.float32(th - he)
            elif m == 4:
                flat_i[e] = -1
            elif m == 5:
                flat_i[e] = H
            elif m == 6:
                flat_v[e] = -0.0
            elif m == 7:
                flat_v[e] = np.nextafter(th, np.float32(np.inf), dtype=np.float32)
            else:
                flat_v[e] = np.inf
        if H >= 4:
            theta[0], theta[1], theta[2], theta[3] = np.nan, np.inf, 0.0, -0.0
    else:
        raise ValueError(kind)
    return idx, val, theta, np.float32(eps)


KINDS = ("all", "none", "mixed", "special")
