"""The numpy restatement of include/qsae_jump_dense.h, written from the header: oracle.encode for the pre-activations, the two
predicates over every unit, the rank order (value descending with -0 and +0 as one value, then unit ascending), truncation to K,
l0 from the uncapped counts, and the report.  Shared by tests/test_jump_dense_host.py and tests/test_jump_dense_gpu.py; no GPU,
no library but the oracle."""
import numpy as np

import oracle

REPORT_WORDS = 6
REPORT_NAMES = ("selected", "band_entries", "truncated_rows", "empty_rows", "band_truncated_rows", "firing")
NAMES = ("idx_sel", "val_sel", "counts", "idx_band", "counts_band", "l0", "report")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def half_eps(eps):
    """fl32(0.5f * eps)"""
    return np.float32(np.float32(0.5) * np.float32(eps))


def preact(x, W, bias):
    """z fp32 [B, H]: the fmaf chain in ascending k, seeded with the bias"""
    return oracle.encode(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(W, np.float32),
                         None if bias is None else np.ascontiguousarray(bias, np.float32))


def predicates(z, theta, eps):
    """-> (selected, in the band), two bool [B, H]"""
    z, theta = np.asarray(z, np.float32), np.asarray(theta, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sel = z > theta[None, :]                               # NaN on either side: False
        d = (z - theta[None, :]).astype(np.float32)            # one fp32 subtraction
        band = np.abs(d) < half_eps(eps)
    return sel, band


def rank_order(zr, units):
    """`units` (of one row) by value descending -- -0 and +0 are one value --, then unit ascending"""
    units = np.asarray(units, np.int64)
    v = zr[units].astype(np.float64) + 0.0                      # -0 + 0 = +0; no NaN is ever kept
    return units[np.lexsort((units, -v))]


def ranked_lists(z, keep, K, with_val):
    B, H = z.shape
    idx = np.full((B, K), -1, np.int32)
    val = np.zeros((B, K), np.float32) if with_val else None
    n = keep.sum(axis=1).astype(np.int64)
    for r in range(B):
        order = rank_order(z[r], np.flatnonzero(keep[r]))[:K]
        idx[r, :order.size] = order
        if with_val:
            val[r, :order.size] = z[r, order]
    return idx, val, n


def encode_jump_from_z(z, theta, K, eps):
    """-> (idx_sel, val_sel, counts, idx_band, counts_band, l0 fp32, report int64 [6]) from the pre-activations"""
    z = np.asarray(z, np.float32)
    B = z.shape[0]
    sel, band = predicates(z, theta, eps)
    idx_sel, val_sel, n_sel = ranked_lists(z, sel, K, True)
    idx_band, _, n_band = ranked_lists(z, band, K, False)
    counts = np.minimum(n_sel, K).astype(np.int32)
    counts_band = np.minimum(n_band, K).astype(np.int32)
    report = np.array([int(counts.sum()), int(counts_band.sum()), int((n_sel > K).sum()), int((counts == 0).sum()),
                       int((n_band > K).sum()), int(n_sel.sum())], dtype=np.int64)
    l0 = np.float32(np.float64(int(n_sel.sum())) / np.float64(B))
    return idx_sel, val_sel, counts, idx_band, counts_band, l0, report


def encode_jump(x, W, bias, theta, K, eps):
    """qsaed_encode_jump, restated"""
    return encode_jump_from_z(preact(x, W, bias), theta, K, eps)


def dense_latent(z, theta):
    """where(z > theta, z, 0): the model's JumpReLU output"""
    with np.errstate(invalid="ignore"):
        return np.where(z > np.asarray(theta, np.float32)[None, :], z, np.float32(0.0)).astype(np.float32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
KINDS = ("all", "none", "mixed", "special")


def operands(B, D, H, seed, with_bias=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, D)).astype(np.float32)
    W = (rng.standard_normal((H, D)) / np.sqrt(D)).astype(np.float32)
    bias = (rng.standard_normal(H) * 0.1).astype(np.float32) if with_bias else None
    return x, W, bias


def case(kind, B, D, H, seed=0, eps=0.25, with_bias=True, quantile=0.9):
    """-> (x, W, bias, theta, eps) of a named threshold pattern.  "all": every unit fires (theta = -inf); "none": theta = +inf;
    "mixed": one threshold per unit around the `quantile` of the pre-activations, so some units fire in every row and bands are
    populated; "special": thresholds that EQUAL a pre-activation, sit one ulp beside it or exactly on a band edge, NaN / inf / +-0
    thresholds, a row of x with a NaN, a row of zeros (z = bias, or +0), and a bias entry of -0."""
    x, W, bias = operands(B, D, H, seed + 31 * B + 7 * D + H, with_bias)
    rng = np.random.default_rng(seed + 1000)
    eps = np.float32(eps)
    if kind == "special":
        x = x.copy()
        if B >= 2:
            x[B - 1, :] = 0.0                                  # z = bias (or +0): -0 against +0
        if B >= 3:
            x[1, D // 2] = np.nan                              # the whole row is NaN: neither predicate anywhere
        if bias is not None:
            bias = bias.copy()
            bias[H - 1] = -0.0
    z = preact(x, W, bias)
    zf = z[np.isfinite(z)]
    base = np.float32(np.quantile(zf, quantile)) if zf.size else np.float32(0.5)
    theta = (base + np.abs(rng.standard_normal(H)) * 0.1).astype(np.float32)
    if kind == "all":
        theta = np.full(H, -np.inf, np.float32)
    elif kind == "none":
        theta = np.full(H, np.inf, np.float32)
    elif kind == "mixed":
        pass
    elif kind == "special":
        he = half_eps(eps)
        rows = [r for r in range(B) if np.isfinite(z[r]).all()] or [0]
        for t, h in enumerate(rng.permutation(H)[:max(1, (H * 3) // 4)]):
            zr = z[rows[t % len(rows)], h]
            m = t % 8
            if not np.isfinite(zr):
                continue
            if m == 0:
                theta[h] = zr                                  # equal: not selected, in the band
            elif m == 1:
                theta[h] = np.nextafter(zr, np.float32(-np.inf), dtype=np.float32)     # one ulp below: selected
            elif m == 2:
                theta[h] = np.float32(zr - he)                 # on the band's edge (as rounding leaves it)
            elif m == 3:
                theta[h] = np.float32(zr + he)
            elif m == 4:
                theta[h] = np.nextafter(zr, np.float32(np.inf), dtype=np.float32)
            elif m == 5:
                theta[h] = np.float32(zr + np.float32(0.5) * he)                      # in the band, not selected
            elif m == 6:
                theta[h] = np.float32(-abs(zr))                # a negative threshold: zeros fire
        if H >= 8:
            theta[0], theta[1], theta[2], theta[3] = np.nan, np.inf, 0.0, -0.0
            theta[H - 1] = -1.0                                # the unit whose bias is -0 fires in the row of zeros: val -0
    else:
        raise ValueError(kind)
    return x, W, bias, theta.astype(np.float32), eps
