"""What the tests of the recipe around the Adam step share (include/qsae_optim.h): the numpy restatements of
qsaeo_project_columns in the header's order, of qsaeo_grad_norm in the chunked fp64 order and of its coefficient, of the
clipped / averaged element in fp32 with one rounding per line, and the case generators.  The Adam element itself, fmaf and the
pack_w restatement are tests/optim_util.py's."""
import math

import numpy as np

import optim_util as U

F32 = np.float32
GROUPS = 16                      # QSAEO_PROJECT_GROUPS
CHUNK, SLAB, THREADS = 8192, 1024, 256
HEAD = 4                         # QSAEO_NORM_HEAD

NORM_COUNTS = [0, 1, 3, 8192, 8193, 70001]
NORM_SHIFTED = 4                 # the tensor that starts 4 bytes off its 16-byte boundary
# (D, H, ld): one row; a few rows; a strip tail with ld > H; 32 trips a chain; D no multiple of the 16 chains (and > 16)
PROJECT_CASES = [(1, 4, 4), (5, 8, 8), (7, 260, 264), (512, 64, 64), (37, 72, 76)]
COEFS = [None, 1.0, 0.25, 0.0, float("nan")]
DECAY = 0.999


# ---- the projection -------------------------------------------------------------------------------------------------------
def project_columns(W, G, H):
    """-> G' [D, ld]: 16 chains per column (chain r: rows r, r + 16, ... ascending, fmaf from +0), joined in ascending r;
    a column whose dot compares equal to zero keeps its bits; columns at or past H are not touched."""
    W, G = np.asarray(W, F32), np.asarray(G, F32)
    D = W.shape[0]
    out = G.copy()
    w, g = W[:, :H], G[:, :H]
    with np.errstate(all="ignore"):
        chains = np.zeros((GROUPS, H), F32)
        for d in range(D):
            chains[d % GROUPS] = U.fma_f32(g[d], w[d], chains[d % GROUPS])
        dot = chains[0].copy()
        for r in range(1, GROUPS):
            dot = (dot + chains[r]).astype(F32)
        new = U.fma_f32(np.broadcast_to(-dot, w.shape), w, g)
    out[:, :H] = np.where(dot == 0, g, new)
    return out


def project_case(D, H, ld, seed=0):
    """-> W, G [D, ld]: unit-norm columns, except: column 1 scaled by 3 (non-unit), column 2 zero in W, column 3 zero in G (with
    a -0.0), and -- where there are at least 8 columns -- a NaN in column 5 of G; the columns past H hold a pattern."""
    rng = np.random.default_rng([seed, D, H])
    W = rng.normal(0, 1, (D, ld)).astype(F32)
    W[:, :H] /= np.maximum(np.linalg.norm(W[:, :H].astype(np.float64), axis=0), 1e-8).astype(F32)
    G = U.bulk_grad(rng, (D, ld))
    W[:, 1] *= F32(3)
    W[:, 2] = 0
    G[:, 3] = 0
    G[0, 3] = -0.0
    if H >= 8:
        G[D // 2, 5] = np.nan
    return W, G


# ---- the norm ---------------------------------------------------------------------------------------------------------------
def _butterfly(v):
    """[..., 64] -> [...]: the xor tree 32, 16, ..., 1 in fp64; lane 0"""
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ m]
    return v[..., 0]


def _block_add(v):
    """[..., 256] fp64 -> [...]: the waves' butterflies, then the 4 wave sums in ascending order"""
    w = _butterfly(v.reshape(v.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def sum_squares(x):
    """One tensor's sum of squares in the kernel's order (fp64)."""
    x = np.asarray(x, F32).reshape(-1)
    n = x.size
    if n == 0:
        return np.float64(0.0)
    chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(chunks * CHUNK, np.float64)
    pad[:n] = x.astype(np.float64)
    with np.errstate(all="ignore"):
        sq = pad * pad                                       # the padding adds +0.0 to sums that are never -0.0
        # [chunk, slab, thread, 4] -> a thread's elements in ascending (slab, element) order
        seq = sq.reshape(chunks, CHUNK // SLAB, THREADS, 4).transpose(0, 2, 1, 3).reshape(chunks, THREADS, -1)
        acc = np.zeros((chunks, THREADS), np.float64)
        for i in range(seq.shape[2]):
            acc = acc + seq[:, :, i]
        parts = _block_add(acc)                              # [chunks]
        trips = (chunks + THREADS - 1) // THREADS
        padded = np.zeros(trips * THREADS, np.float64)
        padded[:chunks] = parts
        per = np.zeros(THREADS, np.float64)
        for t in range(trips):
            per = per + padded[t * THREADS:(t + 1) * THREADS]
        return np.float64(_block_add(per))


def coefficient(norm, max_norm):
    """-> the fp32 word: torch's formula in fp64; c >= 1 -> 1; NaN -> NaN; else c rounded once"""
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6))
        if c >= 1.0:
            return F32(1.0)
        if c != c:
            return F32(np.nan)
        return F32(c)


def grad_norm(tensors, max_norm):
    """-> (coef fp32, report: int64 [4 + T] holding the words qsaeo_grad_norm writes)"""
    per = [sum_squares(t) for t in tensors]
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for s in per:
            total = total + s
        norm = np.sqrt(total)
    coef = coefficient(norm, max_norm)
    f = np.array([total, norm, np.float64(coef)] + [0.0] + per, np.float64)
    words = f.view(np.int64).copy()
    words[3] = 0 if coef == F32(1.0) else 1
    return coef, words


def same_report(got, want):
    """int64 words: the fp64 words bit for bit (a NaN where a NaN is), the flag equal"""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    if got.shape != want.shape or got[3] != want[3]:
        return False
    keep = np.arange(got.size) != 3
    return U.same_bits(got[keep].view(np.float64), want[keep].view(np.float64))


def norm_case(kind, seed=0):
    """-> the six tensors of NORM_COUNTS.  kind: "bulk", "zeros", "inf" (one +inf in the largest), "nan" (one NaN in the
    fifth)"""
    rng = np.random.default_rng([seed, 11])
    ts = [np.zeros(n, F32) if kind == "zeros" else U.bulk_grad(rng, n) for n in NORM_COUNTS]
    if kind == "inf":
        ts[5][12345] = np.inf
    if kind == "nan":
        ts[4][8192] = np.nan
    return ts


# ---- the element ------------------------------------------------------------------------------------------------------------
def clip_grad(g, coef):
    """g * coef in fp32, one rounding; coef None: g"""
    if coef is None:
        return np.asarray(g, F32)
    with np.errstate(all="ignore"):
        return (np.asarray(g, F32) * F32(coef)).astype(F32)


def ema_f32(e, p_new, one_minus_decay):
    """t = p' - e; te = t * (1 - decay); e' = e + te: one fp32 rounding per line"""
    e, p_new, omd = np.asarray(e, F32), np.asarray(p_new, F32), F32(one_minus_decay)
    with np.errstate(all="ignore"):
        t = (p_new - e).astype(F32)
        te = (t * omd).astype(F32)
        return (e + te).astype(F32)


def ema_f64(e, p_new, one_minus_decay):
    e, p_new = np.asarray(e, np.float64), np.asarray(p_new, np.float64)
    return e + (p_new - e) * float(one_minus_decay)


def recipe_f32(p, g, m, v, sc, coef=None, ema=None, one_minus_decay=0.0):
    """The clipped / averaged element -> (p', m', v', e' or None)"""
    p2, m2, v2 = U.adam_f32(p, clip_grad(g, coef), m, v, sc)
    return p2, m2, v2, (ema_f32(ema, p2, one_minus_decay) if ema is not None else None)


def ema_case(n, seed=0):
    rng = np.random.default_rng([seed, n, 5])
    return rng.normal(0, 0.05, n).astype(F32)


def one_minus(decay):
    """1 - decay as the optimizer forms it: in Python floats, rounded to fp32 once at the C boundary"""
    return F32(1 - decay)


def exact_norm(tensors):
    """The ruler: sqrt of math.fsum over the fp64 squares (exact products of fp32 values)"""
    return math.sqrt(math.fsum(float(x) * float(x) for t in tensors for x in np.asarray(t, F32).reshape(-1).astype(np.float64)))
