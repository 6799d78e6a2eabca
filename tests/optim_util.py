"""What the optimizer tests share: the Adam step restated in numpy (fp32, one rounding per operation, and fp64 as the ruler),
qsae_prefilter_pack_w restated in numpy (lane chains, xor-shuffle tree, safety factors), the case generators and the
comparison.

"Bit for bit" here means: the same bit pattern wherever the value is not a NaN, and a NaN in the same places.  Which
payload (and sign) a NaN carries after an operation on two NaNs is the hardware's choice, not part of the contract.
"""
import math

import numpy as np

F32 = np.float32

# (n) of the flat cases; 70001 needs more than one grid-stride trip on the emulated grid
ADAM_SIZES = [1, 3, 4, 5, 1023, 1029, 70001]
# (H, D, variant) of the encoder-pair cases
PREF_CASES = [(1, 4, "plain"), (5, 4, "plain"), (4, 68, "plain"), (9, 64, "plain"), (8, 512, "plain"), (8, 64, "nobias"),
              (8, 64, "zero"), (8, 64, "nan")]


def scalars(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, t=3):
    """The six scalars of step t in Python floats (doubles), as the optimizer computes them."""
    b1, b2 = betas
    return (1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** t), eps, lr / (1 - b1 ** t))


def adam_f32(p, g, m, v, sc):
    """One step, every operation rounded to fp32 -> (p', m', v')."""
    omb1, b2, omb2, bc2, eps, step = (F32(s) for s in sc)
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        d = (g - m).astype(F32)
        m2 = (m + (d * omb1).astype(F32)).astype(F32)
        a = (v * b2).astype(F32)
        q = (g * g).astype(F32)
        v2 = (a + (q * omb2).astype(F32)).astype(F32)
        s = np.sqrt(v2).astype(F32)
        r = (s / bc2).astype(F32)
        den = (r + eps).astype(F32)
        u = (m2 / den).astype(F32)
        p2 = (p - (step * u).astype(F32)).astype(F32)
    return p2, m2, v2


def adam_f64(p, g, m, v, sc):
    """The same step in fp64 with the scalars as doubles: the ruler."""
    omb1, b2, omb2, bc2, eps, step = sc
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        m2 = m + (g - m) * omb1
        v2 = v * b2 + g * g * omb2
        p2 = p - step * (m2 / (np.sqrt(v2) / bc2 + eps))
    return p2, m2, v2


def fma_f32(a, b, c):
    """fmaf on fp32 arrays, exactly: the product is exact in fp64, the sum is taken with its rounding error (two-sum) and
    rounded to odd, and fp64 rounded to odd rounds to fp32 like the exact value (53 >= 2 * 24 + 2)."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        prod = a * b
        hi = prod + c
        bb = hi - prod
        lo = (prod - (hi - bb)) + (c - bb)
        fix = np.isfinite(hi) & np.isfinite(lo) & (lo != 0) & ((hi.view(np.uint64) & np.uint64(1)) == 0)
        toward = np.where(lo > 0, np.inf, -np.inf)
        hi = np.where(fix, np.nextafter(hi, toward), hi)
        return hi.astype(F32)


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _lane_major(row, D):
    """[trips, 64] view of a row: element [t, l] is d = l + 64 t; the idle lanes of the last trip are masked out."""
    trips = (D + 63) // 64
    pad = np.zeros(trips * 64, F32)
    pad[:D] = row
    live = np.arange(trips * 64) < D
    return pad.reshape(trips, 64), live.reshape(trips, 64)


def _tree_sum(x):
    for off in (32, 16, 8, 4, 2, 1):
        x = (x + x[np.arange(64) ^ off]).astype(F32)
    return x[0]


def _tree_max(mx):
    for off in (32, 16, 8, 4, 2, 1):
        o = mx[np.arange(64) ^ off]
        mx = np.where((o > mx) | (o != o), o, mx)
    return mx[0]


def pow2_scale_for(maxabs):
    maxabs = F32(maxabs)
    if maxabs != maxabs or maxabs == F32(np.inf):
        return F32(0)
    if maxabs == 0:
        return F32(1)
    _, e = np.frexp(maxabs)
    with np.errstate(all="ignore"):
        return F32(np.ldexp(F32(1), 7 - int(e)))


def pack_w(W, bias):
    """qsae_prefilter_pack_w restated -> (Wq fp16 [H, D], meta fp32 [4])."""
    W = np.asarray(W, F32)
    H, D = W.shape
    meta = np.zeros(4, np.uint32)
    wmax = np.uint32(0)
    with np.errstate(all="ignore"):
        for h in range(H):
            w, live = _lane_major(W[h], D)
            mx, ss = np.zeros(64, F32), np.zeros(64, F32)
            for t in range(w.shape[0]):
                a = np.abs(w[t])
                mx = np.where(live[t] & ((a > mx) | (a != a)), a, mx)
                ss = np.where(live[t], fma_f32(w[t], w[t], ss), ss)
            nrm = (np.sqrt(_tree_sum(ss)).astype(F32) * F32(1.000001)).astype(F32)
            meta[1] = max(meta[1], _bits(nrm))
            wmax = max(wmax, _bits(_tree_max(mx)))
            if bias is not None:
                meta[2] = max(meta[2], _bits(np.abs(F32(bias[h]))))
        sw = pow2_scale_for(np.uint32(wmax).view(F32))
        meta[0] = _bits(sw)
        scaled = ((W * sw).astype(F32) + F32(0)).astype(F32)          # + 0: an exactly zero product is +0 (pref_w_cast)
        Wq = scaled.astype(np.float16)
        if sw > 0:
            back = (F32(1) / sw).astype(F32)
            kept = (Wq.astype(F32) * back).astype(F32)
            err = np.abs((W - kept).astype(F32))
            err = np.where(np.abs(Wq.astype(F32)) < F32(6.103515625e-5), np.fmax(err, np.abs(W)), err)
            # fmaxf returns the other operand for a NaN; with sw > 0 there is none
            for h in range(H):
                e, live = _lane_major(err[h], D)
                ff = np.zeros(64, F32)
                for t in range(e.shape[0]):
                    ff = np.where(live[t], fma_f32(e[t], e[t], ff), ff)
                meta[3] = max(meta[3], _bits((np.sqrt(_tree_sum(ff)).astype(F32) * F32(1.0001)).astype(F32)))
    return Wq, meta.view(F32)


def same_bits(got, want):
    """Bit for bit in the sense of this module's docstring."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    view = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(view)[~gn], want.view(view)[~wn]))


# ---- cases -------------------------------------------------------------------------------------------------------------------
PLANTS = ("zero", "tiny", "huge", "negzero", "nan")


def bulk_grad(rng, shape):
    """magnitudes 10 ** U(-6, 0) with a random sign"""
    return (10.0 ** rng.uniform(-6, 0, shape) * rng.choice([-1.0, 1.0], shape)).astype(F32)


def plant(g, m, v, plants=PLANTS):
    """One element per planted gradient (as many as fit), spread over the flat tensors; in place.
    zero: g = 0 with m = v = 0 (den = eps, u = 0); tiny: g = 1e-22 (g * g subnormal); huge: g = 1e20 (g * g = inf, p
    unchanged); negzero: g = -0.0; nan: arrives in p', m', v'."""
    n = g.size
    gf, mf, vf = g.reshape(-1), m.reshape(-1), v.reshape(-1)
    for k, name in enumerate(plants[:n]):
        i = k if n < 64 else (k * (n // len(plants)) + 3 * k + 1) % n
        if name == "zero":
            gf[i] = 0.0; mf[i] = 0.0; vf[i] = 0.0
        elif name == "tiny":
            gf[i] = 1e-22
        elif name == "huge":
            gf[i] = 1e20
        elif name == "negzero":
            gf[i] = -0.0
        elif name == "nan":
            gf[i] = np.nan


def adam_case(n, seed=0, plants=PLANTS):
    """-> p, g, m, v (fp32 [n]): a state as after a few steps, the bulk gradient and the plants."""
    rng = np.random.default_rng([seed, n])
    p = rng.normal(0, 0.05, n).astype(F32)
    g = bulk_grad(rng, n)
    m = (bulk_grad(rng, n) * F32(0.1)).astype(F32)
    v = (rng.uniform(0, 1e-3, n)).astype(F32)
    plant(g, m, v, plants)
    return p, g, m, v


def pref_case(H, D, variant, seed=0):
    """-> (W, gW, mW, vW) [H, D] and (bias, gb, mb, vb) [H] or None.  plain / nobias: every plant but the NaN; zero: zero
    weights, gradients and moments (W' = 0); nan: the NaN plant as well."""
    if variant == "zero":
        z = lambda *s: np.zeros(s, F32)                                            # noqa: E731
        return (z(H, D), z(H, D), z(H, D), z(H, D)), (z(H), z(H), z(H), z(H))
    plants = PLANTS if variant == "nan" else PLANTS[:4]
    w = tuple(a.reshape(H, D) for a in adam_case(H * D, seed=seed + 1, plants=plants))
    b = None if variant == "nobias" else adam_case(H, seed=seed + 2, plants=())
    return w, b


def pref_expected(w, b, sc):
    """restatement-Adam followed by the pack_w restatement -> (W', mW', vW'), (b', mb', vb') or None, Wq, meta"""
    W2, mW2, vW2 = adam_f32(*w, sc)
    b2 = adam_f32(*b, sc) if b is not None else None
    Wq, meta = pack_w(W2, b2[0] if b2 is not None else None)
    return (W2, mW2, vW2), b2, Wq, meta
