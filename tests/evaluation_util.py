"""Numpy restatements of csrc/evaluation.hip (quantization error of a BinarySAE decoder, dataset moments), the test cases
and the error bounds the tests use.

Summation orders restated here:
  * quantization error, inside a unit: lane l of 64 adds d = l, l + 64, ... in ascending order from 0.0, then the butterfly
    s[l] + s[l ^ m] for m = 32, 16, ..., 1 (every lane ends with the same bits; lane 0's are stored);
  * across units: thread t of 256 starts from unit t and adds t + 256, t + 512, ...; thread 0 then starts from its own sum
    and adds the sums of threads 1 .. min(256, H) - 1 in ascending order;
  * moments, inside a group: row lane r of 16 adds rows r, r + 16, ... from 0.0, then lane 0's sum + lane 1's + ... + lane
    15's; the unflagged groups are added to the running state in ascending group order.

The soft-side bound.  With u = 2^-24 (the unit roundoff of fp32; one ulp is at most 2 u relative), in units of one integer
step:
  * p = 1 / (1 + expf(-l)): an expf within 2 ulp has relative error <= 4 u; it enters 1 + e damped by e / (1 + e) = 1 - p;
    the add and the divide round once each (<= u relative each).  So |dp| <= (4 (1 - p) + 2) u p <= 6 u.
  * p 2^b is exact.  The chain soft = sum_b p_b bw_b: the partial sum after bit b < n - 1 lies in [0, 2^(b+1)), so that add
    rounds by at most 2^b u (the first add, to 0.0, is exact); the last add (the negative MSB term) gives a result of
    magnitude <= 2^(n-1) and rounds by at most 2^(n-1) u: together <= (2^n - 2) u.  The p errors weigh
    sum_b 2^b = 2^n - 1: <= 6 (2^n - 1) u.  So |d soft| <= 7 (2^n - 1) u.
  * step is a power of two in every test, so step * soft and step * hard are exact; diff = w_quant - w_float rounds once
    more, by at most u |diff| <= u (2^n - 1) / 2.  So |d diff| <= 7.5 (2^n - 1) u.
Both are covered by  eps = 8 * 2^-24 * (2^n - 1) * step  per entry.  A sum of N entries differs by at most N eps, a mean by
eps; a sum of squares by N (2 max|v| eps + eps^2); minima and maxima by eps."""
import numpy as np

SIG_GT_BITS, SIG_GE_BITS = 0x33C00001, 0xB43FFFFE          # csrc/common.h
U24, U53 = 2.0 ** -24, 2.0 ** -53
MARGIN = float(np.log(3.0))
GROUP_LANES = 16

# (H, D, n): the GPU cases; the emulator runs the same ones
QUANT_CASES = [(5, 20, 4), (300, 516, 4), (12, 4, 1), (8, 36, 8), (7, 20, 3)]
# (B, D, dtype name)
MOMENT_CASES = [(1, 4, "float32"), (1025, 20, "float32"), (3000, 516, "float32"), (2048, 512, "float16"), (2048, 512, "bfloat16")]


def f32_from_bits(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def eps_of(n, step):
    return 8.0 * U24 * (2 ** n - 1) * step


def step_of(n, gamma=4.0):
    return gamma / 2 ** (n - 1)                            # a power of two for gamma = 4


# ---- inputs -------------------------------------------------------------------------------------------------------------
def max_tuple(n):
    """The n logits of the planted largest |diff|: every bit's probability next to 0.5 and every bit's error of one sign
    (low bits just undecided-off, the sign bit just on): |diff| = 0.49975 (2^n - 1) step, a hair under the supremum."""
    t = np.full(n, -1e-3, np.float32)
    t[n - 1] = 1e-3
    return t


def quant_logits(H, D, n, variant="plain"):
    """fp32 [H, D n]: N(0, 2^2) with planted saturated bits (+-30, +-100), -0.0, the two sigmoid cutoffs of csrc/common.h
    and their predecessors, and the largest-|diff| tuple at flat entry 3 (variant "tie": the same tuple again at the last
    entry but two, which must lose to the lower index; variant "nan": one NaN logit)."""
    rng = np.random.default_rng(1000 * H + 10 * D + n)
    l = (rng.standard_normal((H, D * n)) * 2.0).astype(np.float32)
    flat = l.reshape(-1)
    plants = [30.0, -30.0, 100.0, -100.0, -0.0, f32_from_bits(SIG_GT_BITS), f32_from_bits(SIG_GT_BITS - 1),
              f32_from_bits(SIG_GE_BITS), f32_from_bits(SIG_GE_BITS - 1)]
    first = 5 * n                                          # past the planted maximum at entry 3
    where = first + (np.arange(len(plants)) * 7) % (flat.size - first)
    assert len(set(where.tolist())) == len(plants)
    flat[where] = np.array(plants, np.float32)
    e = l.reshape(H * D, n)
    e[3] = max_tuple(n)
    if variant == "tie":
        e[H * D - 3] = max_tuple(n)
        if n == 1:                                         # at n = 1 the cutoffs reach the supremum: repeat each of them later on
            e[H * D - 8:H * D - 4, 0] = np.array(plants[5:9], np.float32)
    if variant == "nan":
        e[H * D // 2, n // 2] = np.nan
    return l


def moment_rows(B, D, dtype, seed=0):
    rng = np.random.default_rng(77 + B + D + seed)
    x = (rng.standard_normal((B, D)) * 3.0 + 0.25).astype(np.float32)
    if dtype == "float16":
        return x.astype(np.float16)
    if dtype == "bfloat16":                                # kept as the upper 16 bits (truncation: any bf16 will do)
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return x


def moments_as_f32(x):
    """What the kernel's register conversion gives: fp16 widened, bf16 bits << 16."""
    if x.dtype == np.uint16:
        return (x.astype(np.uint32) << 16).view(np.float32)
    return x.astype(np.float32)


# ---- quantization error ---------------------------------------------------------------------------------------------------
def sigmoid32(l):
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-l.astype(np.float32)))).astype(np.float32)


def entries(logits, D, n, step, exact=False):
    """Per entry (h, d), as float64 [H, D]: w_float, w_quant, diff.  exact=False follows the kernel's fp32 chain (on this
    machine's expf); exact=True is the fp64 restatement (sigmoid and sum in fp64, nothing rounded to fp32)."""
    H = logits.shape[0]
    l = logits.reshape(H, D, n)
    bits = l >= f32_from_bits(SIG_GT_BITS)                 # NaN: not set
    code = (bits.astype(np.int64) << np.arange(n)).sum(-1)
    hard = code - ((code >> (n - 1)) << n)
    bw = 2.0 ** np.arange(n)
    bw[-1] *= -1
    if exact:
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-l.astype(np.float64)))
        wf = step * (p * bw).sum(-1)
        wq = step * hard.astype(np.float64)
        return wf, wq, wq - wf
    p = sigmoid32(l)
    soft = np.zeros((H, D), np.float32)
    for b in range(n):
        soft = (soft + (p[..., b] * np.float32(bw[b])).astype(np.float32)).astype(np.float32)
    s = np.float32(step)
    wf = (s * soft).astype(np.float32)
    wq = (s * hard.astype(np.float32)).astype(np.float32)
    diff = (wq - wf).astype(np.float32)
    return wf.astype(np.float64), wq.astype(np.float64), diff.astype(np.float64)


def unit_sums(v):
    """[H, D] float64 -> [H]: the per-unit order (lane chains, then the butterfly).  Zero padding adds +0.0, which changes
    no chain that started from +0.0."""
    H, D = v.shape
    it = (D + 63) // 64
    pad = np.zeros((H, it * 64), np.float64)
    pad[:, :D] = v
    pad = pad.reshape(H, it, 64)
    s = np.zeros((H, 64), np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(it):
            s = s + pad[:, i]
        lanes = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ m]
    return s[:, 0]


def join_sum(u):
    """[H] float64 -> the sum over units in the second kernel's order."""
    H = u.size
    part = []
    with np.errstate(invalid="ignore"):
        for t in range(min(256, H)):
            acc = u[t]
            for h in range(t + 256, H, 256):
                acc = acc + u[h]
            part.append(acc)
        acc = part[0]
        for v in part[1:]:
            acc = acc + v
    return acc


def mono_key32(v):
    v = np.asarray(v, np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    k = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(v), 0xFFFFFFFF, k).astype(np.uint64)


def quant_restate(logits, D, n, step, margin=MARGIN, exact=False):
    """What qsae_quantization_error returns, as a dict: sums [6], min_f, max_f, min_q, max_q, key, max_abs, flat, n_nan,
    abs [n], pol [n], und [n] (per plane), unit_err_sq [H], logits of the key's entry.  With exact=True the soft side is
    the fp64 restatement (|diff| for the key included, so its high word is not comparable)."""
    H = logits.shape[0]
    wf, wq, diff = entries(logits, D, n, step, exact)
    unit = unit_sums(diff * diff)
    sums = [join_sum(unit)] + [join_sum(unit_sums(v)) for v in (np.abs(diff), wf, wf * wf, wq, wq * wq)]
    l = logits.reshape(H, D, n)
    if exact:
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-l.astype(np.float64)))
        pol_terms = p * (1.0 - p)
    else:
        p = sigmoid32(l)
        pol_terms = (p * (np.float32(1.0) - p)).astype(np.float32).astype(np.float64)
    a = np.abs(l)
    ad = np.abs(diff).reshape(-1)
    if exact:
        flat = int(np.argmax(np.where(np.isnan(ad), np.inf, ad)))
        key = None
    else:
        keys = (mono_key32(ad.astype(np.float32)) << np.uint64(32)) | (~np.arange(H * D, dtype=np.uint64) & np.uint64(0xFFFFFFFF))
        key = int(keys.max())
        flat = (~key) & 0xFFFFFFFF
    with np.errstate(invalid="ignore"):
        return {"sums": np.array(sums), "min_f": np.nanmin(wf), "max_f": np.nanmax(wf), "min_q": wq.min(), "max_q": wq.max(),
                "key": key, "max_abs": float(ad[flat]), "flat": flat, "n_nan": int(np.isnan(l).sum()),
                "abs": np.array([join_sum(unit_sums(a[..., b].astype(np.float64))) for b in range(n)]),
                "pol": np.array([join_sum(unit_sums(pol_terms[..., b])) for b in range(n)]),
                "und": np.array([int((a[..., b] < np.float32(margin)).sum()) for b in range(n)]),
                "unit_err_sq": unit, "entry_logits": l.reshape(H * D, n)[flat].astype(np.float64)}


def parse_block(block):
    """The 48-word result block (float64 array) -> the dict of quant_restate."""
    f = np.asarray(block, np.float64)
    i, k = f.view(np.int64), f.view(np.uint64)
    key = int(k[10])
    hi = key >> 32
    if hi == 0xFFFFFFFF:
        max_abs = float("nan")
    else:
        bits = (hi & 0x7FFFFFFF) if hi & 0x80000000 else (~hi & 0xFFFFFFFF)
        max_abs = float(f32_from_bits(bits))
    return {"sums": f[:6].copy(), "min_f": f[6], "max_f": f[7], "min_q": f[8], "max_q": f[9], "key": key, "max_abs": max_abs,
            "flat": (~key) & 0xFFFFFFFF, "n_nan": int(i[11]), "abs": f[16:24].copy(), "pol": f[24:32].copy(),
            "und": i[32:40].copy(), "entry_logits": f[40:48].copy(), "reserved": k[12:16].copy()}


def check_quant(got, unit_err_sq, logits, D, n, step):
    """Asserts a result block (parse_block) and unit_err_sq against the restatements: the hard side, the counts and the
    index for equality, the soft side within the bounds of this module's docstring.  Returns the fp64 restatement."""
    H = logits.shape[0]
    N = H * D
    eps = eps_of(n, step)
    ref = quant_restate(logits, D, n, step, exact=True)
    r32 = quant_restate(logits, D, n, step, exact=False)
    nan = ref["n_nan"] > 0
    # hard side: integers times a power-of-two step, exact in fp64 whatever the order
    assert got["sums"][4] == ref["sums"][4] and got["sums"][5] == ref["sums"][5]
    assert got["min_q"] == ref["min_q"] and got["max_q"] == ref["max_q"]
    assert got["n_nan"] == ref["n_nan"]
    assert np.array_equal(got["und"][:n], ref["und"]) and not got["und"][n:].any()
    assert not got["reserved"].any() and not got["abs"][n:].any() and not got["pol"][n:].any()
    # |logit| sums: fp32 values widened, the same order -> the same bits as the fp32-chain restatement (no expf involved)
    assert np.array_equal(got["abs"][:n], r32["abs"], equal_nan=True)
    if nan:
        assert all(np.isnan(got["sums"][j]) for j in range(4)) and np.isnan(got["max_abs"])
        assert got["flat"] == int(np.flatnonzero(np.isnan(logits.reshape(N, n)).any(1))[0])     # the first NaN entry
        assert np.isnan(unit_err_sq).sum() == 1
        return ref
    max_d, max_f = float(np.abs(ref["max_abs"])), float(max(abs(ref["min_f"]), abs(ref["max_f"])))
    sq_d, sq_f = 2 * max_d * eps + eps * eps, 2 * max_f * eps + eps * eps
    assert abs(got["sums"][0] - ref["sums"][0]) <= N * sq_d
    assert abs(got["sums"][1] - ref["sums"][1]) <= N * eps
    assert abs(got["sums"][2] - ref["sums"][2]) <= N * eps
    assert abs(got["sums"][3] - ref["sums"][3]) <= N * sq_f
    assert abs(got["min_f"] - ref["min_f"]) <= eps and abs(got["max_f"] - ref["max_f"]) <= eps
    assert abs(got["max_abs"] - ref["max_abs"]) <= eps
    assert np.all(np.abs(unit_err_sq - ref["unit_err_sq"]) <= D * sq_d)
    # p (1 - p): |dp| <= 6 u and |1 - 2 p| <= 1, the product rounds once more (<= u / 4): per term <= 7 u
    assert np.all(np.abs(got["pol"][:n] - ref["pol"]) <= N * 7 * U24)
    assert np.array_equal(got["entry_logits"][:n], logits.reshape(N, n)[got["flat"]].astype(np.float64))
    # identical logit tuples give identical values on any expf: of those the lowest flat index must be the one reported
    e = logits.reshape(N, n).view(np.uint32)
    assert got["flat"] == int(np.flatnonzero((e == e[got["flat"]]).all(1))[0])
    return ref


def lead_over_runner_up(logits, D, n, step):
    """(flat index of the largest fp64 |diff|, its lead over the largest |diff| of any other entry that holds other logits)."""
    _, _, diff = entries(logits, D, n, step, exact=True)
    ad = np.abs(diff).reshape(-1)
    flat = int(np.argmax(ad))
    e = logits.reshape(-1, n)
    others = np.array([not np.array_equal(e[i].view(np.uint32), e[flat].view(np.uint32)) for i in range(e.shape[0])])
    return flat, float(ad[flat] - ad[others].max()) if others.any() else float("inf")


# ---- dataset moments -------------------------------------------------------------------------------------------------------
def group_partial(v):
    """[rows, D] float64 terms of one group -> [D]: the 16 row lanes' chains, then lane 0 + lane 1 + ... + lane 15."""
    rows, D = v.shape
    it = (rows + GROUP_LANES - 1) // GROUP_LANES
    pad = np.zeros((it * GROUP_LANES, D), np.float64)
    pad[:rows] = v
    pad = pad.reshape(it, GROUP_LANES, D)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((GROUP_LANES, D), np.float64)
        for i in range(it):
            s = s + pad[i]
        acc = s[0]
        for r in range(1, GROUP_LANES):
            acc = acc + s[r]
    return acc


def moments_restate(x, recon, group_rows, cuts=None, state=None):
    """The running state after adding x [B, D] (as the kernel converts it: fp32) in the calls cut at `cuts`:
    (sums float64 [3, D], rows kept, rows skipped)."""
    B, D = x.shape
    sums = np.zeros((3, D), np.float64) if state is None else state[0].copy()
    kept, skipped = (0, 0) if state is None else state[1:]
    cuts = [0, B] if cuts is None else cuts
    xd = x.astype(np.float64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        for g0 in range(a, b, group_rows):
            g1 = min(g0 + group_rows, b)
            if np.isnan(x[g0:g1]).any():
                skipped += g1 - g0
                continue
            kept += g1 - g0
            with np.errstate(invalid="ignore", over="ignore"):
                sums[0] = sums[0] + group_partial(xd[g0:g1])
                sums[1] = sums[1] + group_partial(xd[g0:g1] * xd[g0:g1])
                if recon is not None:
                    e = (recon[g0:g1] - x[g0:g1]).astype(np.float32)
                    sums[2] = sums[2] + group_partial((e * e).astype(np.float32).astype(np.float64))
    return sums, kept, skipped


def fp64_sum_bound(terms, axis=None):
    """|ordered fp64 sum - exact sum| <= n 2^-53 sum |terms| (first order; any order)."""
    n = terms.size if axis is None else terms.shape[axis]
    return n * U53 * np.abs(terms).sum(axis=axis)


def fp32_sum_bound(terms):
    """|fp32 sum in any order - exact sum| <= n 2^-24 sum |terms|."""
    return terms.size * U24 * float(np.abs(terms).sum())
