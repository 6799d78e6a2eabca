"""Numpy restatement of csrc/watch.hip (qsae_tensor_stats), the torch restatement of wandb's recipe, the test cases and the
error bounds the tests use.

The bin rule, every operation in fp32 with one rounding each, as torch.histc applies it on the CPU:
    q = ((x - lo) * float32(bins)) / (hi - lo);  bin = int(q);  bin == bins (x == hi) goes to bins - 1.
The other fp32 candidate, ((x - lo) / (hi - lo)) * bins, is the same whenever bins is a power of two (the scaling is exact
in either place, short of overflow and underflow); at bins = 100 the two part, and SEPARATORS keeps three (lo, hi, x)
triples on which torch sides with the first form.  lo == hi: torch widens the range to lo' = fl(lo - 1), or the float below
lo where that rounds back to lo (lo itself where that float is -inf), and hi' likewise upwards; found by probing torch 2.10
and pinned by tests/test_watch_host.py.  hi - lo = inf: torch counts nothing.  A zero lo or hi is reported as +0.0.

Order of the fp64 sums.  A tensor is cut into chunks of CHUNK = 8192 elements, a chunk into 8 slabs of 1024.  Thread j of 256
adds its finite elements 4 j .. 4 j + 3 of slab 0, then of slab 1, ... from 0.0; the 64 lane sums of a wave are joined by the
butterfly s[l] + s[l ^ m], m = 32, 16, ..., 1; the 4 wave sums are added in ascending order.  Thread j of the join adds the
chunk partials j, j + 256, ... from 0.0 and the 256 thread sums are joined the same way.  mean = S / n_finite; the second
sum adds (float64(x) - mean)^2 in the same order.  (Skipped elements are restated as adding +0.0: no accumulator here is
ever -0.0, so that changes no bit.)

Bounds against torch's fp64 mean and std.  With u = 2^-53, any order of adding n numbers in fp64 is within (n - 1) u sum|x|
of the exact sum (first order; doubled below), and so is torch's.  Hence |mean - mean_ref| <= d_mean = 4 n u mean|x|.  A mean
off by d adds exactly n d^2 to the sum of squared deviations; each term (x - mean)^2 carries 3 roundings and the sum n more:
|m2 - m2_ref| <= d_m2 = 4 (n + 4) u m2 + 2 n d_mean^2.  std = sqrt(m2 / (n - 1)) moves by d_m2 / (2 std (n - 1)) + 2 u std, or
by sqrt(d_m2 / (n - 1)) where std is 0."""
import numpy as np
import torch

F = np.float32
CHUNK, SLABS, THREADS, TABLE, HEAD, MAX_BINS = 8192, 8, 256, 32, 8, 256
U53 = 2.0 ** -53
FMAX = float(np.finfo(F).max)

# (bits of lo, bits of hi, bits of x, bin of the form above, bin of the other form) at bins = 100; torch gives the first
SEPARATORS = [(3201122413, 3192201823, 3197416824, 53, 52), (3235263508, 3233635361, 3233912146, 82, 83),
              (1067233501, 1069976633, 1069729751, 90, 91)]
SEPARATOR_BINS = 100


# ---- the bin rule -------------------------------------------------------------------------------------------------------------
def widened(lo, hi):
    """-> (lo', hi') of the bins for lo <= hi (fp32)"""
    lo, hi = F(lo), F(hi)
    if lo != hi:
        return lo, hi
    with np.errstate(over="ignore"):
        rlo, rhi = F(lo - F(1)), F(hi + F(1))
        if rlo == lo:
            rlo = np.nextafter(lo, F(-np.inf))
            rlo = lo if np.isinf(rlo) else rlo
        if rhi == hi:
            rhi = np.nextafter(hi, F(np.inf))
            rhi = hi if np.isinf(rhi) else rhi
    return F(rlo), F(rhi)


def bin_index(x, lo, hi, bins):
    """x: finite fp32 array within [lo, hi] -> int64 bins, or None where hi' - lo' overflows (no histogram)"""
    rlo, rhi = widened(lo, hi)
    with np.errstate(over="ignore", invalid="ignore"):
        width = F(rhi - rlo)
        if not np.isfinite(width):
            return None
        num = (x - rlo).astype(F)
        scaled = (num * F(bins)).astype(F)
        q = (scaled / width).astype(F)
        ok = (q >= 0) & (q < F(bins) + F(1))                   # q infinite or NaN: bin 0
    b = np.where(ok, q, 0).astype(np.int64)
    b[b == bins] = bins - 1
    return b


def other_form_index(x, lo, hi, bins):
    q = (((x - lo).astype(F) / F(hi - lo)).astype(F) * F(bins)).astype(F)
    b = q.astype(np.int64)
    b[b == bins] = bins - 1
    return b


# ---- the sums ---------------------------------------------------------------------------------------------------------------
def _block_add(v):
    """v float64 [..., 256] -> [...]: butterfly inside each wave of 64, then the 4 waves in ascending order"""
    s = v.reshape(v.shape[:-1] + (4, 64)).copy()
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lanes ^ m]
    w = s[..., 0]
    r = w[..., 0]
    for k in range(1, 4):
        r = r + w[..., k]
    return r


def ordered_sum(terms):
    """terms float64 [n], +0.0 where an element is skipped -> the sum in the kernel's order"""
    n = terms.size
    if n == 0:
        return 0.0
    C = -(-n // CHUNK)
    t = np.zeros(C * CHUNK, np.float64)
    t[:n] = terms
    t = t.reshape(C, SLABS, THREADS, 4).transpose(0, 2, 1, 3).reshape(C, THREADS, SLABS * 4)
    acc = np.zeros((C, THREADS), np.float64)
    for k in range(SLABS * 4):
        acc = acc + t[:, :, k]
    parts = _block_add(acc)                                    # [C]
    G = -(-C // THREADS)
    p = np.zeros(G * THREADS, np.float64)
    p[:C] = parts
    p = p.reshape(G, THREADS)
    acc = np.zeros(THREADS, np.float64)
    for g in range(G):
        acc = acc + p[g]
    return float(_block_add(acc))


def restate_one(x, bins):
    """x fp32 [n] -> dict of the result words of one tensor"""
    x = np.ascontiguousarray(x, F).reshape(-1)
    fin = np.isfinite(x)
    f = x[fin]
    out = {"lo": F(0), "hi": F(0), "mean": 0.0, "m2": 0.0, "n_finite": int(f.size), "n_nonfinite": int(x.size - f.size),
           "n_zero": int((f == 0).sum()), "counts": np.zeros(bins, np.int64)}
    if f.size == 0:
        return out
    lo, hi = F(f.min()), F(f.max())
    lo = F(0) if lo == 0 else lo                               # -0.0 -> +0.0
    hi = F(0) if hi == 0 else hi
    xd = np.where(fin, x, 0).astype(np.float64)
    mean = ordered_sum(xd) / float(f.size)
    d = xd - mean
    m2 = ordered_sum(np.where(fin, d * d, 0.0))
    b = bin_index(f, lo, hi, bins)
    if b is not None:
        out["counts"] = np.bincount(b, minlength=bins).astype(np.int64)
    out.update(lo=lo, hi=hi, mean=mean, m2=m2)
    return out


def restate_block(tensors, bins):
    """-> uint64 [T, HEAD + bins]: the result block of qsae_tensor_stats"""
    blk = np.zeros((len(tensors), HEAD + bins), np.uint64)
    for t, x in enumerate(tensors):
        r = restate_one(x, bins)
        blk[t, 0:4] = np.array([float(r["lo"]), float(r["hi"]), r["mean"], r["m2"]], np.float64).view(np.uint64)
        blk[t, 4:7] = np.array([r["n_finite"], r["n_nonfinite"], r["n_zero"]], np.int64).view(np.uint64)
        blk[t, HEAD:] = r["counts"].view(np.uint64)
    return blk


def block_counts(blk):
    return np.ascontiguousarray(blk[:, HEAD:]).view(np.int64)


# ---- wandb's recipe (wandb.sdk.lib / wandb/integration/torch/wandb_torch.py: log_tensor_stats) in torch ----------------------------
def wandb_recipe(t: torch.Tensor, bins: int = 64):
    """-> (counts list, edges list) or None where wandb logs nothing; on the device of t, with wandb's host reads"""
    flat = t.detach().reshape(-1)
    if not torch.isfinite(flat).all():
        flat = flat[torch.isfinite(flat)]
    if flat.numel() == 0:
        return None
    lo, hi = flat.min().item(), flat.max().item()
    counts = torch.histc(flat, bins=bins, min=lo, max=hi).cpu()
    edges = torch.linspace(lo, hi, steps=bins + 1)
    return counts.tolist(), edges.tolist()


def histc_cpu(x, bins):
    """x fp32 numpy -> (int64 counts of torch.histc on the CPU over the finite elements, lo, hi), None without any"""
    t = torch.from_numpy(np.ascontiguousarray(x, F).reshape(-1))
    t = t[torch.isfinite(t)]
    if t.numel() == 0:
        return None
    lo, hi = t.min().item(), t.max().item()
    return torch.histc(t, bins=bins, min=lo, max=hi).numpy().astype(np.int64), lo, hi


def moment_bounds(x):
    """x: the finite elements (fp64 numpy) -> (d_mean, d_std) of the module docstring"""
    n = x.size
    d_mean = 4.0 * n * U53 * float(np.abs(x).mean())
    m2 = float(((x - x.mean()) ** 2).sum())
    d_m2 = 4.0 * (n + 4) * U53 * m2 + 2.0 * n * d_mean ** 2
    if n < 2:
        return d_mean, 0.0
    std = np.sqrt(m2 / (n - 1))
    d_std = d_m2 / (2.0 * std * (n - 1)) + 2.0 * U53 * std if std > 0 else float(np.sqrt(d_m2 / (n - 1)))
    return d_mean, d_std


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _bits(*u):
    return np.array(u, np.uint32).view(F)


def _gauss(rng, n, scale=1.0, shift=0.0):
    return (rng.standard_normal(n) * scale + shift).astype(F)


def _sparse_grad(rng, n):
    """mostly exact zeros, as the gradient of a top-k model's decoder"""
    g = np.zeros(n, F)
    at = rng.choice(n, max(1, n // 50), replace=False)
    g[at] = _gauss(rng, at.size, 1e-3)
    return g


def case_lists():
    """name -> list of fp32 arrays.  Every list mixes several of the paths."""
    rng = np.random.default_rng(20260)
    small = [_gauss(rng, n, s, m) for n, s, m in zip((1, 2, 63, 64, 65, 255, 257, 1023),
                                                     (1.0, 1e-3, 37.5, 1.0, 0.02, 5.0, 1e-3, 1.0),
                                                     (0.0, 0.0, 3.0, -1.0, 0.0, 100.0, 0.0, 0.0))]
    one_finite = np.array([np.inf, -np.inf, np.nan, 2.5, np.nan, np.inf] * 20, F)
    one_finite[3::6][1:] = np.nan
    chunks = [_gauss(rng, CHUNK), _gauss(rng, CHUNK + 3, 0.5, 0.25), _sparse_grad(rng, 3 * CHUNK + 77), np.zeros(0, F),
              np.full(65, np.nan, F), one_finite, np.full(300, 0.375, F)]                       # T = 7
    zeros = np.zeros(257, F)
    zeros[5::7] = -0.0
    dyadic = np.tile(np.arange(-32, 33, dtype=F) / F(8), 16)[:1023]
    denormal = (rng.integers(-4000, 4000, 255).astype(np.float64) * 1.4e-45).astype(F)
    huge = _bits(0xFF7FFFFF, 0x7F7FFFFF, 0x7F000000, 0xFF000000, 0, 0x7E967699, 0xFE967699, 0x3F800000) .repeat(8)
    nanmix = _gauss(rng, 1000)
    nanmix[::9] = np.nan
    nanmix[4::50] = np.inf
    edge = [zeros, dyadic, denormal, huge, np.full(64, 2.0 ** 24, F), np.full(3, 2.0 ** 26, F), np.full(5, FMAX, F),
            np.full(5, -FMAX, F), np.full(2, -3.0e10, F), nanmix, np.zeros(1, F)]
    seps = [np.concatenate([_bits(lo, hi, x), _bits(x).repeat(6)]) for lo, hi, x, _, _ in SEPARATORS]
    sizes = (1, 2, 63, 64, 65, 255, 257, 1023)
    table = [_gauss(rng, sizes[i % 8] if i != 20 else 0, 1.0 + i) for i in range(TABLE + 1)]    # one above the launch's table
    return {"small": small, "chunks": chunks, "edge": edge, "separators": seps + [dyadic], "table": table,
            "single": [_gauss(rng, 1023, 2.0)]}


# (list name, bins): every list at 64, the small and the edge list at 1 and 256 as well, the separators at their own 100
RUNS = [("small", 64), ("chunks", 64), ("edge", 64), ("table", 64), ("single", 64), ("small", 1), ("edge", 1), ("small", 256),
        ("edge", 256), ("separators", SEPARATOR_BINS)]
RUN_IDS = [f"{n}_{b}" for n, b in RUNS]
