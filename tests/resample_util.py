"""The numpy restatement of csrc/resample.hip: every sum in the order the kernel's comment states,
operation for operation, so that the results are compared bit for bit.  Imports no GPU.

The two orders:

* ``block_sum``: 256 partial sums, partial t adds a[t], a[t + 256], ... in that order onto 0.0; then s[t] += s[t + k] for
  t < k, k = 128, 64, ..., 1.
* ``prefix_sum``: chunks of 1024 weights, 4 consecutive ones per thread added in order onto 0.0; the 256 thread totals of a
  chunk added in order onto 0.0; the chunk totals added in order onto 0.0; cdf = O_g + (E_t + p_i).
"""
import numpy as np

THREADS = 256
PER = 4
CHUNK = THREADS * PER
MAX_D = 4096
REPORT_WORDS = 8
DEAD, REVIVED, DUPLICATE, DEGENERATE, NO_WEIGHT, SKIPPED = range(6)
NO_ROW, LOST_ROW = -1, -2
POISON32 = np.frombuffer(b"\x5a" * 4, np.int32)[0]


def align256(v):
    return (v + 255) // 256 * 256


def draw_workspace_bytes(N):
    if N <= 0:
        return 0
    return align256(8 * N) + align256(8 * ((N + CHUNK - 1) // CHUNK)) + align256(4 * N)


def block_sum(a):
    """fp64 [..., L] -> [...] in the workgroup's order"""
    a = np.asarray(a, np.float64)
    L = a.shape[-1]
    k = max((L + THREADS - 1) // THREADS, 1)
    pad = np.zeros(a.shape[:-1] + (k * THREADS,), np.float64)
    pad[..., :L] = a
    pad = pad.reshape(a.shape[:-1] + (k, THREADS))
    s = np.zeros(a.shape[:-1] + (THREADS,), np.float64)
    with np.errstate(all="ignore"):
        for i in range(k):
            s = s + pad[..., i, :]
        step = THREADS // 2
        while step >= 1:
            s = s[..., :step] + s[..., step:2 * step]
            step //= 2
    return s[..., 0]


def row_weights(x, recon):
    """x, recon fp32 [N, D] -> w fp64 [N]"""
    with np.errstate(all="ignore"):
        diff = (np.asarray(x, np.float32) - np.asarray(recon, np.float32)).astype(np.float32).astype(np.float64)
        e = block_sum(diff * diff)
        return np.where(np.isfinite(e), e * e, 0.0)


def prefix_sum(w):
    """w fp64 [N] -> cdf fp64 [N]"""
    w = np.asarray(w, np.float64)
    N = w.size
    chunks = (N + CHUNK - 1) // CHUNK
    pad = np.zeros(chunks * CHUNK, np.float64)
    pad[:N] = w
    pad = pad.reshape(chunks, THREADS, PER)
    with np.errstate(all="ignore"):
        p = np.cumsum(np.concatenate([np.zeros((chunks, THREADS, 1)), pad], axis=2), axis=2)[..., 1:]      # 0.0 + w0, + w1, ...
        run = np.cumsum(np.concatenate([np.zeros((chunks, 1)), p[..., PER - 1]], axis=1), axis=1)         # E_0 = 0.0, ..., C_g
        before, total = run[:, :THREADS], run[:, THREADS]
        offset = np.cumsum(np.concatenate([[0.0], total]))[:chunks]
        cdf = offset[:, None, None] + (before[:, :, None] + p)
    return cdf.reshape(-1)[:N]


def draw(w, u):
    """-> (rows int32 [n], report int64 [8]) of qsae_resample_draw"""
    u = np.asarray(u, np.float64)
    n = u.size
    report = np.zeros(REPORT_WORDS, np.int64)
    rows = np.full(n, NO_ROW, np.int32)
    if n == 0:
        return rows, report
    report[DEAD] = n
    cdf = prefix_sum(w)
    total = cdf[-1]
    if not (total > 0.0) or not np.isfinite(total):
        report[NO_WEIGHT] = n
        return rows, report
    owner = {}
    for j in range(n):
        target = u[j] * total
        r = int(np.argmax((cdf > target) | (cdf >= total)))     # the smallest r at which the predicate holds
        rows[j] = r
        owner.setdefault(r, j)                                   # j ascending: the first drawer is the smallest j
    for j in range(n):
        if owner[int(rows[j])] != j:
            rows[j] = LOST_ROW
            report[DUPLICATE] += 1
    return rows, report


def alive_stats(W_enc, logits, dead):
    """-> stats fp64 [2]"""
    W = np.asarray(W_enc, np.float32).astype(np.float64)
    H = W.shape[0]
    unit_norm = np.sqrt(block_sum(W * W))
    counted = np.ones(H, bool)
    counted[np.asarray(dead, np.int64)] = False
    if not counted.any():
        counted[:] = True
    count = float(counted.sum())
    stats = np.zeros(2, np.float64)
    stats[0] = block_sum(np.where(counted, unit_norm, 0.0)) / count
    if logits is not None:
        A = np.abs(np.asarray(logits, np.float32).astype(np.float64))
        unit_abs = block_sum(A)
        stats[1] = block_sum(np.where(counted, unit_abs, 0.0)) / (count * float(A.shape[1]))
    return stats


def quantize(v, n_bits):
    """v fp32 [D] (not all zero) -> q int [D]: clamp(rint(fp64(v) (max(qmax, 1) / fp64(max |v|))), -2^(n_bits-1), qmax)"""
    wide = np.asarray(v, np.float32).astype(np.float64)
    qmax, qmin = 2 ** (n_bits - 1) - 1, -(2 ** (n_bits - 1))
    ratio = float(max(qmax, 1)) / np.abs(wide).max()
    return np.clip(np.rint(wide * ratio), qmin, qmax).astype(np.int64)


def write(dead, rows, x, dec_bias, stats, W_enc, b_enc, dec, report, *, n_bits=None, moments=None, last=None, rows_seen=0,
          encoder_scale=0.2, logit_scale=None):
    """The write of qsae_resample_write_table (n_bits None, dec fp32 [D, H]) or _binary (dec fp32 [H, D n_bits]) on copies ->
    dict of W_enc, b_enc, dec, report, moments (list of 6 arrays or None), last, q (unit -> the integers written)."""
    W_enc, b_enc, dec, report = W_enc.copy(), b_enc.copy(), dec.copy(), report.copy()
    moments = [m.copy() if m is not None else None for m in (moments if moments is not None else [None] * 6)]
    last = last.copy() if last is not None else None
    x = np.asarray(x, np.float32)
    H, D = W_enc.shape
    N = x.shape[0]
    q_of = {}

    def put(t, m, v, at, value):
        t[at] = value
        for s in (m, v):
            if s is not None:
                s[at] = 0.0
    for j in range(len(dead)):
        h, r = int(dead[j]), int(rows[j])
        if h < 0 or h >= H or (j > 0 and int(dead[j - 1]) >= h) or r >= N:
            report[SKIPPED] += 1
            continue
        if r < 0:
            continue
        with np.errstate(all="ignore"):
            v = (x[r] - np.asarray(dec_bias, np.float32)).astype(np.float32)
            wide = v.astype(np.float64)
            s = block_sum(wide * wide)
        if not (s > 0.0) or not np.isfinite(s):
            report[DEGENERATE] += 1
            continue
        nrm = np.sqrt(s)
        c = (np.float64(encoder_scale) * stats[0]) / nrm
        put(W_enc, moments[0], moments[1], h, (wide * c).astype(np.float32))
        put(b_enc, moments[2], moments[3], h, np.float32(0.0))
        if n_bits is None:
            put(dec, moments[4], moments[5], (slice(None), h), (wide / nrm).astype(np.float32))
        else:
            q = quantize(v, n_bits)
            q_of[h] = q
            L = np.float32(logit_scale) if logit_scale is not None else np.float32(stats[1])
            bits = ((q[:, None] & (2 ** n_bits - 1)) >> np.arange(n_bits)[None, :]) & 1
            put(dec, moments[4], moments[5], h, np.where(bits.reshape(-1) == 1, L, -L).astype(np.float32))
        if last is not None:
            last[h] = rows_seen
        report[REVIVED] += 1
    return {"W_enc": W_enc, "b_enc": b_enc, "dec": dec, "report": report, "moments": moments, "last": last, "q": q_of}


# ---- cases shared by the host-emulation and the GPU tests -------------------------------------------------------------------
ROW_SHAPES = [(1, 4, 4), (67, 36, 36), (1029, 516, 520), (3, 4096, 4096)]            # (N, D, row stride)


def rows_case(N, D, ld, seed=0, specials=True):
    """x, recon fp32 [N, ld] (columns >= D are never read: they hold NaN); with ``specials`` some rows hold NaN, +-inf, 3e38"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, ld)).astype(np.float32)
    recon = (x + 0.1 * rng.standard_normal((N, ld))).astype(np.float32)
    x[:, D:], recon[:, D:] = np.nan, np.nan
    if specials and N >= 8:
        x[1, 0] = np.nan
        x[2, D - 1] = np.inf
        recon[3, 1] = -np.inf
        x[4, 2], recon[4, 2] = 3e38, -3e38                       # the fp32 difference overflows: weight 0
        x[5, 3] = 3e38                                           # finite in fp64: e = 9e76, w = 8.1e153
        x[6, :D], recon[6, :D] = 1.0, 1.0                        # weight 0
    return x, recon


def weights_case(N, seed=0, zeros=True):
    """fp64 [N] >= 0 with zero weights interleaved"""
    rng = np.random.default_rng(seed)
    w = rng.random(N) ** 4 * 10.0
    if zeros:
        w[rng.random(N) < 0.4] = 0.0
        w[:min(3, N)] = 0.0
        w[N - 1] = 0.0
        if N > 1 and not w.any():
            w[N // 2] = 1.0
    return w


def uniforms(n, seed=0):
    """fp64 [n] in [0, 1) holding 0 and the largest value below 1"""
    u = np.random.default_rng(seed).random(n)
    u[0] = 0.0
    if n > 1:
        u[n - 1] = np.nextafter(1.0, 0.0)
    return u


def model_case(H, D, n_bits=None, seed=0):
    """W_enc [H, D], b_enc [H], dec ([D, H], or [H, D n_bits] logits), dec_bias [D] as fp32"""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((H, D)) / np.sqrt(D)).astype(np.float32)
    b = rng.standard_normal(H).astype(np.float32)
    dec = rng.standard_normal((D, H) if n_bits is None else (H, D * n_bits)).astype(np.float32) * np.float32(3.0)
    return W, b, dec, rng.standard_normal(D).astype(np.float32)


def write_case(H, D, n_bits=None, n=None, seed=0):
    """A whole write call: dead (holding 0 and H - 1), rows (one -1, one -2, one degenerate row), x [N, D], the model, the
    moments, last and the report as the draw left it."""
    rng = np.random.default_rng(seed + 1)
    W, b, dec, bias = model_case(H, D, n_bits, seed)
    n = min(H, 7 if n is None else n)
    assert 2 <= n <= H
    middle = np.sort(rng.choice(np.arange(1, H - 1), size=n - 2, replace=False))
    dead = np.concatenate([[0], middle, [H - 1]]).astype(np.int32)
    N = n + 3
    x = rng.standard_normal((N, D)).astype(np.float32)
    rows = rng.permutation(N)[:n].astype(np.int32)
    report = np.zeros(REPORT_WORDS, np.int64)
    report[DEAD] = n
    if n >= 4:
        x[rows[1]] = bias                                         # degenerate: the row equals the decoder bias
        rows[2] = NO_ROW
        rows[3] = LOST_ROW
        report[NO_WEIGHT], report[DUPLICATE] = 1, 1
    moments = [rng.standard_normal(t.shape).astype(np.float32) for t in (W, W, b, b, dec, dec)]
    last = rng.integers(0, 1000, H).astype(np.int64)
    stats = alive_stats(W, dec if n_bits is not None else None, dead)
    return {"dead": dead, "rows": rows, "x": x, "dec_bias": bias, "stats": stats, "W_enc": W, "b_enc": b, "dec": dec,
            "report": report, "moments": moments, "last": last, "n_bits": n_bits, "N": N, "H": H, "D": D}


WRITE_SHAPES = [(4, 4), (1000, 4), (4, 36), (1000, 36), (4, 260), (1000, 260)]         # (H, D); and (H, 4096) with n = 2
