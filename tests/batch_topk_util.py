"""Shared helpers of the BatchTopK tests: the numpy restatement of the contract of include/qsae_batch.h.

``mono_key``: the order of csrc/common.h (NaN first, then +inf ... -0 == +0 ... -inf).  ``batch_select``: the ``n_select`` first
entries in key order (mono_key descending, then row, then list position) -> counts, val_sel, report.  ``threshold_update``: the
moving average of the smallest selected value.  ``threshold_select``: the longest prefix with ``val >= theta``.
``decode_ragged`` / ``row_grad_ragged`` / ``csr_ragged``: the CPU oracle's sparse decode, the row gradient in the kernels' order
of operations and the per-unit lists, over the first ``counts[r]`` entries of every row."""
from __future__ import annotations

import numpy as np

import oracle
from quantizedsae_amd import synthetic as S
from sparsity_curve_util import gaussian, packed_dictionary, ranked_lists

__all__ = ["mono_key", "batch_select", "threshold_update", "threshold_select", "clamp_counts", "decode_ragged", "row_grad_ragged",
           "csr_ragged", "select_values", "SELECT_SHAPES", "SELECT_KINDS", "special_rows", "ragged_case", "RAGGED_CASES",
           "count_patterns"]


# ---- keys -------------------------------------------------------------------------------------------------------------
def mono_key(val) -> np.ndarray:
    """uint32, larger value -> larger key; every NaN 0xFFFFFFFF (above +inf); -0 == +0"""
    v = np.ascontiguousarray(val, dtype=np.float32)
    u = v.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(v)] = 0xFFFFFFFF
    return key


def _key_order(val) -> np.ndarray:
    """flat indices r K + j of val [B, K] in key order: mono_key descending, then row, then position"""
    key = mono_key(val).reshape(-1).astype(np.int64)
    return np.lexsort((np.arange(key.size), -key))          # (the flat index is row-major: row, then position)


def _outputs(val, sel):
    """counts, val_sel, report of a selected set ``sel`` (bool [B, K])"""
    val = np.ascontiguousarray(val, dtype=np.float32)
    B, K = val.shape
    counts = sel.sum(axis=1).astype(np.int32)
    val_sel = np.where(sel, val, np.float32(0.0)).astype(np.float32)
    bits = 0
    if sel.any():
        order = _key_order(val)
        last = order[sel.reshape(-1)[order]][-1]              # the last selected entry in key order
        bits = int(val.view(np.uint32).reshape(-1)[last])
    report = np.array([int(sel.sum()), int((counts == K).sum()), int((counts == 0).sum()), bits], dtype=np.int64)
    return counts, val_sel, report


def batch_select(val, n_select: int):
    """-> (counts int32 [B], val_sel fp32 [B, K], report int64 [4])"""
    val = np.ascontiguousarray(val, dtype=np.float32)
    assert 0 <= n_select <= val.size
    sel = np.zeros(val.size, dtype=bool)
    sel[_key_order(val)[:n_select]] = True
    return _outputs(val, sel.reshape(val.shape))


def threshold_update(theta, batches: int, report, lr):
    """-> (theta fp32, batches) after a batch with this report: the smallest selected value m moves theta when it is > 0"""
    theta, lr = np.float32(theta), np.float32(lr)
    if int(report[0]) == 0:
        return theta, int(batches)
    m = np.array([int(report[3])], dtype=np.uint32).view(np.float32)[0]
    if not m > 0:
        return theta, int(batches)
    if batches == 0:
        return m, 1
    with np.errstate(all="ignore"):
        diff = np.float32(m - theta)
        step = np.float32(lr * diff)
        return np.float32(theta + step), int(batches) + 1


def threshold_select(val, theta):
    """-> (counts, val_sel, report): row r keeps its longest prefix with val >= theta (a float compare)"""
    val = np.ascontiguousarray(val, dtype=np.float32)
    B, K = val.shape
    with np.errstate(invalid="ignore"):
        ok = val >= np.float32(theta)
    sel = np.logical_and.accumulate(ok, axis=1)
    return _outputs(val, sel)


def clamp_counts(counts, K: int) -> np.ndarray:
    return np.clip(np.asarray(counts, dtype=np.int64), 0, K).astype(np.int32)


# ---- ragged rows ------------------------------------------------------------------------------------------------------
def _decode(idx, val, decoder, bias):
    if decoder[0] == "packed":
        _, packed, D, n_bits, step = decoder
        return oracle.decode_binary(idx, val, packed, D, n_bits, step, bias)
    _, table, scale = decoder
    return oracle.decode_table(idx, val, table, scale, bias)


def decode_ragged(idx, val, counts, decoder, bias) -> np.ndarray:
    """-> fp32 [B, D]: the oracle's sparse decode of every row's first counts[r] entries (ids clamped into [0, H) as the sparse
    decoders do).  ``decoder`` = ("packed", packed uint8 [H, row_bytes], D, n_bits, step) or ("table", fp32 [H, D], scale)."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float32)
    B, K = idx.shape
    H = decoder[1].shape[0]
    D = decoder[2] if decoder[0] == "packed" else decoder[1].shape[1]
    c = clamp_counts(counts, K)
    idx = np.clip(idx, 0, H - 1)
    out = np.empty((B, D), dtype=np.float32)
    for n in np.unique(c):                                   # one oracle call per group of rows of equal count
        rows = np.nonzero(c == n)[0]
        out[rows] = _decode(np.ascontiguousarray(idx[rows, :n]), np.ascontiguousarray(val[rows, :n]), decoder, bias)
    return out


def _lane_columns(D: int):
    """columns of lane l in the order it walks them: 4 (l + 64 i) .. + 3"""
    D4 = D // 4
    return [np.concatenate([np.arange(4 * c, 4 * c + 4) for c in range(l, D4, 64)]) if l < D4 else np.zeros(0, np.int64)
            for l in range(64)]


def row_grad_ragged(idx, counts, table, step, g_recon, g_latent, W_enc):
    """-> (gv fp32 [B, K], dx fp32 [B, D] or None) in the kernels' order of operations (csrc/train_row.h): per entry the 64
    lanes' fmaf chains over their own columns, a butterfly of fp32 adds (xor 32, 16, .. 1), ``step *`` and ``g_latent +``
    rounded one by one; dx per column one fmaf chain over the row's entries in list order.  gv behind the prefix is +0."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.float32)
    B, K = idx.shape
    H, D = table.shape
    c = clamp_counts(counts, K)
    hh = np.clip(idx, 0, H - 1)
    cols = _lane_columns(D)
    width = max(1, max(len(x) for x in cols))
    lanes = np.arange(64)
    gv = np.zeros((B, K), dtype=np.float32)
    dx = np.zeros((B, D), dtype=np.float32) if W_enc is not None else None
    step = np.float32(step)
    for r in range(B):
        for j in range(int(c[r])):
            h = int(hh[r, j])
            v = np.float32(0.0)
            if g_recon is not None:
                a = np.zeros((64, width), dtype=np.float32)   # padding: fmaf(0, 0, acc) leaves acc (never -0) as it is
                t = np.zeros((64, width), dtype=np.float32)
                for l in range(64):
                    a[l, :len(cols[l])] = g_recon[r, cols[l]]
                    t[l, :len(cols[l])] = table[h, cols[l]]
                part = np.diagonal(oracle.encode(a, t)).astype(np.float32)
                for off in (32, 16, 8, 4, 2, 1):
                    part = (part + part[lanes ^ off]).astype(np.float32)
                v = np.float32(step * part[0])
            if g_latent is not None:
                v = np.float32(np.float32(g_latent[r, h]) + v)
            gv[r, j] = v
        if dx is not None and c[r] > 0:
            n = int(c[r])
            dx[r] = oracle.encode(gv[r:r + 1, :n], np.ascontiguousarray(np.asarray(W_enc, dtype=np.float32)[hh[r, :n]].T))[0]
    return gv, dx


def csr_ragged(idx, counts, H: int):
    """-> (offsets int32 [H + 1], entries int32 [B K]): entries r K + j with j < counts[r] and 0 <= idx < H grouped by unit,
    ordered by row within a unit; behind offsets[H] the entries are -1"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    B, K = idx.shape
    c = clamp_counts(counts, K)
    keep = (np.arange(K)[None, :] < c[:, None]) & (idx >= 0) & (idx < H)
    flat = np.nonzero(keep.reshape(-1))[0]
    units = idx.reshape(-1)[flat]
    order = np.argsort(units, kind="stable")                 # flat order is row order: stable keeps it within a unit
    entries = np.full(B * K, -1, dtype=np.int32)
    entries[:flat.size] = flat[order]
    offsets = np.zeros(H + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(units, minlength=H))
    return offsets, entries


# ---- inputs of the selection ----------------------------------------------------------------------------------------------
#: (B, K) of the issue: one entry, one full row, odd sizes, more rows than a workgroup has waves, a K that is no multiple of 64,
#: and many histogram workgroups (1024 x 256 keys = 64 workgroups of 4096)
SELECT_SHAPES = [(1, 1), (1, 256), (3, 5), (70, 64), (257, 33), (1024, 256)]
SELECT_KINDS = ["gaussian", "eight_levels", "all_equal", "shared_high_bits", "special"]


def _sorted_rows(v: np.ndarray) -> np.ndarray:
    """every row non-increasing in mono_key (a stable sort: equal keys keep their order)"""
    order = np.argsort(-mono_key(v).astype(np.int64), axis=1, kind="stable")
    return np.ascontiguousarray(np.take_along_axis(v, order, axis=1))


def special_rows(K: int) -> np.ndarray:
    """one row of K values that holds NaN (two payloads), +-inf, +-0, denormals of both signs and ordinary numbers"""
    pool = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF,
                     0x3F800000, 0xBF800000, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)
    return np.resize(pool, K).view(np.float32)


def select_values(kind: str, B: int, K: int, seed: int = 0) -> np.ndarray:
    """fp32 [B, K], every row non-increasing in mono_key"""
    g = S.normal(5000 + seed, (B, K), stream=67).astype(np.float32)
    if kind == "gaussian":
        v = g
    elif kind == "eight_levels":
        v = (np.floor(np.clip(g, -2, 1.99) * 2) / 2).astype(np.float32)     # -2, -1.5, .. 1.5: heavy ties
    elif kind == "all_equal":
        v = np.full((B, K), 0.75, dtype=np.float32)
    elif kind == "shared_high_bits":
        i = (np.abs(g) * 1000).astype(np.int64) % 4096       # 1 + i 2^-23: the keys differ in their low 12 bits only
        v = (np.uint32(0x3F800000) + i.astype(np.uint32)).view(np.float32)
    elif kind == "special":
        v = g.copy()
        for r in range(0, B, 3):
            v[r] = np.roll(special_rows(K), r)
    else:
        raise ValueError(kind)
    return _sorted_rows(np.ascontiguousarray(v, dtype=np.float32))


# ---- inputs of the ragged row operations ------------------------------------------------------------------------------------
#: name -> (decoder kind, D, n_bits or scale, bias, B, K, H)
RAGGED_CASES = {}
for _D in (4, 48, 516):
    for _n in (1, 4, 8):
        RAGGED_CASES[f"packed_D{_D}_n{_n}"] = ("packed", _D, _n, True, 9, 12, 512)
    RAGGED_CASES[f"table_D{_D}"] = ("table", _D, 1.0, True, 9, 12, 512)
RAGGED_CASES["table_D48_s0.5_nobias_H8"] = ("table", 48, 0.5, False, 9, 7, 8)
RAGGED_CASES["packed_D48_n4_H8"] = ("packed", 48, 4, True, 9, 7, 8)
RAGGED_CASES["table_D48_K256"] = ("table", 48, 1.0, True, 5, 256, 512)
RAGGED_CASES["packed_D48_n4_K256"] = ("packed", 48, 4, False, 5, 256, 512)


def count_patterns(B: int, K: int):
    """name -> counts int32 [B]: all 0, all K, mixed (with a 0, a K and a 1), and values outside [0, K] for the clamp"""
    mixed = (np.arange(B) * 5 + 1) % (K + 1)
    mixed[0], mixed[B - 1] = 0, K
    if B > 2:
        mixed[1] = 1
    outside = mixed.copy()
    outside[0], outside[B - 1] = -3, K + 1000
    if B > 3:
        outside[2] = np.iinfo(np.int32).min
        outside[3] = np.iinfo(np.int32).max
    return {"none": np.zeros(B, np.int32), "all": np.full(B, K, np.int32), "mixed": mixed.astype(np.int32),
            "outside": outside.astype(np.int32)}


def ragged_case(name: str):
    """-> (idx, val, decoder (host form), bias or None, H).  Row 0 holds an id below 0 and one at H (clamped by the decode and
    the row gradient, dropped by the lists)."""
    kind, D, par, with_bias, B, K, H = RAGGED_CASES[name]
    seed = 6000 + sorted(RAGGED_CASES).index(name)
    idx, val = ranked_lists(seed + 1, B, min(K, H), H)
    if K > H:                                                # more list places than units: ids repeat across the tail
        idx = np.concatenate([idx, idx[:, :K - H]], axis=1)
        val = np.concatenate([val, val[:, :K - H] - 10], axis=1)
    idx = np.ascontiguousarray(idx[:, :K])
    val = np.ascontiguousarray(val[:, :K])
    if K >= 4:
        idx[0, 1], idx[0, 2] = -2, H
    bias = gaussian(seed + 2, 1, D)[0] if with_bias else None
    if kind == "packed":
        decoder = ("packed", packed_dictionary(seed + 3, H, D, par), D, par, 0.25)
    else:
        decoder = ("table", gaussian(seed + 3, H, D), par)
    return idx, val, decoder, bias, H
