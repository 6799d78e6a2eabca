"""The numpy restatement of include/qsae_batch_dense.h, written from the header: oracle.encode for the pre-activations, the
candidates above the floor in the library's rank order (tests/jump_dense_util.py), the batch-wide selection of
tests/batch_topk_util.py over them, the certificate and the second attempt, the eight report words, the threshold state and the
next floor.  Shared by tests/test_batch_dense_host.py and tests/test_batch_dense_gpu.py; no GPU, no library but the oracle."""
import numpy as np

import batch_topk_util as BT
import jump_dense_util as JD

REPORT_WORDS = 8
REPORT_NAMES = ("selected", "saturated_rows", "empty_rows", "min_selected_bits", "candidates", "second_attempt", "rows_over_cap",
                "floor_bits")
NAMES = ("idx_sel", "val_sel", "counts", "report")

bits = JD.bits
preact = JD.preact
operands = JD.operands


def f32_bits(v) -> int:
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def bits_f32(b) -> np.float32:
    return np.array([int(b) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]


def candidates(z, floor, K):
    """-> (idx int32 [B, K], val fp32 [B, K], n int64 [B]): per row the units with z > floor (``floor`` None: every z that is
    not a NaN) in rank order, the first K of them; n the uncapped number"""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        keep = ~np.isnan(z) if floor is None else z > np.float32(floor)
    return JD.ranked_lists(z, keep, K, True)


def select_ragged(val, cand, n_select):
    """batch_topk_util.batch_select over the first cand[r] entries of every row (all of them when fewer than n_select)"""
    val = np.ascontiguousarray(val, np.float32)
    B, K = val.shape
    valid = (np.arange(K)[None, :] < np.asarray(cand)[:, None]).reshape(-1)
    flat = np.flatnonzero(valid)
    key = BT.mono_key(val).reshape(-1)[flat].astype(np.int64)
    order = flat[np.lexsort((flat, -key))]                     # mono_key descending, then row, then position
    sel = np.zeros(B * K, dtype=bool)
    sel[order[:n_select]] = True
    return BT._outputs(np.where(valid.reshape(B, K), val, np.float32(0.0)), sel.reshape(B, K))


def encode_batch_topk_from_z(z, K, n_select, floor, floor_ratio=1.0, floor_dev=False, theta=None, batches=0, lr=0.0):
    """-> (idx_sel, val_sel, counts, report int64 [8], (theta, batches, floor) after the call)"""
    z = np.asarray(z, np.float32)
    idx, val, n1 = candidates(z, floor, K)
    cand1 = np.minimum(n1, K)
    second = int(cand1.sum()) < int(n_select)
    cand = cand1
    if second:
        idx, val, n2 = candidates(z, None, K)
        cand = np.minimum(n2, K)
    counts, val_sel, rep = select_ragged(val, cand, int(n_select))
    idx_sel = np.where(np.arange(K)[None, :] < counts[:, None], idx, np.int32(-1)).astype(np.int32)
    report = np.array(rep.tolist() + [int(cand1.sum()), int(second), int((n1 > K).sum()), f32_bits(floor)], dtype=np.int64)
    new_theta, new_batches = (theta, batches)
    if theta is not None:
        new_theta, new_batches = BT.threshold_update(theta, batches, rep, lr)
    new_floor = np.float32(floor)
    m = bits_f32(rep[3])
    if floor_dev and int(rep[0]) > 0 and m > 0:
        new_floor = np.float32(np.float32(floor_ratio) * m)
    return idx_sel, val_sel, counts, report, (new_theta, new_batches, new_floor)


def encode_batch_topk(x, W, bias, K, n_select, floor, **kw):
    """qsaebd_encode_batch_topk, restated"""
    return encode_batch_topk_from_z(preact(x, W, bias), K, n_select, floor, **kw)


def capped_reference_from_z(z, K, n_select):
    """What the header promises for every floor (no NaN in z): batch_topk_util.batch_select on the rows' top-K lists
    -> (idx_sel, val_sel, counts, report int64 [4])"""
    z = np.asarray(z, np.float32)
    assert not np.isnan(z).any()
    idx, val, _ = JD.ranked_lists(z, np.ones(z.shape, bool), K, True)
    counts, val_sel, rep = BT.batch_select(val, int(n_select))
    idx_sel = np.where(np.arange(K)[None, :] < counts[:, None], idx, np.int32(-1)).astype(np.int32)
    return idx_sel, val_sel, counts, rep


def smallest_selected(z, K, n_select) -> np.float32:
    """m of the batch, from the capped reference"""
    return bits_f32(capped_reference_from_z(z, K, n_select)[3][3])


def rows_resolved(z, floor, cap=64, row_max=512, tile=128, target=512, max_splits=8):
    """The rows of attempt one that the row kernel cannot take from the regions (csrc/batch_dense.hip: a (split, row) region
    holds ``cap`` records, a row ``row_max``; the units are split as bd_plan splits them) -> bool [B]"""
    z = np.asarray(z, np.float32)
    B, H = z.shape
    tiles_q, tiles_c = -(-B // tile), -(-H // tile)
    want = min(-(-target // tiles_q), max_splits, tiles_c)
    sweep = -(-tiles_c // want)
    splits = -(-tiles_c // sweep)
    with np.errstate(invalid="ignore"):
        keep = z > np.float32(floor)
    over = keep.sum(axis=1) > row_max
    for s in range(splits):
        over |= keep[:, s * sweep * tile:(s + 1) * sweep * tile].sum(axis=1) > cap
    return over
