"""The resampling kernels' own source, run on the CPU: csrc/resample.hip is compiled for the host against the stand-in
runtime of tests/emu (threads as lanes, real barriers, the integer atomics) and compared with the numpy restatement
of tests/resample_util.py at the shapes the GPU tests use, bit for bit, with guard bytes around every buffer and the outputs
and the workspace poisoned.  This checks what a GPU-less machine can: indexing and tails, the order of every sum, the
three levels of the prefix sum, the binary search and the owner rule, the strided decoder column and the bit layout of the
logit row, and that nothing but the stated positions is written.  The source compiles for the host as it stands (no
multiply-add is contracted: -ffp-contract=off, as in the library's build)."""
import numpy as np
import pytest

import resample_util as U
from emu_util import CSRC, compile_emu, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_emu")
    src = (CSRC / "resample.hip").read_text()
    assert src.count('#include "common.h"') == 1
    (d / "resample_emu.hip").write_text(src.replace('#include "common.h"', f'#include "{CSRC / "common.h"}"'))
    exe = compile_emu(d, "resample_emu.cpp", "resample_emu", include=(d,))

    def run(head, arrays):
        head = list(head) + [0] * (8 - len(head))
        (d / "in.bin").write_bytes(np.array(head, np.int64).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
        run_emu(exe, ["in.bin", "out.bin"], d, 600)
        return (d / "out.bin").read_bytes()
    return run


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("shape", U.ROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_weights_source_on_the_host(emu, shape):
    N, D, ld = shape
    x, recon = U.rows_case(N, D, ld)
    w = np.frombuffer(emu([0, N, D, ld], [x, recon]), np.float64)
    want = U.row_weights(x[:, :D], recon[:, :D])
    _same(w, want)
    if N >= 8:
        assert (w[[1, 2, 3, 4, 6]] == 0).all() and np.isfinite(w[5]) and w[5] > 1e150 and (w[7:] > 0).all()


def _draw(emu, w, u):
    raw = emu([1, w.size, u.size], [w, u])
    return np.frombuffer(raw[:4 * u.size], np.int32), np.frombuffer(raw[4 * u.size:], np.int64)


@pytest.mark.parametrize("case", [(1, 1), (1029, 67), (70001, 1000)], ids=lambda c: f"N{c[0]}_n{c[1]}")
def test_draw_source_on_the_host(emu, case):
    N, n = case
    w = U.weights_case(N, zeros=N > 1)
    if N == 1:
        w[0] = 2.5
    u = U.uniforms(n)
    rows, report = _draw(emu, w, u)
    want_rows, want_report = U.draw(w, u)
    _same(rows, want_rows)
    _same(report, want_report)
    drawn = rows[rows >= 0]
    assert (w[drawn] > 0).all() and np.unique(drawn).size == drawn.size       # no zero-weight row, no row twice
    assert rows[0] == np.flatnonzero(w > 0)[0]                                  # u = 0: the first row with weight


def test_draw_without_weight_and_with_three_rows(emu):
    rows, report = _draw(emu, np.zeros(1029), U.uniforms(67))
    assert (rows == U.NO_ROW).all() and report.tolist() == [67, 0, 0, 0, 67, 0, 0, 0]
    w = np.zeros(1029)
    w[[5, 500, 1028]] = 1.0, 2.0, 3.0
    u = U.uniforms(67, seed=3)
    rows, report = _draw(emu, w, u)
    want_rows, want_report = U.draw(w, u)
    _same(rows, want_rows)
    _same(report, want_report)
    kept = np.flatnonzero(rows >= 0)
    assert 1 <= kept.size <= 3 and report[U.DUPLICATE] == 67 - kept.size and rows[0] == 5 and rows[66] == U.LOST_ROW
    raw = np.array([int(np.argmax(U.prefix_sum(w) > t)) if t < 6.0 else 1028 for t in u * 6.0])
    for j in kept:                                                            # the owner is the lowest j that drew the row
        assert j == np.flatnonzero(raw == rows[j])[0]


@pytest.mark.parametrize("H", [4, 1000])
def test_alive_stats_source_on_the_host(emu, H):
    D, nb = 36, 4
    W, _, logits, _ = U.model_case(H, D, nb)
    for dead in (np.zeros(0, np.int32), np.array([0, H - 1], np.int32), np.arange(H, dtype=np.int32)):
        for with_logits in ((True, False) if dead.size == 2 else (True,)):
            raw = emu([2, H, D, nb if with_logits else 0, dead.size], [W, logits if with_logits else np.zeros(0, np.float32), dead])
            _same(np.frombuffer(raw, np.float64), U.alive_stats(W, logits if with_logits else None, dead))


def _write(emu, c, *, moments=True, last=True, logit_scale=None, encoder_scale=0.2, rows_seen=4242):
    nb = c["n_bits"] or 0
    flags = (1 if moments else 0) | (2 if last else 0) | (4 if logit_scale is not None else 0)
    scales = np.array([encoder_scale, logit_scale if logit_scale is not None else 0.0], np.float64)
    raw = emu([3, c["H"], c["D"], nb, c["dead"].size, c["N"], flags, rows_seen],
              [c["dead"], c["rows"], c["x"], c["dec_bias"], c["stats"], scales, c["W_enc"], c["b_enc"], c["dec"], *c["moments"],
               c["last"], c["report"]])
    want = U.write(c["dead"], c["rows"], c["x"], c["dec_bias"], c["stats"], c["W_enc"], c["b_enc"], c["dec"], c["report"],
                   n_bits=c["n_bits"], moments=c["moments"] if moments else None, last=c["last"] if last else None,
                   rows_seen=rows_seen, encoder_scale=encoder_scale, logit_scale=logit_scale)
    at = 0
    expect = [want["W_enc"], want["b_enc"], want["dec"]] + [m if moments else c["moments"][i] for i, m in enumerate(want["moments"])] \
        + [want["last"] if last else c["last"], want["report"]]
    for e in expect:
        _same(np.frombuffer(raw[at:at + e.nbytes], e.dtype).reshape(e.shape), e)
        at += e.nbytes
    assert at == len(raw)
    return want


@pytest.mark.parametrize("n_bits", [None, 1, 4, 8], ids=lambda b: f"bits{b}")
@pytest.mark.parametrize("shape", U.WRITE_SHAPES, ids=lambda s: f"H{s[0]}_D{s[1]}")
def test_write_source_on_the_host(emu, shape, n_bits):
    H, D = shape
    c = U.write_case(H, D, n_bits)
    want = _write(emu, c)
    n = c["dead"].size
    assert want["report"].tolist()[:6] == [n, n - 3, 1, 1, 1, 0]
    # what the restatement leaves alone, the kernel leaves alone: rows of units that are not revived keep their bits
    revived = [int(h) for j, h in enumerate(c["dead"]) if j not in (1, 2, 3)]
    others = np.setdiff1d(np.arange(H), revived)
    assert want["W_enc"][others].tobytes() == c["W_enc"][others].tobytes()
    assert (want["moments"][0][revived] == 0).all() and want["moments"][0][others].tobytes() == c["moments"][0][others].tobytes()
    assert (want["last"][revived] == 4242).all() and (want["last"][others] == c["last"][others]).all()
    _write(emu, c, moments=False, last=False, logit_scale=2.5 if n_bits else None)


@pytest.mark.parametrize("n_bits", [None, 8], ids=lambda b: f"bits{b}")
def test_write_source_at_the_largest_row(emu, n_bits):
    _write(emu, U.write_case(4, 4096, n_bits, n=2))


def test_out_of_order_and_out_of_range_entries_are_skipped(emu):
    c = U.write_case(1000, 36, 4)
    c["dead"] = np.array([5, 5, 1000, -1, 7, 6, 999], np.int32)               # repeated, too large, negative, descending
    c["rows"] = np.array([0, 1, 2, 3, 4, 5, c["N"]], np.int32)                # ... and a row past the batch
    c["x"] = np.random.default_rng(9).standard_normal(c["x"].shape).astype(np.float32)
    want = _write(emu, c)
    assert want["report"][U.SKIPPED] == 5 and want["report"][U.REVIVED] == 2
