"""The resampling feature's host surface; runs without a GPU: the six C-ABI symbols and their argument checks, the dispatcher
schemas, known answers of the numpy restatement (tests/resample_util.py) worked out by hand, and the Trainer's new
constructor arguments."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import resample_util as U
import quantizedsae_amd
from quantizedsae_amd import _lib, training
from quantizedsae_amd import torch_ops  # noqa: F401  (registers torch.ops.qsae.*)
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE, TernarySparseAutoencoder
from quantizedsae_amd.training import ResampleReport, Trainer, resample_dead

ROOT = Path(__file__).resolve().parents[1]
P = ctypes.c_void_p
NEW = ("qsae_resample_row_weights", "qsae_resample_draw_workspace_bytes", "qsae_resample_draw", "qsae_resample_alive_stats",
       "qsae_resample_write_table", "qsae_resample_write_binary")
OPS = ("resample_row_weights", "resample_draw", "resample_alive_stats", "resample_write_table", "resample_write_binary")
A = 4096                                                   # a well aligned address that is never dereferenced


def test_symbols_are_declared_bound_and_exported_by_both_libraries_and_the_abi_version_stays():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = ctypes.CDLL(str(path))
        for name in NEW:
            assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, (path.name, name)
    assert _lib.load().qsae_abi_version() == _lib.ABI_VERSION == 4
    assert "resample.hip" in __import__("quantizedsae_amd.build", fromlist=["SOURCES"]).SOURCES
    for name in ("resample_dead", "ResampleReport"):
        assert name in training.__all__ and hasattr(training, name)
    ops = quantizedsae_amd.ops
    assert (ops.RESAMPLE_MAX_D, ops.RESAMPLE_REPORT_WORDS) == (U.MAX_D, U.REPORT_WORDS)
    for name in OPS:
        assert hasattr(ops, name) and hasattr(torch_ops, name) and hasattr(torch.ops.qsae, name)


def test_the_library_is_built_without_contracting_multiply_adds():
    from quantizedsae_amd import build
    assert "-ffp-contract=off" in build.FLAGS                # the restatement has a product and a sum where the kernel has


def test_workspace_bytes():
    lib = _lib.load()
    for N in (0, -1, -(2 ** 31)):
        assert lib.qsae_resample_draw_workspace_bytes(N) == 0
    for N in (1, 1000, 1024, 1025, 70001, 2 ** 31 - 1):
        assert lib.qsae_resample_draw_workspace_bytes(N) == U.draw_workspace_bytes(N), N
    assert U.draw_workspace_bytes(1) == 768 and U.draw_workspace_bytes(1024) == 8192 + 256 + 4096
    assert U.draw_workspace_bytes(70001) == 560128 + 768 + 280064


def _weights(lib, x=P(A), ldx=8, recon=P(A), ldr=8, N=4, D=8, w=P(A)):
    return lib.qsae_resample_row_weights(x, ldx, recon, ldr, N, D, w, None)


def _draw(lib, w=P(A), N=4, u=P(A), n=2, rows=P(A), report=P(A), ws=P(A), ws_bytes=1 << 20):
    return lib.qsae_resample_draw(w, N, u, n, rows, report, ws, ws_bytes, None)


def _alive(lib, W=P(A), H=10, D=8, logits=P(A), n_bits=4, dead=P(A), n=2, unit_norm=P(A), unit_abs=P(A), stats=P(A)):
    return lib.qsae_resample_alive_stats(W, H, D, logits, n_bits, dead, n, unit_norm, unit_abs, stats, None)


def _write(lib, binary, dead=P(A), rows=P(A), n=2, x=P(A), ldx=8, N=4, D=8, H=10, n_bits=4, bias=P(A), stats=P(A), scale=0.2,
           W=P(A), b=P(A), dec=P(A), m=(None,) * 6, last=None, rows_seen=0, report=P(A)):
    if binary:
        return lib.qsae_resample_write_binary(dead, rows, n, x, ldx, N, D, H, n_bits, bias, stats, scale, 0, 0.0, W, b, dec, *m, last,
                                              rows_seen, report, None)
    return lib.qsae_resample_write_table(dead, rows, n, x, ldx, N, D, H, bias, stats, scale, W, b, dec, *m, last, rows_seen, report,
                                         None)


def test_invalid_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    bad, uns = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    # row weights
    assert _weights(lib, N=-1) == bad and b"invalid argument" in lib.qsae_last_error()
    assert b"qsae_resample_row_weights" in lib.qsae_last_error()
    assert _weights(lib, D=0) == bad and _weights(lib, ldx=7) == bad and _weights(lib, ldr=4) == bad
    assert _weights(lib, D=6, ldx=6, ldr=6) == uns and b"unsupported" in lib.qsae_last_error()
    assert _weights(lib, D=4100, ldx=4100, ldr=4100) == uns and _weights(lib, D=4096, ldx=4096, ldr=4096, x=None) == bad
    assert _weights(lib, x=None) == bad and _weights(lib, recon=None) == bad and _weights(lib, w=None) == bad
    assert _weights(lib, x=P(A + 2)) == bad and _weights(lib, recon=P(A + 1)) == bad and _weights(lib, w=P(A + 4)) == bad
    # draw
    assert _draw(lib, N=0) == bad and _draw(lib, N=-3) == bad and _draw(lib, n=-1) == bad
    assert _draw(lib, w=None) == bad and _draw(lib, u=None) == bad and _draw(lib, rows=None) == bad and _draw(lib, report=None) == bad
    assert _draw(lib, w=P(A + 4)) == bad and _draw(lib, u=P(A + 4)) == bad and _draw(lib, rows=P(A + 2)) == bad
    assert _draw(lib, report=P(A + 4)) == bad
    assert _draw(lib, ws=None) == _lib.ERR_WORKSPACE and _draw(lib, ws_bytes=767) == _lib.ERR_WORKSPACE
    assert b"qsae_resample_draw_workspace_bytes" in lib.qsae_last_error()
    assert _draw(lib, ws=P(A + 4)) == _lib.ERR_WORKSPACE and _draw(lib, N=70001, ws_bytes=840959) == _lib.ERR_WORKSPACE
    # alive stats
    assert _alive(lib, H=0) == bad and _alive(lib, D=0) == bad and _alive(lib, D=10) == uns and _alive(lib, D=8192) == uns
    assert _alive(lib, n=-1) == bad and _alive(lib, n=11) == bad                        # more dead units than units
    assert _alive(lib, n_bits=0) == bad and _alive(lib, n_bits=9) == bad
    assert _alive(lib, W=None) == bad and _alive(lib, dead=None) == bad and _alive(lib, stats=None) == bad
    assert _alive(lib, unit_norm=None) == bad and _alive(lib, unit_abs=None) == bad     # logits without unit_abs
    assert _alive(lib, W=P(A + 2)) == bad and _alive(lib, logits=P(A + 2)) == bad and _alive(lib, dead=P(A + 1)) == bad
    assert _alive(lib, unit_norm=P(A + 4)) == bad and _alive(lib, stats=P(A + 4)) == bad
    # both writes
    for binary in (False, True):
        w = lambda **kw: _write(lib, binary, **kw)  # noqa: E731
        assert w(n=-1) == bad and w(N=0) == bad and w(H=0) == bad and w(D=0) == bad and w(ldx=7) == bad and w(rows_seen=-1) == bad
        assert w(n=11) == bad and b"more dead units than units" in lib.qsae_last_error()
        assert w(D=6, ldx=6) == uns and w(D=4100, ldx=4100) == uns
        for name in ("dead", "rows", "x", "bias", "stats", "W", "b", "dec", "report"):
            assert w(**{name: None}) == bad, name
        for name in ("dead", "rows", "x", "bias", "W", "b", "dec"):
            assert w(**{name: P(A + 2)}) == bad, name
        assert w(stats=P(A + 4)) == bad and w(report=P(A + 4)) == bad and w(last=P(A + 4)) == bad
        for i in range(6):
            assert w(m=tuple(P(A + 2) if k == i else None for k in range(6))) == bad
    assert _write(lib, True, n_bits=0) == bad and _write(lib, True, n_bits=9) == bad


def test_an_empty_dead_list_is_a_no_op_without_a_device():
    lib = _lib.load()
    assert _draw(lib, n=0) == _lib.OK and _draw(lib, n=0, w=None, u=None, rows=None, report=None, ws=None) == _lib.OK
    assert _weights(lib, N=0) == _lib.OK and _weights(lib, N=0, x=None, recon=None, w=None) == _lib.OK
    for binary in (False, True):
        assert _write(lib, binary, n=0) == _lib.OK
        assert _write(lib, binary, n=0, dead=None, rows=None, x=None, W=None, report=None) == _lib.OK
        assert _write(lib, binary, n=0, D=6, ldx=6) == _lib.ERR_UNSUPPORTED            # ... but not a licence for a bad shape
    model = BaselineSparseAutoencoder(8, 16)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    report = resample_dead(model, torch.zeros(0, dtype=torch.int32), torch.zeros((4, 8)))
    assert isinstance(report, ResampleReport) and report.block is None and report.revived == 0 and report.dead == 0
    assert report.metrics()["resampled_features"] == 0
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_op_schemas_declare_the_mutated_tensors():
    def written(op):
        return [a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    q = torch.ops.qsae
    want = ["W_enc", "b_enc", "dec", "report", "m_We", "v_We", "m_be", "v_be", "m_dec", "v_dec", "last"]
    assert written(q.resample_write_table) == want and written(q.resample_write_binary) == want
    assert written(q.resample_row_weights) == written(q.resample_draw) == written(q.resample_alive_stats) == []
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty((10, 8))
        w = q.resample_row_weights(x, x.clone())
        assert w.shape == (10,) and w.dtype == torch.float64
        rows, report = q.resample_draw(w, torch.empty(3, dtype=torch.float64))
        assert rows.shape == (3,) and rows.dtype == torch.int32 and report.shape == (U.REPORT_WORDS,) and report.dtype == torch.int64
        stats = q.resample_alive_stats(torch.empty((16, 8)), None, torch.empty(3, dtype=torch.int32), 8)
        assert stats.shape == (2,) and stats.dtype == torch.float64


def test_cpu_tensors_and_other_models_are_refused():
    ops = quantizedsae_amd.ops
    x = torch.zeros((4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_row_weights(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_draw(torch.ones(4, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_alive_stats(torch.zeros((16, 8)), None, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample_dead(BaselineSparseAutoencoder(8, 16), torch.zeros(2, dtype=torch.int32), x, u=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="TernarySparseAutoencoder"):
        resample_dead(TernarySparseAutoencoder(8, 16), torch.zeros(2, dtype=torch.int32), x)
    with pytest.raises(ValueError, match="generator"):                        # the default generator is never used
        resample_dead(BinarySAE(8, 512, 4), torch.zeros(2, dtype=torch.int32), x)
    with pytest.raises(ValueError, match="uniforms"):
        resample_dead(BinarySAE(8, 512, 4), torch.zeros(2, dtype=torch.int32), x, u=torch.zeros(3, dtype=torch.float64))


# ---- known answers of the restatement, by hand ----------------------------------------------------------------------------------
def test_block_sum_order_is_the_stated_one():
    # 513 values: partial 0 adds a[0], a[256], a[512] in that order; with 1, 2^53 and -2^53 the order decides the answer
    a = np.zeros(513)
    a[0], a[256], a[512] = 1.0, 2.0 ** 53, -(2.0 ** 53)
    assert U.block_sum(a) == 0.0                                  # (1 + 2^53) rounds to 2^53, then - 2^53
    a[0], a[256], a[512] = 2.0 ** 53, -(2.0 ** 53), 1.0
    assert U.block_sum(a) == 1.0
    # the fold: s[0] += s[128] comes first (k = 128), s[0] += s[1] last
    a = np.zeros(256)
    a[0], a[128], a[1] = 1.0, 2.0 ** 53, -(2.0 ** 53)
    assert U.block_sum(a) == 0.0
    assert U.block_sum(np.arange(1000.0)) == 499500.0 and U.block_sum(np.zeros((3, 0))).tolist() == [0.0, 0.0, 0.0]


def test_row_weights_by_hand():
    x = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0], [np.nan, 0, 0, 0], [3e38, 0, 0, 0]], np.float32)
    recon = np.array([[0.0, 0.0, 0.0, 2.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0, 0, 0], [-3e38, 0, 0, 0]], np.float32)
    w = U.row_weights(x, recon)
    assert w.tolist() == [(1.0 + 4.0 + 9.0 + 4.0) ** 2, 0.0, 0.0, 0.0]      # NaN and the fp32 overflow of 3e38 - -3e38: weight 0
    big = U.row_weights(np.array([[3e38, 0, 0, 0]], np.float32), np.zeros((1, 4), np.float32))[0]
    assert np.isfinite(big) and big == (float(np.float32(3e38)) ** 2) ** 2


def test_a_three_row_cdf_with_the_smallest_and_the_largest_uniform():
    w = np.array([0.0, 3.0, 0.0, 1.0, 0.0])
    assert U.prefix_sum(w).tolist() == [0.0, 3.0, 3.0, 4.0, 4.0]
    last = np.nextafter(1.0, 0.0)
    rows, report = U.draw(w, np.array([0.0, last]))
    assert rows.tolist() == [1, 3] and report.tolist() == [2, 0, 0, 0, 0, 0, 0, 0]           # never a row of weight 0
    rows, _ = U.draw(np.array([2.0, 1.0, 5.0]), np.array([0.0, 0.25, 0.2499, 0.375, last]))
    assert rows.tolist() == [0, 1, U.LOST_ROW, 2, U.LOST_ROW]     # cdf 2, 3, 8: 0.25 * 8 = 2 is not below cdf[0] = 2 -> row 1
    # u < 1 keeps u * total below the total in round-to-nearest; a u outside the contract still lands inside the batch, on the
    # row at which the cdf reaches the total
    w = np.array([1.0, 0.0, 2.0, 0.0])
    assert float(last * 3.0) < 3.0 and U.draw(w, np.array([last]))[0].tolist() == [2]
    assert U.draw(w, np.array([1.0]))[0].tolist() == [2] and U.draw(w, np.array([np.nan]))[0].tolist() == [2]
    rows, report = U.draw(np.zeros(4), np.array([0.0, 0.5]))
    assert rows.tolist() == [U.NO_ROW, U.NO_ROW] and report[U.NO_WEIGHT] == 2


def test_first_owner_on_a_repeated_draw():
    w = np.array([0.0, 1.0, 1.0])
    rows, report = U.draw(w, np.array([0.9, 0.1, 0.2, 0.6, 0.0]))
    assert rows.tolist() == [2, 1, U.LOST_ROW, U.LOST_ROW, U.LOST_ROW]
    assert report[U.DEAD] == 5 and report[U.DUPLICATE] == 3 and report[U.NO_WEIGHT] == 0


def test_quantized_direction_by_hand():
    v = np.array([1.0, -1.0, 0.5, -0.26], np.float32)
    assert U.quantize(v, 1).tolist() == [0, -1, 0, 0]             # qmax = 0: rint(v / 1) clamped to [-1, 0]; rint(0.5) = 0, to even
    assert U.quantize(v, 4).tolist() == [7, -7, 4, -2]            # 7, -7, rint(3.5) = 4 (to even), rint(-1.82) = -2
    assert U.quantize(v, 8).tolist() == [127, -127, 64, -33]      # rint(63.5) = 64 (to even), rint(-33.02) = -33
    assert U.quantize(np.array([-2.0, 1.0], np.float32), 4).tolist() == [-7, 4]     # the scale is max(qmax, 1) / max |v|: -8 is
    #                                                                                 reached by the clamp alone, never by it
    # the logit row: bit b of q & 15 at column 4 d + b, LSB first
    W, b, dec, bias = U.model_case(4, 4, 4)
    x = (bias + v)[None, :].astype(np.float32)
    vv = (x[0] - bias).astype(np.float32)
    out = U.write(np.array([2], np.int32), np.array([0], np.int32), x, bias, np.array([1.5, 3.0]), W, b, dec,
                  np.zeros(8, np.int64), n_bits=4)
    q = U.quantize(vv, 4)
    row = out["dec"][2].reshape(4, 4)
    for d in range(4):
        assert [1 if row[d, k] > 0 else 0 for k in range(4)] == [(int(q[d]) & 15) >> k & 1 for k in range(4)]
    assert (np.abs(out["dec"][2]) == np.float32(3.0)).all() and out["dec"][[0, 1, 3]].tobytes() == dec[[0, 1, 3]].tobytes()
    nrm = np.sqrt(np.sum(vv.astype(np.float64) ** 2))
    assert np.allclose(np.linalg.norm(out["W_enc"][2].astype(np.float64)), 0.2 * 1.5, rtol=1e-6) and out["b_enc"][2] == 0.0
    assert out["report"][U.REVIVED] == 1 and nrm > 0


def test_alive_stats_by_hand():
    W = np.zeros((4, 4), np.float32)
    W[0, 0], W[1, :2], W[2, 3], W[3] = 3.0, (3.0, 4.0), 10.0, (1.0, 1.0, 1.0, 1.0)
    logits = np.arange(32, dtype=np.float32).reshape(4, 8) - 16.0
    assert U.alive_stats(W, None, np.array([2], np.int32)).tolist() == [(3.0 + 5.0 + 2.0) / 3.0, 0.0]
    s = U.alive_stats(W, logits, np.array([0, 3], np.int32))
    assert s.tolist() == [(5.0 + 10.0) / 2.0, float(np.abs(logits[[1, 2]]).sum()) / 16.0]
    everything = U.alive_stats(W, logits, np.arange(4, dtype=np.int32))      # no unit alive: the mean over all of them
    assert everything.tolist() == [(3.0 + 5.0 + 10.0 + 2.0) / 4.0, float(np.abs(logits).sum()) / 32.0]


# ---- the Trainer's arguments -----------------------------------------------------------------------------------------------------
CONFIG = {"input_dim": 64, "n_bits": 4, "hidden_dim": 1024, "gamma": 1.5, "epochs": 1, "lr": 1e-4, "top_k": 32,
          "sparsity_lambda": 1.5e-3, "polarize_lambda": 1e-2, "batch_size": 64}


def test_trainer_accepts_and_validates_resample_every(tmp_path):
    t = Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path))
    assert t.resample_every is None and t.activity is None and "activity" not in t.model.__dict__
    assert not [k for k in t.model.__dict__ if "resample" in k]                 # None sets nothing on the model
    for bad in (0, -5):
        with pytest.raises(ValueError, match="resample_every"):
            Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), activity_window=100, resample_every=bad)
    with pytest.raises(ValueError, match="activity_window"):
        Trainer(CONFIG, "b_sae", False, True, dataset_dir=str(tmp_path), resample_every=4)
    for st in ("q_sae", "rq_sae", "bl_sae", "t_sae"):
        with pytest.raises(ValueError, match="baseline_sae and b_sae"):
            Trainer(CONFIG, st, st == "t_sae", True, dataset_dir=str(tmp_path), activity_window=100, resample_every=4)
    for st in ("baseline_sae", "b_sae"):
        t = Trainer(CONFIG, st, False, True, dataset_dir=str(tmp_path), activity_window=100, resample_every=4, resample_seed=7,
                    resample_scale=0.5)
        assert t.resample_every == 4 and t.resample_scale == 0.5 and t.model.activity is t.activity
        assert not [k for k in t.model.__dict__ if "resample" in k]

