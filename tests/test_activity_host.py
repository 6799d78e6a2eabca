"""The activity feature's host surface; runs without a GPU: the five C-ABI entry points and their argument checks, the
dispatcher schemas, known answers of the numpy restatement (tests/activity_util.py), the tracker's bookkeeping on the host
side, ``FeatureActivity.for_model`` and the Trainer's new constructor argument."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import activity_util as U
import quantizedsae_amd
from quantizedsae_amd import _lib, training
from quantizedsae_amd import torch_ops  # noqa: F401  (registers torch.ops.qsae.*)
from quantizedsae_amd.sae import (BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, ResidualQuantizedSAE,
                                  TernarySparseAutoencoder)
from quantizedsae_amd.sae.binary_latent import BinaryLatentSAE
from quantizedsae_amd.training import ActivitySummary, FeatureActivity, Trainer, activity_line
from quantizedsae_amd.training.activity import _parse

ROOT = Path(__file__).resolve().parents[1]
P = ctypes.c_void_p
NEW = ("qsae_activity_add_compact", "qsae_activity_add_bits", "qsae_activity_add_dense", "qsae_activity_summary_workspace_bytes",
       "qsae_activity_summary")
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
    assert "activity.hip" in __import__("quantizedsae_amd.build", fromlist=["SOURCES"]).SOURCES
    for name in ("FeatureActivity", "ActivitySummary", "activity_line"):
        assert name in training.__all__ and hasattr(training, name)
    ops = quantizedsae_amd.ops
    assert (ops.ACTIVITY_HEAD, ops.ACTIVITY_BINS, ops.ACTIVITY_MAX_SEGMENTS) == (U.HEAD, U.BINS, U.MAX_SEGMENTS)
    for name in ("activity_add_compact", "activity_add_bits", "activity_add_dense", "activity_summary"):
        assert hasattr(ops, name) and hasattr(torch_ops, name) and hasattr(torch.ops.qsae, name)


def test_workspace_bytes():
    lib = _lib.load()
    for H in (0, -1, -(2 ** 31)):
        assert lib.qsae_activity_summary_workspace_bytes(H) == 0
    for H in (1, 1000, 1024, 1025, 65536, 65537, 2 ** 31 - 1):
        assert lib.qsae_activity_summary_workspace_bytes(H) == U.workspace_bytes(H), H
    assert U.workspace_bytes(1) == 256 and U.workspace_bytes(65536) == 256 and U.workspace_bytes(65537) == 512


def _compact(lib, idx=P(A), val=P(A), B=4, k=3, H=10, stamp=1, fired=P(A), last=P(A)):
    return lib.qsae_activity_add_compact(idx, val, B, k, H, stamp, fired, last, None)


def _bits(lib, z=P(A), ld=2, B=4, nbits=64, index=P(A), H=50, stamp=1, fired=P(A), last=P(A)):
    return lib.qsae_activity_add_bits(z, ld, B, nbits, index, H, stamp, fired, last, None)


def _dense(lib, x=P(A), ld=16, B=4, H=10, stamp=1, fired=P(A), last=P(A)):
    return lib.qsae_activity_add_dense(x, ld, B, H, stamp, fired, last, None)


def _summary(lib, fired=P(A), base=P(A), last=P(A), H=100, clock=10, window=5, sizes=None, n_seg=None, advance=1, result=P(A),
             dead=P(A), ws=P(A), ws_bytes=1 << 20):
    arr = (ctypes.c_int32 * max(len(sizes), 1))(*sizes) if sizes is not None else None
    n_seg = (len(sizes) if sizes is not None else 0) if n_seg is None else n_seg
    return lib.qsae_activity_summary(fired, base, last, H, clock, window, arr, n_seg, advance, result, dead, ws, ws_bytes, None)


def test_invalid_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    bad, uns = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    # compact
    assert _compact(lib, B=-1) == bad and b"invalid argument" in lib.qsae_last_error()
    assert b"qsae_activity_add_compact" in lib.qsae_last_error()
    assert _compact(lib, k=0) == bad and _compact(lib, H=0) == bad and _compact(lib, H=-5) == bad
    assert _compact(lib, stamp=0) == bad and _compact(lib, stamp=-3) == bad
    assert _compact(lib, idx=None) == bad and _compact(lib, fired=None) == bad and _compact(lib, last=None) == bad
    assert _compact(lib, idx=P(A + 2)) == bad and _compact(lib, val=P(A + 1)) == bad
    assert _compact(lib, fired=P(A + 4)) == bad and _compact(lib, last=P(A + 4)) == bad
    assert _compact(lib, B=2 ** 16, k=2 ** 15) == uns and b"unsupported" in lib.qsae_last_error()
    assert _compact(lib, B=2 ** 31 - 1, k=2) == uns
    # bits
    assert _bits(lib, B=-1) == bad and _bits(lib, nbits=0) == bad and _bits(lib, H=0) == bad and _bits(lib, stamp=0) == bad
    assert _bits(lib, nbits=48) == uns and _bits(lib, nbits=33) == uns
    assert _bits(lib, ld=1) == bad                                               # words_ld < nbits / 32
    assert _bits(lib, index=None, H=63) == bad                                   # the identity needs nbits <= H
    assert _bits(lib, z=None) == bad and _bits(lib, fired=None) == bad and _bits(lib, last=None) == bad
    assert _bits(lib, z=P(A + 2)) == bad and _bits(lib, index=P(A + 2)) == bad and _bits(lib, fired=P(A + 4)) == bad
    # dense
    assert _dense(lib, B=-1) == bad and _dense(lib, H=0) == bad and _dense(lib, stamp=0) == bad
    assert _dense(lib, ld=9) == bad                                              # ld < H
    assert _dense(lib, x=None) == bad and _dense(lib, x=P(A + 2)) == bad
    assert _dense(lib, fired=None) == bad and _dense(lib, last=P(A + 4)) == bad
    # summary
    assert _summary(lib, H=0) == bad and _summary(lib, window=0) == bad and _summary(lib, clock=-1) == bad
    assert _summary(lib, fired=None) == bad and _summary(lib, last=None) == bad and _summary(lib, result=None) == bad
    assert _summary(lib, fired=P(A + 4)) == bad and _summary(lib, base=P(A + 4)) == bad and _summary(lib, result=P(A + 4)) == bad
    assert _summary(lib, dead=P(A + 2)) == bad
    assert _summary(lib, sizes=[50, 49]) == bad and _summary(lib, sizes=[50, 51]) == bad and _summary(lib, sizes=[101, -1]) == bad
    assert _summary(lib, sizes=[100] + [0] * 16) == bad                          # 17 segments
    assert _summary(lib, n_seg=2) == bad and _summary(lib, sizes=[100], n_seg=-1) == bad
    assert _summary(lib, ws=None) == _lib.ERR_WORKSPACE and _summary(lib, ws_bytes=255) == _lib.ERR_WORKSPACE
    assert b"qsae_activity_summary_workspace_bytes" in lib.qsae_last_error()
    assert _summary(lib, H=65537, ws_bytes=256) == _lib.ERR_WORKSPACE


def test_an_empty_batch_is_a_no_op_without_a_device():
    lib = _lib.load()
    assert _compact(lib, B=0) == _lib.OK and _compact(lib, B=0, idx=None, val=None, fired=None, last=None) == _lib.OK
    assert _bits(lib, B=0) == _lib.OK and _bits(lib, B=0, z=None, index=None, H=64, fired=None, last=None) == _lib.OK
    assert _dense(lib, B=0) == _lib.OK and _dense(lib, B=0, x=None, fired=None, last=None) == _lib.OK
    # ... but not a licence for a bad shape
    assert _compact(lib, B=0, k=0) == _lib.ERR_INVALID_ARG and _bits(lib, B=0, nbits=40) == _lib.ERR_UNSUPPORTED
    t = FeatureActivity(8, "cpu")
    t.add_compact(torch.zeros((0, 3), dtype=torch.int32), None)
    t.add_bits(torch.zeros((0, 1), dtype=torch.int32))
    t.add_dense(torch.zeros((0, 8)))
    assert t.rows_seen == 0 and not t.fired.any() and not t.last.any()


def test_op_schemas_declare_the_mutated_state():
    def written(op):
        return [a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    q = torch.ops.qsae
    assert written(q.activity_add_compact) == written(q.activity_add_bits) == written(q.activity_add_dense) == ["fired", "last"]
    assert written(q.activity_summary) == ["base", "dead_out"]
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        s = torch.empty(10, dtype=torch.int64)
        out = q.activity_summary(s, s.clone(), s.clone(), 5, 2, [4, 6], True, None)
        assert out.shape == (3, U.WORDS) and out.dtype == torch.int64


def test_cpu_tensors_are_refused():
    s = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FeatureActivity(8, "cpu").add_compact(torch.zeros((2, 3), dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quantizedsae_amd.ops.activity_summary(s, None, s, 1, 1)


# ---- known answers of the restatement -------------------------------------------------------------------------------------------
def test_octave_bins():
    want = {0: 0, 1: 1, 2: 2, 3: 2, 4: 3, 7: 3, 8: 4, 2 ** 32 - 1: 32, 2 ** 32: 33, 2 ** 33: 33, 2 ** 40: 33, 2 ** 62: 33}
    for c, b in want.items():
        assert U.octave_bin(c) == b, c
    fired = np.array(list(want), np.int64)
    res, _ = U.summary(fired, None, np.ones_like(fired), clock=1, window=5)
    bins = res[0, U.HEAD:]
    assert bins.sum() == len(want) and bins.tolist()[:5] == [1, 1, 2, 2, 1] and bins[32] == 1 and bins[33] == 4
    assert res[0, U.MAX_INTERVAL] == 2 ** 62 and res[0, U.SILENT] == 1 and res[0, U.SUM_FIRED] == int(fired.sum())


def test_the_window_edge_and_never_fired_units():
    W, clock = 100, 1000
    last = np.array([clock - W, clock - W + 1, clock, 0, 1], np.int64)           # == W: dead; W - 1: not; now; never; long ago
    fired = np.array([3, 3, 3, 0, 1], np.int64)
    res, dead = U.summary(fired, fired.copy(), last, clock, W)
    assert dead.tolist() == [0, 3, 4] and res[0, U.DEAD] == 3 and res[0, U.NEVER] == 1 and res[0, U.SILENT] == 5
    # a never-fired unit is dead once clock >= W, not before; before that nothing is dead
    never = np.zeros(3, np.int64)
    assert U.summary(never, None, never, W - 1, W)[0][0, U.DEAD] == 0
    assert U.summary(never, None, never, W, W)[0][0, U.DEAD] == 3
    assert U.summary(never, None, never, W - 1, W)[0][0, U.NEVER] == 3
    early = np.array([1, 5, 0], np.int64)
    assert U.summary(np.array([1, 1, 0], np.int64), None, early, 5, 100)[0][0, U.DEAD] == 0


def test_restatement_of_the_three_adds():
    H = 6
    z, one = np.zeros(H, np.int64), np.int64(1)
    idx = np.array([[0, 0, 5], [-1, 6, 2]], np.int32)
    val = np.array([[1.0, 2.0, np.nan], [1.0, 1.0, -0.0]], np.float32)
    f, l = U.add_compact(idx, val, H, 7, z, z)
    assert f.tolist() == [2, 0, 0, 0, 0, 0] and l.tolist() == [7, 0, 0, 0, 0, 0]          # listed twice: counted twice
    f, l = U.add_compact(idx, None, H, 3, f, l)
    assert f.tolist() == [4, 0, 1, 0, 0, 1] and l.tolist() == [7, 0, 3, 0, 0, 3]          # a smaller stamp never lowers last
    bits = np.array([[0b101], [0b100]], np.uint32)
    index = np.full(32, -1, np.int32)
    index[0], index[2] = 4, 1
    f, l = U.add_bits(bits, 32, index, H, 9, z, z)
    assert f.tolist() == [0, 2, 0, 0, 1, 0] and l.tolist() == [0, 9, 0, 0, 9, 0]
    x = np.array([[np.nan, -0.0, np.inf, 1e-45, -1.0, 0.0]], np.float32)
    f, l = U.add_dense(x, H, 2, z, z)
    assert f.tolist() == [0, 0, 1, 1, 0, 0] and l.tolist() == [0, 0, 2, 2, 0, 0]


def test_segments_of_the_restatement_add_up():
    fired, base, last = U.state_case(1000)
    assert (base <= fired).all()
    res, dead = U.summary(fired, base, last, 5000, 700, [37, 300, 1, 662])
    assert res[1:, :U.MAX_INTERVAL].sum(0).tolist() == res[0, :U.MAX_INTERVAL].tolist()
    assert res[1:, U.HEAD:].sum(0).tolist() == res[0, U.HEAD:].tolist() and res[1:, U.MAX_INTERVAL].max() == res[0, U.MAX_INTERVAL]
    assert res[:, U.UNITS].tolist() == [1000, 37, 300, 1, 662] and res[0, U.DEAD] == dead.size and (np.diff(dead) > 0).all()


# ---- the tracker, for_model and the Trainer's argument ----------------------------------------------------------------------------
def test_summary_parsing_and_the_printed_line():
    fired, base, last = U.state_case(300)
    res, _ = U.summary(fired, base, last, 5000, 700, [100, 200])
    blocks = _parse(torch.from_numpy(res), 64)
    s = blocks[0]
    s.levels = blocks[1:]
    assert isinstance(s, ActivitySummary) and (s.units, s.dead, s.never, s.silent) == tuple(res[0, [0, 2, 1, 3]].tolist())
    assert s.interval_rows == 64 and s.interval_count == res[0, U.SUM_INTERVAL] and s.mean_l0 == res[0, U.SUM_INTERVAL] / 64
    assert s.octaves == res[0, U.HEAD:].tolist() and len(s.octaves) == 34 and s.dead_fraction == s.dead / 300
    line = activity_line(s)
    assert line.startswith(f"  activity: dead={s.dead}/300") and f"never_fired={s.never}" in line and "dead_per_level=[" in line
    assert _parse(torch.from_numpy(res), 0)[0].mean_l0 == 0.0


def test_tracker_bookkeeping_and_state_dict():
    with pytest.raises(ValueError):
        FeatureActivity(0, "cpu")
    with pytest.raises(ValueError, match="level_sizes"):
        FeatureActivity(10, "cpu", [4, 5])
    with pytest.raises(ValueError, match="level_sizes"):
        FeatureActivity(17, "cpu", [1] * 17)
    t = FeatureActivity(10, "cpu", [4, 6])
    assert t.H == 10 and t.rows_seen == 0 and t.fired.dtype == t.last.dtype == t.base.dtype == torch.int64
    t.advance(48)
    seg = t.segment(4, 6)
    assert seg.H == 6 and seg.fired.data_ptr() == t.fired[4:].data_ptr() and seg.last.data_ptr() == t.last[4:].data_ptr()
    seg.add_bits(torch.zeros((0, 1), dtype=torch.int32))
    assert t.rows_seen == 48
    for bad in ((-1, 2), (8, 3), (0, 0)):
        with pytest.raises(ValueError):
            t.segment(*bad)
    with pytest.raises(ValueError, match="window"):
        t.summary(0)
    t.fired[3], t.last[3] = 5, 48
    state = t.state_dict()
    assert state["rows_seen"] == 48 and state["fired"][3] == 5
    fresh = FeatureActivity(10, "cpu", [4, 6])
    fresh.load_state_dict(state)
    assert fresh.rows_seen == 48 and torch.equal(fresh.fired, t.fired) and torch.equal(fresh.last, t.last)
    with pytest.raises(ValueError):
        FeatureActivity(11, "cpu").load_state_dict(state)


def test_for_model_picks_the_units_and_the_levels():
    D = 16
    q = QuantizedMatryoshkaSAE(D, 200, 8, 1.5, 4)
    t = FeatureActivity.for_model(q)
    assert t.H == 200 and t.level_sizes == list(q.decoder.nested_dictionary_size) and sum(t.level_sizes) == 200
    rq = ResidualQuantizedSAE(D, 200, 8, 1.5, 4)
    t = FeatureActivity.for_model(rq)
    assert t.level_sizes == list(rq.sae_hidden_dims) and t.H == sum(rq.sae_hidden_dims) == 200
    for model in (BinarySAE(D, 512, 4), BaselineSparseAutoencoder(D, 100), TernarySparseAutoencoder(D, 100), BinaryLatentSAE(D, 96)):
        t = FeatureActivity.for_model(model)
        assert t.H == model.encoder.linear.weight.shape[0] and t.level_sizes == [] and t.device.type == "cpu"
    for cls in (BinarySAE, BaselineSparseAutoencoder, TernarySparseAutoencoder, BinaryLatentSAE, QuantizedMatryoshkaSAE,
                ResidualQuantizedSAE):
        assert cls.activity is None


CONFIG = {"input_dim": 64, "n_bits": 4, "hidden_dim": 1024, "gamma": 1.5, "epochs": 1, "lr": 1e-4, "top_k": 32,
          "sparsity_lambda": 1.5e-3, "polarize_lambda": 1e-2, "batch_size": 64}


def test_trainer_accepts_and_validates_activity_window(tmp_path):
    t = Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path))
    assert t.activity is None and t.activity_window is None and "activity" not in t.model.__dict__ and t.model.activity is None
    for bad in (0, -5):
        with pytest.raises(ValueError, match="activity_window"):
            Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), activity_window=bad)
    t = Trainer(CONFIG, "q_sae", False, True, dataset_dir=str(tmp_path), activity_window=1000)
    assert isinstance(t.activity, FeatureActivity) and t.model.activity is t.activity and t.activity_window == 1000
    assert t.activity.level_sizes == list(t.model.decoder.nested_dictionary_size) and t.activity.H == 1024
    t = Trainer(CONFIG, "rq_sae", False, True, dataset_dir=str(tmp_path), activity_window=1)
    assert t.activity.level_sizes == list(t.model.sae_hidden_dims)
    assert all("activity" not in s.__dict__ for s in t.model.saes)
