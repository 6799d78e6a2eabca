"""The watch feature's host surface; runs without a GPU: the two new C-ABI entry points and their argument checks, the
dispatcher schema, the numpy restatement of csrc/watch.hip pinned to torch on the CPU (counts equal to torch.histc, edges to
torch.linspace, mean and std within the bound tests/watch_util.py derives), the Trainer's new constructor arguments, and
TensorStats."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import quantizedsae_amd
import watch_util as U
from quantizedsae_amd import _lib, training
from quantizedsae_amd import torch_ops  # noqa: F401  (registers torch.ops.qsae.*)
from quantizedsae_amd.training import ModelWatch, TensorStats, Trainer, tensor_stats
from quantizedsae_amd.training.watch import _parse

ROOT = Path(__file__).resolve().parents[1]
P = ctypes.c_void_p
NEW = ("qsae_tensor_stats_workspace_bytes", "qsae_tensor_stats")


@pytest.fixture(scope="module")
def lists():
    return U.case_lists()


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.load().qsae_abi_version() == _lib.ABI_VERSION == 4
    assert "watch.hip" in __import__("quantizedsae_amd.build", fromlist=["SOURCES"]).SOURCES
    for name in ("ModelWatch", "TensorStats", "tensor_stats"):
        assert name in training.__all__ and hasattr(training, name)
    assert quantizedsae_amd.ops.TENSOR_STATS_HEAD == U.HEAD and quantizedsae_amd.ops.TENSOR_STATS_MAX_BINS == U.MAX_BINS


def _call(lib, ptrs, counts, dtype=0, bins=64, result=P(4096), ws=P(8192), ws_bytes=1 << 20, T=None):
    T = len(counts) if T is None else T
    cp = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    cc = (ctypes.c_int64 * max(len(counts), 1))(*counts) if counts is not None else None
    return lib.qsae_tensor_stats(cp, cc, T, dtype, bins, result, ws, ws_bytes, None)


def test_invalid_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    a = 4096
    assert _call(lib, [], [], T=0) == _lib.OK                                       # nothing to do, nothing launched
    assert lib.qsae_tensor_stats(None, None, 0, 0, 64, None, None, 0, None) == _lib.OK
    assert _call(lib, [None, a], [0, 0], result=None, ws=None, ws_bytes=0) == _lib.OK  # every count 0
    assert _call(lib, [a], [8], T=-1) == _lib.ERR_INVALID_ARG
    assert b"invalid argument" in lib.qsae_last_error() and b"qsae_tensor_stats" in lib.qsae_last_error()
    assert _call(lib, [a, a], [8, -1]) == _lib.ERR_INVALID_ARG                      # a negative count
    assert _call(lib, [a, None], [8, 8]) == _lib.ERR_INVALID_ARG                    # a null pointer with a non-zero count
    assert _call(lib, [a, a + 2], [8, 8]) == _lib.ERR_INVALID_ARG                   # a pointer off its 4 bytes
    for bins in (0, -1, 257):
        assert _call(lib, [a], [8], bins=bins) == _lib.ERR_INVALID_ARG
    for dtype in (1, 2, 3, -1):
        assert _call(lib, [a], [8], dtype=dtype) == _lib.ERR_UNSUPPORTED
    assert b"unsupported" in lib.qsae_last_error()
    assert lib.qsae_tensor_stats(None, None, 2, 0, 64, P(a), P(a), 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert _call(lib, [a], [8], result=None) == _lib.ERR_INVALID_ARG
    assert _call(lib, [a], [8], result=P(a + 4)) == _lib.ERR_INVALID_ARG
    assert _call(lib, [a], [(1 << 40) + 1]) == _lib.ERR_UNSUPPORTED                 # the cap on one tensor
    assert _call(lib, [a] * 9, [1 << 40] * 9) == _lib.ERR_UNSUPPORTED               # the cap on the chunks of a call
    assert _call(lib, [a], [8], T=65537) == _lib.ERR_UNSUPPORTED                    # the cap on T
    assert _call(lib, [a], [8], ws=None) == _lib.ERR_WORKSPACE
    assert _call(lib, [a], [8], ws_bytes=8) == _lib.ERR_WORKSPACE
    assert b"qsae_tensor_stats_workspace_bytes" in lib.qsae_last_error()
    # workspace: 32 bytes per chunk of 8192 elements in six arrays of 256-byte pieces, and one 256-byte piece of records
    size = lambda counts: lib.qsae_tensor_stats_workspace_bytes((ctypes.c_int64 * len(counts))(*counts), len(counts))  # noqa: E731
    assert size([1]) == 7 * 256 and size([8192, 8193, 0]) == 7 * 256
    assert size([8192 * 64]) == 2 * 512 + 4 * 256 + 256
    assert size([0, 0]) == 0 and size([-1]) == 0 and size([(1 << 40) + 1]) == 0
    assert lib.qsae_tensor_stats_workspace_bytes(None, 0) == 0


def test_op_schema_and_fake_are_registered():
    op = torch.ops.qsae.tensor_stats
    assert [a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write] == []
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = op([torch.empty(5, 3), torch.empty(0), torch.empty(70000)], 64)
        assert out.shape == (3, 8 + 64) and out.dtype == torch.int64


def test_cpu_tensors_and_what_would_need_a_copy_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.qsae.tensor_stats([torch.zeros(4)], 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tensor_stats([torch.zeros(4)])
    with pytest.raises(ValueError, match="bins"):
        quantizedsae_amd.ops.tensor_stats([], 257)
    model = torch.nn.Linear(4, 3)
    with pytest.raises(RuntimeError, match="MI355X only.*parameters/weight"):
        ModelWatch(model).collect()
    with pytest.raises(ValueError, match="log must be"):
        ModelWatch(model, log="weights")
    with pytest.raises(ValueError, match="bins"):
        ModelWatch(model, bins=0)
    assert ModelWatch(torch.nn.Identity()).collect() == {}


# ---- the restatement against torch on the CPU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bins", U.RUNS, ids=U.RUN_IDS)
def test_restatement_equals_torch_on_the_cpu(lists, name, bins):
    for t, x in enumerate(lists[name]):
        r = U.restate_one(x, bins)
        ref = U.histc_cpu(x, bins)
        where = (name, t, x.size)
        if ref is None:
            assert r["n_finite"] == 0 and not r["counts"].any() and r["n_nonfinite"] == x.size, where
            continue
        counts, lo, hi = ref
        assert np.array_equal(r["counts"], counts), where                          # zero mismatches
        assert float(r["lo"]) == lo and float(r["hi"]) == hi, where
        stats = _parse(torch.from_numpy(U.restate_block([x], bins).view(np.int64)))[0]
        assert np.array_equal(stats.edges.numpy(), torch.linspace(lo, hi, bins + 1).numpy(), equal_nan=True), where
        recipe = U.wandb_recipe(torch.from_numpy(x), bins)                          # (an overflowing range has NaN edges)
        mine = stats.np_histogram()
        assert mine[0] == recipe[0] and np.array_equal(np.array(mine[1]), np.array(recipe[1]), equal_nan=True), where
        f = x[np.isfinite(x)].astype(np.float64)
        d_mean, d_std = U.moment_bounds(f)
        td = torch.from_numpy(f)
        assert abs(r["mean"] - td.mean().item()) <= d_mean, where
        assert r["n_zero"] == int((f == 0).sum()) and r["n_finite"] == f.size
        if f.size > 1:
            assert abs(stats.std - td.std().item()) <= d_std, where
        else:
            assert np.isnan(stats.std)


def test_the_bin_rule_is_the_form_torch_uses_where_the_two_fp32_forms_part():
    for lo, hi, x, ours, other in U.SEPARATORS:
        lo, hi, x = (np.array([v], np.uint32).view(np.float32)[0] for v in (lo, hi, x))
        assert int(U.bin_index(np.array([x]), lo, hi, U.SEPARATOR_BINS)[0]) == ours
        assert int(U.other_form_index(np.array([x]), lo, hi, U.SEPARATOR_BINS)[0]) == other != ours
        t = torch.histc(torch.tensor([lo, hi, x]), bins=U.SEPARATOR_BINS, min=float(lo), max=float(hi))
        t[0] -= 1
        t[-1] -= 1
        assert int(t.argmax()) == ours and t.sum() == 1


def test_constant_tensors_land_where_torch_puts_them():
    """the widened range: [lo - 1, hi + 1] below 2^24, the neighbouring floats where the 1 is rounded away"""
    values = [0.0, -0.0, 1.0, 0.375, 1e-45, 2.0 ** 24 - 1, 2.0 ** 24, -2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 25, 2.0 ** 26, 1e10, -3e10,
              2.0 ** 100, 3e38, U.FMAX, -U.FMAX]
    for v in values:
        x = np.full(5, v, np.float32)
        for bins in (1, 2, 3, 7, 64, 100, 255, 256):
            ref = U.histc_cpu(x, bins)[0]
            assert np.array_equal(U.restate_one(x, bins)["counts"], ref), (v, bins)
            if abs(v) < 2.0 ** 24:
                assert ref[bins // 2] == 5
    assert U.restate_one(np.full(9, 0.25, np.float32), 64)["counts"][32] == 9      # bin 32 of 64


def test_a_range_that_overflows_counts_nothing_as_in_torch():
    x = np.array([-U.FMAX, 0.0, 1.0, U.FMAX], np.float32)
    for bins in (1, 64, 256):
        assert not U.histc_cpu(x, bins)[0].any() and not U.restate_one(x, bins)["counts"].any()
    r = U.restate_one(x, 64)
    assert float(r["lo"]) == -U.FMAX and float(r["hi"]) == U.FMAX and r["n_finite"] == 4


def test_the_ordered_sum_is_the_kernels_order():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(2 * U.CHUNK + 5)
    # by hand: thread chains over (slab, element), butterfly, waves, then the chunk partials
    parts = []
    for c in range(3):
        chunk = np.zeros(U.CHUNK)
        seg = x[c * U.CHUNK:(c + 1) * U.CHUNK]
        chunk[:seg.size] = seg
        lanes = np.zeros(256)
        for j in range(256):
            acc = 0.0
            for k in range(8):
                for e in range(4):
                    acc = acc + chunk[k * 1024 + 4 * j + e]
            lanes[j] = acc
        waves = []
        for w in range(4):
            s = lanes[64 * w:64 * w + 64].copy()
            for m in (32, 16, 8, 4, 2, 1):
                s = s + s[np.arange(64) ^ m]
            waves.append(s[0])
        parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    lanes = np.zeros(256)
    lanes[:3] = parts
    waves = []
    for w in range(4):
        s = lanes[64 * w:64 * w + 64].copy()
        for m in (32, 16, 8, 4, 2, 1):
            s = s + s[np.arange(64) ^ m]
        waves.append(s[0])
    assert U.ordered_sum(x) == ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert U.ordered_sum(np.zeros(0)) == 0.0


# ---- TensorStats and the Trainer's arguments ------------------------------------------------------------------------------------
def test_tensor_stats_fields_edges_and_np_histogram():
    x = np.array([0.0, 1.0, 2.0, 4.0, np.nan, -0.0], np.float32)
    s = _parse(torch.from_numpy(U.restate_block([x, np.zeros(0, np.float32)], 4).view(np.int64)))
    assert isinstance(s[0], TensorStats) and s[0].bins == 4
    assert (s[0].lo, s[0].hi, s[0].n_finite, s[0].n_nonfinite, s[0].n_zero) == (0.0, 4.0, 5, 1, 2)
    assert s[0].counts.dtype == torch.int64 and s[0].counts.tolist() == [2, 1, 1, 1]
    assert s[0].mean == 1.4 and abs(s[0].std - float(torch.tensor([0.0, 1, 2, 4, 0], dtype=torch.float64).std())) < 1e-15
    assert s[0].edges.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and s[0].edges.dtype == torch.float32
    assert s[0].np_histogram() == ([2, 1, 1, 1], [0.0, 1.0, 2.0, 3.0, 4.0])
    assert s[1].n_finite == 0 and not s[1].counts.any() and np.isnan(s[1].std)


CONFIG = {"input_dim": 64, "n_bits": 4, "hidden_dim": 1024, "gamma": 1.5, "epochs": 1, "lr": 1e-4, "top_k": 32,
          "sparsity_lambda": 1.5e-3, "polarize_lambda": 1e-2, "batch_size": 64}


def test_trainer_accepts_and_validates_watch_and_watch_freq(tmp_path):
    t = Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path))
    assert t._watch is None and t.watch_freq == 256                                 # the default changes nothing
    for mode in ("all", "parameters", "gradients"):
        t = Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), watch=mode, watch_freq=7)
        assert isinstance(t._watch, ModelWatch) and t._watch.log == mode and t._watch.model is t.model and t.watch_freq == 7
        assert t._watch.bins == 64
    with pytest.raises(ValueError, match="watch"):
        Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), watch="weights")
    with pytest.raises(ValueError, match="watch_freq"):
        Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), watch="all", watch_freq=0)
