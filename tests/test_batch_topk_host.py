"""BatchTopK without a GPU: hand-worked cases of the numpy restatement (tests/batch_topk_util.py); the ledger of
include/qsae_batch.h -- every function declared there is bound in _lib.BATCH_SIGNATURES with as many arguments as it declares,
exported by the product and the debug library as qsaeb_*, and is either a *_bytes sizer or driven between guard words in
tests/test_batch_topk_gpu.py; the calls of the C ABI that return before they look at a pointer, in the order the header states;
the front ends' refusals; and the kernels' own source run on the CPU (tests/emu, tests/emu_util.py: threads as lanes, real barriers),
which must equal the restatement bit for bit, twice on poisoned outputs and a poisoned workspace of exactly the sizer's bytes,
also in a stand-alone build with AddressSanitizer where every operand is a heap block of exactly its size."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import batch_topk_util as U
import test_batch_topk_gpu as G
from quantizedsae_amd import _lib, build, ops, torch_ops, training
from quantizedsae_amd.sae import (BaselineSparseAutoencoder, BinaryLatentSAE, BinarySAE, QuantizedMatryoshkaSAE,
                                  ResidualQuantizedSAE, TernarySparseAutoencoder)
from quantizedsae_amd.training import BatchTopK, Trainer
from sparsity_curve_util import gaussian
from emu_util import CSRC, ROOT, compile_emu, run_emu


def _f(*v):
    return np.array(v, dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


# ---- the restatement, by hand -----------------------------------------------------------------------------------------
def test_key_order_by_hand():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    v = _f(nan, inf, 3, 2.0 ** -149, 0.0, -0.0, -(2.0 ** -149), -3, -inf)
    key = U.mono_key(v).astype(np.int64)
    assert (np.diff(key) <= 0).all() and key[4] == key[5] and key[0] == 0xFFFFFFFF       # NaN first, -0 == +0
    assert U.mono_key(_f(np.nan)).tolist() == U.mono_key(np.array([0xFFC00001], np.uint32).view(np.float32)).tolist()


def test_batch_selection_by_hand():
    val = np.array([[5, 3, 3, 1], [3, 3, 2, 0], [9, 3, 0, 0]], dtype=np.float32)
    # 9 5 | 3 3 (row 0) 3 3 (row 1) 3 (row 2) | 2 1 0 0 0
    for n, want in ((0, [0, 0, 0]), (1, [0, 0, 1]), (2, [1, 0, 1]), (3, [2, 0, 1]), (5, [3, 1, 1]), (6, [3, 2, 1]), (7, [3, 2, 2]),
                    (8, [3, 3, 2]), (12, [4, 4, 4])):
        counts, val_sel, report = U.batch_select(val, n)
        assert counts.tolist() == want and int(report[0]) == n == int(counts.sum())
        assert all((val_sel[r, :c] == val[r, :c]).all() and not _bits(val_sel[r, c:]).any() for r, c in enumerate(counts))
    assert U.batch_select(val, 5)[2].tolist() == [5, 0, 0, int(_bits(_f(3.0))[0])]
    assert U.batch_select(val, 12)[2].tolist() == [12, 3, 0, 0]                          # the last in key order is a +0
    assert U.batch_select(val, 0)[2].tolist() == [0, 0, 3, 0]
    # the smallest selected value is the LAST in key order: of -0 (row 0) and +0 (row 1) the one in the later row
    z = np.array([[1, -0.0], [1, 0.0]], dtype=np.float32)
    assert U.batch_select(z, 3)[2][3] == 0x80000000 and U.batch_select(z, 4)[2][3] == 0


def test_threshold_by_hand():
    val = np.array([[5, 3, 3, 1], [3, 3, 2, 0], [np.nan, 9, 0, 0], [2, 7, 0, 0]], dtype=np.float32)
    counts, val_sel, report = U.threshold_select(val, 3.0)
    assert counts.tolist() == [3, 2, 0, 0]                   # >= keeps the equal value; NaN ends a prefix; so does a 2 in front
    assert report.tolist() == [5, 0, 2, int(_bits(_f(3.0))[0])]
    assert U.threshold_select(val, np.nan)[0].tolist() == [0, 0, 0, 0]
    assert U.threshold_select(val, -np.inf)[0].tolist() == [4, 4, 0, 4]
    assert U.threshold_select(val, np.inf)[0].tolist() == [0, 0, 0, 0]
    assert U.threshold_select(_f(0.0, -0.0)[None], 0.0)[0].tolist() == [2]
    # the moving average: the first update copies m; later ones move a hundredth of the way, in fp32; m <= 0 changes nothing
    rep = np.array([5, 0, 0, int(_bits(_f(2.0))[0])], dtype=np.int64)
    theta, n = U.threshold_update(0.0, 0, rep, 0.01)
    assert (theta, n) == (np.float32(2.0), 1)
    rep[3] = int(_bits(_f(4.0))[0])
    theta, n = U.threshold_update(theta, n, rep, 0.01)
    assert theta == np.float32(np.float32(2.0) + np.float32(np.float32(0.01) * np.float32(2.0))) and n == 2
    for bits in (0, 0x80000000, int(_bits(_f(-1.0))[0]), 0x7FC00000):
        rep[3] = bits
        assert U.threshold_update(theta, n, rep, 0.01) == (theta, 2)
    rep[0] = 0
    assert U.threshold_update(theta, n, rep, 0.01) == (theta, 2)


def test_ragged_restatement_by_hand():
    table = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, np.inf, 0], [0, 0, 0, 1]], dtype=np.float32)
    idx = np.array([[1, 0, 2], [3, 2, 0]], dtype=np.int32)
    val = np.array([[4, 2, 1], [4, 2, 1]], dtype=np.float32)
    r = U.decode_ragged(idx, val, [2, 1], ("table", table, 1.0), None)
    assert r.tolist() == [[2, 4, 0, 0], [0, 0, 0, 4]]        # the inf row of unit 2 lies behind both prefixes
    r = U.decode_ragged(idx, val, [0, 7], ("table", table, 0.5), _f(1, 1, 1, 1))
    assert r[0].tolist() == [1, 1, 1, 1] and np.isinf(r[1, 2])
    off, ent = U.csr_ragged(np.array([[1, 0, 2], [1, 5, 0]], dtype=np.int32), [2, 3], 4)
    assert off.tolist() == [0, 2, 4, 4, 4] and ent.tolist() == [1, 5, 0, 3, -1, -1]      # unit 5 is dropped, (0, 2) is behind
    g = np.ones((2, 4), np.float32)
    gv, dx = U.row_grad_ragged(idx, [2, 0], np.nan_to_num(table, posinf=7.0), 0.5, g, None, np.full((4, 4), 2, np.float32))
    assert gv.tolist() == [[0.5, 0.5, 0], [0, 0, 0]] and dx.tolist() == [[2, 2, 2, 2], [0, 0, 0, 0]]


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_batch.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_batch.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 9 and sorted(declared) == sorted(_lib.BATCH_SIGNATURES)
    assert all(n.startswith("qsaeb_") for n in declared)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.CURVE_SIGNATURES) | set(_lib.NESTED_SIGNATURES))
    for name, n_params in declared.items():
        assert len(_lib.BATCH_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaeb_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    sizers = {n for n in declared if n.endswith("_bytes")}
    guarded = {entry for entry, *_ in G.GUARD_CASES.values()}
    assert sizers | guarded == set(declared) and not sizers & guarded
    assert all(n[:-len("_workspace_bytes")] in guarded for n in sizers)      # every sizer belongs to a guarded call
    assert {"batch_topk.hip", "batch_topk_decode.hip"} <= set(build.SOURCES) and _lib.ABI_VERSION == 4
    assert "join qsae.h" in (ROOT / "include" / "qsae_batch.h").read_text()
    assert "qsae_batch.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()
    assert ops.BATCH_TOPK_MAX_K == torch_ops.BATCH_TOPK_MAX_K == 256


# ---- calls that need no device ----------------------------------------------------------------------------------------
def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()

    def select(B, K, n=0):
        return lib.qsaeb_batch_select(None, B, K, n, None, None, None, None, None, 0.01, None, 0, None)

    def threshold(B, K, n=0):
        return lib.qsaeb_threshold_select(None, B, K, None, 0.0, None, None, None, None, 0, None)

    for call, name in ((select, b"qsaeb_batch_select"), (threshold, b"qsaeb_threshold_select")):
        assert call(5, 257) == _lib.ERR_UNSUPPORTED                                           # K = 257
        assert name in lib.qsae_last_error()
        assert call(-1, 257) == _lib.ERR_UNSUPPORTED                                          # the limit comes first
        assert call(1 << 23, 256) == _lib.ERR_UNSUPPORTED                                     # B * K = 2^31
        assert call(-1, 8) == _lib.ERR_INVALID_ARG
        assert call(5, 0) == _lib.ERR_INVALID_ARG
        assert call(0, 8) == _lib.OK                                                          # B == 0: nothing launched
        assert call(5, 8, 3) == _lib.ERR_INVALID_ARG                                          # null pointers, before any launch
        assert b"null" in lib.qsae_last_error()
    assert select(5, 8, -1) == _lib.ERR_INVALID_ARG and select(5, 8, 41) == _lib.ERR_INVALID_ARG
    assert b"n_select" in lib.qsae_last_error()
    assert select(0, 8, 1) == _lib.ERR_INVALID_ARG                                            # n_select > B * K = 0

    def binary(B, K, H, D, n_bits=4):
        return lib.qsaeb_decode_ragged_binary(None, None, None, B, K, None, H, D, n_bits, 1.0, None, None, None)

    def table(B, K, H, D):
        return lib.qsaeb_decode_ragged_table(None, None, None, B, K, None, H, D, 1.0, None, None, None)

    def row(B, K, H, D):
        return lib.qsaeb_row_grad_ragged(None, None, B, K, None, H, D, 1.0, None, None, 0, None, None, None, None)

    def csr(B, K, H, D=None):
        return lib.qsaeb_csr_ragged(None, None, B, K, H, None, None, None, 0, None)

    for call, name in ((binary, b"qsaeb_decode_ragged_binary"), (table, b"qsaeb_decode_ragged_table"),
                       (row, b"qsaeb_row_grad_ragged"), (csr, b"qsaeb_csr_ragged")):
        assert call(5, 257, 512, 16) == _lib.ERR_UNSUPPORTED                                  # K = 257
        assert name in lib.qsae_last_error()
        assert call(1 << 23, 256, 64, 16) == _lib.ERR_UNSUPPORTED                             # B * K = 2^31
        assert call(-1, 8, 64, 16) == _lib.ERR_INVALID_ARG
        assert call(-1, 257, 64, 16) == _lib.ERR_INVALID_ARG                                  # sizes that make no sense come first
        assert call(5, 0, 64, 16) == _lib.ERR_INVALID_ARG
        assert call(5, 8, 0, 16) == _lib.ERR_INVALID_ARG                                      # H = 0
        assert call(5, 8, 64, 16) == _lib.ERR_INVALID_ARG                                     # null pointers, before any launch
        assert b"null" in lib.qsae_last_error()
    for call in (binary, table, row):
        for D in (6, 0, 4100, -4):
            assert call(5, 8, 64, D) == _lib.ERR_UNSUPPORTED
        assert call(0, 8, 64, 16) == _lib.OK                                                  # B == 0: nothing launched
    for bits in (0, 9):
        assert binary(5, 8, 64, 16, n_bits=bits) == _lib.ERR_UNSUPPORTED
    assert lib.qsaeb_batch_select_workspace_bytes(7, 6) > 0 and lib.qsaeb_threshold_select_workspace_bytes(7, 6) > 0
    assert lib.qsaeb_csr_ragged_workspace_bytes(7, 6, 512) > 0
    for size in (lib.qsaeb_batch_select_workspace_bytes, lib.qsaeb_threshold_select_workspace_bytes):
        assert size(7, 257) == 0 and size(-1, 6) == 0 and size(7, 0) == 0 and size(1 << 23, 256) == 0
    size = lib.qsaeb_csr_ragged_workspace_bytes
    assert size(7, 257, 512) == 0 and size(7, 6, 0) == 0 and size(-1, 6, 512) == 0 and size(1 << 23, 256, 512) == 0


def test_front_ends_refuse_host_tensors_and_bad_shapes():
    idx, val, cnt = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2), torch.zeros(2, dtype=torch.int32)
    table, packed = torch.zeros(8, 4), torch.zeros(8, 4, dtype=torch.uint8)
    for mod in (ops, torch_ops):
        for call in (lambda: mod.batch_select(val, 2), lambda: mod.threshold_select(val, 0.5),
                     lambda: mod.decode_ragged_table(idx, val, cnt, table, 1.0, None),
                     lambda: mod.decode_ragged_binary(idx, val, cnt, packed, 8, 4, 0.5, None),
                     lambda: mod.train_row_grad_ragged(idx, cnt, table, 1.0, None, None),
                     lambda: mod.train_csr_ragged(idx, cnt, 8)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        ctl = BatchTopK(model, k=2)
        assert (ctl.k, ctl.cap) == (2, 8) and ctl.threshold_lr == 0.01
        for call in (lambda: model.forward_batch_topk(val.new_zeros(2, 4), ctl),
                     lambda: model.forward_train_batch_topk(val.new_zeros(2, 4), ctl),
                     lambda: model.forward_threshold(val.new_zeros(2, 4), ctl)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_controller_and_trainer_validation(tmp_path):
    model = BaselineSparseAutoencoder(4, 512)
    model.topk = 65
    assert BatchTopK(model).cap == 256 and BatchTopK(model).k == 65                           # min(256, H, 4 k)
    assert BatchTopK(model, k=8).cap == 32 and BatchTopK(BaselineSparseAutoencoder(4, 16), k=8).cap == 16
    assert "BatchTopK" in training.__all__
    for kwargs, match in (({"k": 0}, "k"), ({"k": 600}, "k"), ({"k": 8, "cap": 4}, "cap"), ({"k": 8, "cap": 257}, "cap"),
                          ({"k": 8, "cap": 600}, "cap"), ({"threshold_lr": -0.1}, "threshold_lr"), ({"threshold_lr": 1.5}, "threshold_lr")):
        with pytest.raises(ValueError, match=match):
            BatchTopK(model, **kwargs)
    for other in (TernarySparseAutoencoder(4, 8), QuantizedMatryoshkaSAE(4, 32, top_k=2, n_bits=4),
                  ResidualQuantizedSAE(4, 32, top_k=2, n_bits=4), BinaryLatentSAE(4, 8)):
        assert not hasattr(other, "forward_batch_topk")
        with pytest.raises(TypeError, match="top-k"):
            BatchTopK(other)
    ctl = BatchTopK(model, k=8)
    sd = ctl.state_dict()
    assert sorted(sd) == ["batches", "cap", "k", "theta", "threshold_lr"] and float(sd["theta"]) == 0.0 and int(sd["batches"]) == 0
    sd["theta"], sd["batches"] = torch.tensor(0.25), torch.tensor(7)
    ctl.load_state_dict(sd)
    assert ctl.threshold() == 0.25 and int(ctl.batches) == 7
    with pytest.raises(ValueError, match="cap"):
        BatchTopK(model, k=8, cap=16).load_state_dict(sd)
    assert not any("theta" in key or "batch" in key for key in model.state_dict())            # the models' keys stay the reference's
    config = {"input_dim": 4, "n_bits": 4, "hidden_dim": 32, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 2,
              "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 8}
    for sae_type in ("t_sae", "bl_sae", "q_sae", "rq_sae"):
        with pytest.raises(ValueError, match="two top-k models"):
            Trainer(config, sae_type, True, True, dataset_dir=str(tmp_path), save_dir=str(tmp_path), batch_topk=True)
    with pytest.raises(ValueError, match="nested"):
        Trainer(config, "baseline_sae", False, True, model=BaselineSparseAutoencoder(4, 32), dataset_dir=str(tmp_path),
                save_dir=str(tmp_path), batch_topk=True, nested_bounds="default")
    with pytest.raises(ValueError, match="batch_topk_cap"):
        Trainer(config, "baseline_sae", False, True, model=BaselineSparseAutoencoder(4, 32), dataset_dir=str(tmp_path),
                save_dir=str(tmp_path), batch_topk_cap=8)


# ---- the kernels' own source on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("batch_topk_emu")


@pytest.fixture(scope="module")
def emu(build_dir):
    return compile_emu(build_dir, "batch_topk_emu.cpp", "batch_topk_emu", include=(CSRC,))


@pytest.fixture(scope="module")
def emu_asan(build_dir):
    return compile_emu(build_dir, "batch_topk_emu.cpp", "batch_topk_emu_asan", include=(CSRC,), asan=True)


def _hex(v) -> str:
    return f"{int(_bits(np.array([v], dtype=np.float32))[0]):08x}"


def _call(exe, d, *args):
    run_emu(exe, args, d, 900)


def _run_select(exe, d, val, n_select, state=None, lr=0.01):
    B, K = val.shape
    val.tofile(d / "val.bin")
    theta, batches = ("-", 0) if state is None else (_hex(state[0]), state[1])
    _call(exe, d, "s", "val.bin", B, K, n_select, theta, batches, _hex(lr), "counts.bin", "valsel.bin", "report.bin", "state.bin")
    st = np.fromfile(d / "state.bin", np.uint8)
    return (np.fromfile(d / "counts.bin", np.int32), np.fromfile(d / "valsel.bin", np.float32).reshape(B, K),
            np.fromfile(d / "report.bin", np.int64), (st[:4].view(np.float32)[0], int(st[8:].view(np.int64)[0])))


def _run_threshold(exe, d, val, theta, where):
    B, K = val.shape
    val.tofile(d / "val.bin")
    _call(exe, d, "t", "val.bin", B, K, _hex(theta), where, "counts.bin", "valsel.bin", "report.bin")
    return (np.fromfile(d / "counts.bin", np.int32), np.fromfile(d / "valsel.bin", np.float32).reshape(B, K),
            np.fromfile(d / "report.bin", np.int64))


def _same_selection(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w))


#: the shapes the host emulation runs (one thread per lane): all but the largest, and 257 x 33 -- more rows than one scan
#: thread owns, several histogram workgroups -- on the kind with heavy ties only
EMU_SHAPES = [(1, 1), (1, 256), (3, 5), (70, 64)]


@pytest.mark.parametrize("kind", U.SELECT_KINDS)
def test_selection_source_on_the_host_equals_the_restatement(emu, build_dir, kind):
    for B, K in EMU_SHAPES + ([(257, 33)] if kind == "eight_levels" else []):
        val = U.select_values(kind, B, K, seed=B)
        ns = {0, 1, B * max(1, K // 4), B * K, G.straddling_n(val)} if B < 257 else {G.straddling_n(val)}
        for n in sorted(ns):
            got = _run_select(emu, build_dir, val, n)
            want = U.batch_select(val, n)
            _same_selection(got[:3], want)
            assert int(got[0].sum()) == n


def test_selection_of_unsorted_rows_on_the_host(emu_asan, build_dir):
    """Rows that are not rank ordered: memory-safe, sum(counts) == n_select, and still the key order's selection."""
    val = gaussian(41, 37, 21)
    val[3, 5], val[9, 0] = np.nan, -np.inf
    for n in (0, 1, 300, 37 * 21):
        got = _run_select(emu_asan, build_dir, val, n)
        _same_selection(got[:3], U.batch_select(val, n))
        assert int(got[0].sum()) == n


def test_threshold_state_on_the_host(emu, build_dir):
    val = U.select_values("gaussian", 70, 64, seed=3)
    state = (np.float32(0.0), 0)
    for n, scale in ((70 * 16, 1.0), (70 * 16, 2.0), (70 * 60, 1.0), (70 * 8, 0.5)):     # the third batch has m <= 0
        v = (val * np.float32(scale)).astype(np.float32)
        got = _run_select(emu, build_dir, v, n, state=state)
        want = U.batch_select(v, n)
        _same_selection(got[:3], want)
        new = U.threshold_update(state[0], state[1], want[2], 0.01)
        assert _hex(got[3][0]) == _hex(new[0]) and got[3][1] == new[1]
        state = new
    assert state[1] == 3


@pytest.mark.parametrize("kind", ["gaussian", "eight_levels", "special"])
def test_threshold_selection_source_on_the_host(emu, emu_asan, build_dir, kind):
    for B, K in ((3, 5), (70, 64), (5, 256)):
        val = U.select_values(kind, B, K, seed=B + 1)
        present = val[B // 2, K // 2]
        for theta, exe, where in ((present, emu, "device"), (present, emu_asan, "host"), (np.nan, emu, "host"),
                                  (np.inf, emu, "device"), (-np.inf, emu_asan, "device"), (0.0, emu, "host")):
            _same_selection(_run_threshold(exe, build_dir, val, theta, where), U.threshold_select(val, theta))


@pytest.mark.parametrize("asan", [False, True])
@pytest.mark.parametrize("pattern", ["none", "all", "mixed", "outside"])
def test_lists_and_row_gradient_source_on_the_host(emu, emu_asan, build_dir, pattern, asan):
    exe, d = (emu_asan if asan else emu), build_dir
    for name in ("table_D48_s0.5_nobias_H8", "table_D516", "table_D4") if not asan else ("table_D516",):
        idx, val, decoder, _, H = U.ragged_case(name)
        B, K = idx.shape
        counts = U.count_patterns(B, K)[pattern]
        table, D = decoder[1], decoder[1].shape[1]
        idx.tofile(d / "idx.bin")
        counts.tofile(d / "cnt.bin")
        _call(exe, d, "c", "idx.bin", "cnt.bin", B, K, H, "offsets.bin", "entries.bin")
        off, ent = U.csr_ragged(idx, counts, H)
        assert np.array_equal(np.fromfile(d / "offsets.bin", np.int32), off)
        assert np.array_equal(np.fromfile(d / "entries.bin", np.int32), ent)
        g, gl, W = gaussian(81, B, D), gaussian(82, B, H), gaussian(83, H, D)
        table.tofile(d / "table.bin")
        g.tofile(d / "g.bin")
        gl.tofile(d / "gl.bin")
        W.tofile(d / "w.bin")
        for use_g, use_gl, use_w in ((True, True, True), (True, False, False), (False, True, True)):
            _call(exe, d, "g", "idx.bin", "cnt.bin", B, K, "table.bin", H, D, _hex(0.25), "g.bin" if use_g else "-",
                  "gl.bin" if use_gl else "-", "w.bin" if use_w else "-", "gv.bin", "dx.bin")
            gv, dx = U.row_grad_ragged(idx, counts, table, 0.25, g if use_g else None, gl if use_gl else None, W if use_w else None)
            assert np.array_equal(_bits(np.fromfile(d / "gv.bin", np.float32).reshape(B, K)), _bits(gv))
            if use_w:
                assert np.array_equal(_bits(np.fromfile(d / "dx.bin", np.float32).reshape(B, D)), _bits(dx))
