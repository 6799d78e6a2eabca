"""The nested levels over ragged rows without a GPU: hand-worked cases of the numpy restatement (tests/nested_ragged_util.py) and
the coverage its planted inputs give; the ledger of include/qsae_nested_batch.h -- every function declared there is bound in
_lib.NESTED_BATCH_SIGNATURES with as many arguments as it declares, exported by the product and the debug library as qsaem_* (and
nothing else is), and driven between guard words in tests/test_nested_ragged_gpu.py; the calls of the C ABI that return before
they look at a pointer; the front ends' refusal of host tensors, of bad bounds and of the four classes without a top-k; the
Trainer's validation of ``batch_topk_nested_bounds``; and the kernels' own source run on the CPU (tests/emu, tests/emu_util.py:
threads as lanes, real barriers), which must equal the restatement bit for bit, twice on poisoned outputs, also in a stand-alone
build with AddressSanitizer where every operand -- the lists, read only up to counts[r], included -- is a heap block of exactly
its size."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import nested_ragged_util as R
import nested_util as N
import test_nested_ragged_gpu as G
from batch_topk_util import clamp_counts
from quantizedsae_amd import _lib, build, ops, torch_ops
from quantizedsae_amd.inference import nested_errors
from quantizedsae_amd.sae import (BaselineSparseAutoencoder, BinaryLatentSAE, BinarySAE, QuantizedMatryoshkaSAE,
                                  ResidualQuantizedSAE, TernarySparseAutoencoder)
from quantizedsae_amd.training import BatchTopK, Trainer
from sparsity_curve_util import gaussian
from emu_util import CSRC, ROOT, compile_emu, run_emu

HEADER = ROOT / "include" / "qsae_nested_batch.h"


# ---- the restatement, by hand -----------------------------------------------------------------------------------------
def test_restatement_by_hand_with_a_nan_row_behind_the_prefix():
    # H = 4 atoms over D = 4 columns; both rows list (unit 2, unit 0, unit 3, unit 1) with values (2, 1, 4, 8); unit 1 is NaN
    table = np.array([[1, 0, 0, 0], [np.nan] * 4, [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
    idx = np.array([[2, 0, 3, 1]] * 2, dtype=np.int32)
    val = np.array([[2, 1, 4, 8]] * 2, dtype=np.float32)
    counts = np.array([2, 3], dtype=np.int32)                 # row 0 keeps (2, 0), row 1 keeps (2, 0, 3); unit 1 is behind both
    r = R.nested_recons(idx, val, counts, [1, 3, 4], ("table", table, 1.0), None)
    assert r[:, 0].tolist() == [[1, 0, 0, 0], [1, 2, 0, 0], [1, 2, 0, 0]]
    assert r[:, 1].tolist() == [[1, 0, 0, 0], [1, 2, 0, 0], [1, 2, 4, 0]]
    assert R.counts_below(idx, counts, [1, 3, 4], 4).tolist() == [[1, 1], [2, 2], [2, 3]]
    # a multiplication by zero would still give NaN: the masked composition on (idx, val_sel) does
    val_sel = np.where(np.arange(4)[None, :] < counts[:, None], val, np.float32(0)).astype(np.float32)
    assert np.isnan(N.nested_recons(idx, val_sel, [1, 3, 4], ("table", table, 1.0), None)[1:]).all()
    # a scale and a bias, an empty row, counts outside [0, K]
    bias = np.ones(4, dtype=np.float32)
    r = R.nested_recons(idx, val, np.array([0, -7], np.int32), [1, 4], ("table", table, 0.5), bias)
    assert r.tolist() == [[[1, 1, 1, 1]] * 2] * 2
    table[1] = 0
    r = R.nested_recons(idx, val, np.array([1000, 1], np.int32), [1, 4], ("table", table, 0.5), bias)
    assert r[:, 0].tolist() == [[1.5, 1, 1, 1], [1.5, 2, 3, 1]] and r[:, 1].tolist() == [[1, 1, 1, 1], [1, 2, 1, 1]]
    # ids outside the dictionary are dropped, not clamped
    idx[:, 0] = 4
    assert R.counts_below(idx, np.array([2, 4], np.int32), [1, 4], 4).tolist() == [[1, 1], [1, 3]]


def test_row_gradient_restatement_by_hand():
    table = np.array([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 3, 0], [0, 0, 0, 4]], dtype=np.float32)
    idx = np.array([[3, 0, 2], [1, 2, 0]], dtype=np.int32)
    g = [np.full((2, 4), 1, np.float32), np.full((2, 4), 10, np.float32)]
    G, gv, dx = R.row_grad(idx, np.array([2, 0], np.int32), table, 0.5, g, [1, 4], None, np.eye(4, dtype=np.float32))
    assert G[:, 0, 0].tolist() == [11, 10]                   # written for every row, whatever the counts are
    assert G[:, 1, 0].tolist() == [11, 10]
    # row 0 keeps (unit 3 -> level 1, unit 0 -> level 0): 0.5 * 10 * 4 and 0.5 * 11 * 1; behind the prefix +0
    assert gv.tolist() == [[20, 5.5, 0], [0, 0, 0]] and not gv[:, 2].view(np.uint32).any()
    assert dx.tolist() == [[5.5, 0, 0, 20], [0, 0, 0, 0]]
    G2, gv2, _ = R.row_grad(idx, np.array([2, 0], np.int32), table, 0.5, [g[0], None], [1, 4], None, None)
    assert G2[:, 0, 0].tolist() == [1, 0] and gv2[0].tolist() == [0, 0.5, 0]          # an absent level is skipped


def test_the_planted_inputs_cover_what_they_are_there_for():
    planted = [n for n, c in R.CASES.items() if (c[4], c[5]) == (9, 12)]
    assert len(planted) >= 10 and any(len(R.CASES[n][6]) == 8 for n in planted)
    for name in planted:
        facts = R.planted_facts(name)
        assert len(facts) == 5 and all(facts.values()), (name, facts)
    shapes = {(c[4], c[5]) for c in R.CASES.values()}
    assert {b for b, _ in shapes} == {1, 5, 9} and {k for _, k in shapes} == {1, 7, 12, 65, 256}
    assert {c[1] for c in R.CASES.values()} == {4, 48, 516, 520}
    assert {len(c[6]) for c in R.CASES.values()} == {1, 4, 8}
    assert {c[2] for c in R.CASES.values() if c[0] == "packed"} == {1, 4, 8}
    assert {c[2] for c in R.CASES.values() if c[0] == "table"} == {1.0, 0.5}
    assert {c[3] for c in R.CASES.values()} == {True, False}
    around = clamp_counts(R.patterns(5, 256)["around_64"], 256)
    assert around[:3].tolist() == [63, 64, 65] and set(R.patterns(9, 12)) == {"none", "all", "mixed", "outside"}
    assert set(R.EMU_CASES) <= set(R.CASES)


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_nested_batch.h"""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 3 and sorted(declared) == sorted(_lib.NESTED_BATCH_SIGNATURES)
    assert all(n.startswith("qsaem_") for n in declared)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.CURVE_SIGNATURES)
                                | set(_lib.NESTED_SIGNATURES) | set(_lib.BATCH_SIGNATURES))
    for name, n_params in declared.items():
        assert len(_lib.NESTED_BATCH_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaem_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    guarded = {entry for entry, *_ in G.GUARD_CASES.values()}
    assert guarded == set(declared)
    assert "nested_ragged.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in HEADER.read_text()
    assert "qsae_nested_batch.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()


# ---- calls that need no device ----------------------------------------------------------------------------------------
def _ints(*v):
    return (C.c_int * len(v))(*v)


def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()

    def binary(B, K, H, D, bounds, L, n_bits=4):
        return lib.qsaem_decode_nested_ragged_binary(None, None, None, B, K, None, H, D, n_bits, 1.0, None, bounds, L, None, None, None)

    def table(B, K, H, D, bounds, L):
        return lib.qsaem_decode_nested_ragged_table(None, None, None, B, K, None, H, D, 1.0, None, bounds, L, None, None, None)

    def row(B, K, H, D, bounds, L):
        g = (C.c_void_p * 8)()
        return lib.qsaem_row_grad_nested_ragged(None, None, B, K, None, H, D, 1.0, g, bounds, L, None, 0, None, None, None, None, None)
    good = _ints(1, 8, 64)
    for call, name in ((binary, b"qsaem_decode_nested_ragged_binary"), (table, b"qsaem_decode_nested_ragged_table"),
                       (row, b"qsaem_row_grad_nested_ragged")):
        # the order of qsae_batch.h: B, K, H first (invalid argument) ...
        assert call(-1, 257, 64, 6, None, 9) == _lib.ERR_INVALID_ARG
        assert name in lib.qsae_last_error()
        assert call(5, 0, 64, 6, None, 9) == _lib.ERR_INVALID_ARG                             # K = 0
        assert call(5, 8, 0, 6, None, 9) == _lib.ERR_INVALID_ARG                              # H = 0
        # ... then the limits (unsupported), none of which reads bounds
        assert call(5, 257, 512, 16, None, 3) == _lib.ERR_UNSUPPORTED                         # K = 257
        assert call(5, 8, 64, 16, None, 9) == _lib.ERR_UNSUPPORTED                            # 9 levels
        assert call(5, 8, 64, 16, None, 0) == _lib.ERR_UNSUPPORTED
        for D in (6, 0, -4, 4100):
            assert call(5, 8, 64, D, None, 3) == _lib.ERR_UNSUPPORTED
        assert call(1 << 23, 256, 64, 16, None, 3) == _lib.ERR_UNSUPPORTED                    # B * K = 2^31
        # ... then the bounds of qsae_nested.h (invalid argument)
        assert call(5, 8, 64, 16, None, 3) == _lib.ERR_INVALID_ARG                            # bounds is null
        assert call(5, 8, 64, 16, _ints(1, 64, 8), 3) == _lib.ERR_INVALID_ARG                 # not ascending
        assert call(5, 8, 64, 16, _ints(8, 8, 64), 3) == _lib.ERR_INVALID_ARG                 # not distinct
        assert call(5, 8, 64, 16, _ints(0, 8, 64), 3) == _lib.ERR_INVALID_ARG                 # bounds[0] == 0
        assert call(5, 8, 64, 16, _ints(1, 8, 63), 3) == _lib.ERR_INVALID_ARG                 # the last bound is not H
        assert call(0, 8, 64, 16, _ints(1, 8, 63), 3) == _lib.ERR_INVALID_ARG                 # ... also without rows
        # B == 0: nothing launched, no pointer looked at
        assert call(0, 8, 64, 16, good, 3) == _lib.OK
        assert call(0, 1, 1, 4, _ints(1), 1) == _lib.OK
        # ... and only then the pointers
        assert call(5, 8, 64, 16, good, 3) == _lib.ERR_INVALID_ARG
        assert b"null" in lib.qsae_last_error()
    for bits in (0, 9):
        assert binary(5, 8, 64, 16, good, 3, n_bits=bits) == _lib.ERR_UNSUPPORTED
        assert binary(5, 8, 64, 6, good, 3, n_bits=bits) == _lib.ERR_UNSUPPORTED               # D is refused first, the same code
    assert lib.qsaem_row_grad_nested_ragged(None, None, 0, 8, None, 64, 16, 1.0, None, good, 3, None, 0, None, None, None, None,
                                            None) == _lib.OK                                  # g_levels is not looked at either


def test_front_ends_refuse_host_tensors_and_bad_bounds():
    idx, val, x = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2), torch.zeros(2, 4)
    counts = torch.zeros(2, dtype=torch.int32)
    table, packed = torch.zeros(8, 4), torch.zeros(8, 4, dtype=torch.uint8)
    for mod in (ops, torch_ops):
        for call in (lambda: mod.decode_nested_ragged_table(idx, val, counts, table, 1.0, None, [4, 8]),
                     lambda: mod.decode_nested_ragged_binary(idx, val, counts, packed, 4, 8, 0.5, None, [4, 8]),
                     lambda: mod.train_row_grad_nested_ragged(idx, counts, table, 1.0, [None, None], [4, 8], None, None)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        ctl = BatchTopK(model, k=2)
        assert ctl.level_counts is None
        for call in (lambda: model.forward_nested_batch_topk(x, ctl, [4, 8]), lambda: model.forward_nested_threshold(x, ctl, [4, 8]),
                     lambda: model.forward_nested_threshold(x, 0.5, [4, 8], cap=4),
                     lambda: model.forward_train_nested_batch_topk(x, ctl, [4, 8]),
                     lambda: nested_errors(model, [x], [4, 8], threshold=ctl), lambda: nested_errors(model, [x], [4, 8], threshold=0.5)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
        with pytest.raises(ValueError, match="empty loader"):
            nested_errors(model, [], [4, 8], threshold=0.5)
        with pytest.raises(ValueError, match="cap goes with threshold"):
            nested_errors(model, [x], [4, 8], cap=4)
    for bad in ([], [0, 8], [2, 2, 8], [4, 2, 8], [2, 4], [2, 9], list(range(1, 10)), [1.5, 8], None):
        with pytest.raises(ValueError, match="bounds|levels"):
            ops.nested_bounds(bad, 8, "decode_nested_ragged_table")


def test_front_ends_refuse_the_four_classes_without_a_top_k(tmp_path):
    others = (TernarySparseAutoencoder(4, 8), QuantizedMatryoshkaSAE(4, 32, top_k=2, n_bits=4),
              ResidualQuantizedSAE(4, 32, top_k=2, n_bits=4), BinaryLatentSAE(4, 8))
    for model in others:
        for name in ("forward_nested_batch_topk", "forward_nested_threshold", "forward_train_nested_batch_topk"):
            assert not hasattr(model, name)
        with pytest.raises(TypeError, match="not a k"):
            nested_errors(model, [torch.zeros(2, 4)], threshold=0.5)
    for cls in (BinarySAE, BaselineSparseAutoencoder):
        for name in ("forward_nested_batch_topk", "forward_nested_threshold", "forward_train_nested_batch_topk"):
            assert callable(getattr(cls, name))


def test_trainer_validation(tmp_path):
    config = {"input_dim": 4, "n_bits": 4, "hidden_dim": 32, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 2,
              "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 8}
    where = dict(dataset_dir=str(tmp_path), save_dir=str(tmp_path))

    def baseline(**kw):
        return Trainer(config, "baseline_sae", False, True, model=BaselineSparseAutoencoder(4, 32), **where, **kw)
    with pytest.raises(ValueError, match="batch_topk_nested_bounds needs batch_topk=True"):
        baseline(batch_topk_nested_bounds="default")
    with pytest.raises(ValueError, match="batch_topk_nested_bounds needs batch_topk=True"):
        baseline(batch_topk_nested_bounds=[8, 32], nested_bounds=[8, 32])
    for sae_type in ("t_sae", "bl_sae", "q_sae", "rq_sae"):
        with pytest.raises(ValueError, match="two top-k models"):
            Trainer(config, sae_type, True, True, **where, batch_topk=True, batch_topk_nested_bounds="default")
        with pytest.raises(ValueError, match="batch_topk_nested_bounds"):
            Trainer(config, sae_type, True, True, **where, batch_topk_nested_bounds="default")
    with pytest.raises(ValueError, match="nested") as e:      # the old combination still raises, and names the new keyword
        baseline(batch_topk=True, nested_bounds="default")
    assert "batch_topk_nested_bounds" in str(e.value)
    with pytest.raises(ValueError, match="nested"):
        baseline(batch_topk=True, nested_bounds="default", batch_topk_nested_bounds="default")
    with pytest.raises(ValueError, match="batch_topk_cap needs batch_topk=True"):
        baseline(batch_topk_cap=4)
    for bad in ("levels", [8, 8, 32], [8, 16], []):
        with pytest.raises(ValueError, match="bounds|levels"):
            baseline(batch_topk=True, batch_topk_nested_bounds=bad)
    t = baseline(batch_topk=True, batch_topk_nested_bounds="default")
    assert t.nested_bounds == [4, 8, 16, 32] and t.batch_topk is not None and t.batch_topk.level_counts is None
    t = baseline(batch_topk=True, batch_topk_cap=32, batch_topk_nested_bounds=(8, 32))
    assert t.nested_bounds == [8, 32]
    assert baseline(batch_topk=True).nested_bounds is None and baseline(nested_bounds=[8, 32]).batch_topk is None


# ---- the kernels' own source on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("nested_ragged_emu")


@pytest.fixture(scope="module")
def emus(build_dir):
    return {False: compile_emu(build_dir, "nested_ragged_emu.cpp", "nested_ragged_emu", include=(CSRC,)),
            True: compile_emu(build_dir, "nested_ragged_emu.cpp", "nested_ragged_emu_asan", include=(CSRC,), asan=True)}


def _run(exe: Path, d: Path, idx, val, counts, bounds, decoder, bias, want_below=True):
    B, K = idx.shape
    np.ascontiguousarray(idx).tofile(d / "idx.bin")
    np.ascontiguousarray(val).tofile(d / "val.bin")
    np.ascontiguousarray(counts, dtype=np.int32).tofile(d / "counts.bin")
    np.ascontiguousarray(decoder[1]).tofile(d / "dict.bin")
    if bias is not None:
        bias.tofile(d / "bias.bin")
    packed = decoder[0] == "packed"
    D = decoder[2] if packed else decoder[1].shape[1]
    cmd = ["p" if packed else "t", "idx.bin", "val.bin", "counts.bin", B, K, "dict.bin", decoder[1].shape[0], D,
           decoder[3] if packed else 0, repr(float(decoder[-1])), "-" if bias is None else "bias.bin",
           ",".join(str(b) for b in bounds), "recon.bin", "below.bin" if want_below else "-"]
    run_emu(exe, cmd, d, 900)
    recon = np.fromfile(d / "recon.bin", np.float32).reshape(len(bounds), B, D)
    return recon, (np.fromfile(d / "below.bin", np.int32).reshape(len(bounds), B) if want_below else None)


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8))


@pytest.mark.parametrize("asan", [False, True])
@pytest.mark.parametrize("name", R.EMU_CASES)
def test_kernel_source_on_the_host_equals_the_restatement(emus, build_dir, name, asan):
    idx, val, bounds, decoder, bias = R.build_case(name)
    H = decoder[1].shape[0]
    for pattern, counts in R.patterns(*idx.shape).items():
        recon, below = _run(emus[asan], build_dir, idx, val, counts, bounds, decoder, bias, want_below=pattern != "none")
        _same(recon, R.nested_recons(idx, val, counts, bounds, decoder, bias))
        if below is not None:
            _same(below, R.counts_below(idx, counts, bounds, H))


@pytest.mark.parametrize("asan", [False, True])
@pytest.mark.parametrize("name", sorted(R.SPECIAL_CASES))
def test_special_values_on_the_host(emus, build_dir, name, asan):
    idx, val, counts, bounds, decoder, bias, check = R.special_case(name)
    recon, below = _run(emus[asan], build_dir, idx, val, counts, bounds, decoder, bias)
    _same(recon, R.nested_recons(idx, val, counts, bounds, decoder, bias))
    _same(below, R.counts_below(idx, counts, bounds, decoder[1].shape[0]))
    check(recon)


def _run_row_grad(exe: Path, d: Path, idx, counts, table, step, g, present, bounds, g_latent, W):
    B, K = idx.shape
    H, D = table.shape
    np.ascontiguousarray(idx).tofile(d / "idx.bin")
    np.ascontiguousarray(counts, dtype=np.int32).tofile(d / "counts.bin")
    table.tofile(d / "table.bin")
    np.ascontiguousarray(np.stack(g)).tofile(d / "g.bin")
    g_latent.tofile(d / "glat.bin")
    W.tofile(d / "wenc.bin")
    cmd = ["g", "idx.bin", "counts.bin", B, K, "table.bin", H, D, repr(float(step)), ",".join(str(b) for b in bounds), "g.bin",
           ",".join(str(int(p)) for p in present), "glat.bin", "wenc.bin", "G.bin", "gv.bin", "dx.bin"]
    run_emu(exe, cmd, d, 900)
    return (np.fromfile(d / "G.bin", np.float32).reshape(len(bounds), B, D), np.fromfile(d / "gv.bin", np.float32).reshape(B, K),
            np.fromfile(d / "dx.bin", np.float32).reshape(B, D))


@pytest.mark.parametrize("asan", [False, True])
@pytest.mark.parametrize("name,present", [("table_D48", (1, 1, 1, 1)), ("table_D48", (1, 0, 1, 0)), ("table_D4", (0, 0, 0, 0)),
                                          ("table_D516", (1, 1, 0, 1)), ("table_D520_s0.5_nobias_B5_K65", (1, 1, 1, 1)),
                                          ("table_D48_B1_K1_eight_levels", (1, 0, 1, 1, 0, 1, 1, 1))])
def test_row_gradient_source_on_the_host(emus, build_dir, name, present, asan):
    """G, gv and dx bit for bit against the restatement, under every counts pattern"""
    idx, _, bounds, decoder, _ = R.build_case(name)
    B, K = idx.shape
    table = decoder[1]
    H, D = table.shape
    W, g_latent = gaussian(72, H, D), gaussian(73, B, H)
    g = [gaussian(80 + l, B, D) for l in range(len(bounds))]
    for pattern, counts in R.patterns(B, K).items():
        G, gv, dx = _run_row_grad(emus[asan], build_dir, idx, counts, table, 0.5, g, present, bounds, g_latent, W)
        wG, wgv, wdx = R.row_grad(idx, counts, table, 0.5, [t if p else None for t, p in zip(g, present)], bounds, g_latent, W)
        _same(G, wG), _same(gv, wgv), _same(dx, wdx)
        c = clamp_counts(counts, K)
        assert not gv[np.arange(K)[None, :] >= c[:, None]].view(np.uint32).any()              # +0 by bit pattern
