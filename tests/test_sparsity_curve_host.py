"""The sparsity-fidelity curve without a GPU: hand-worked cases of the numpy restatement (tests/sparsity_curve_util.py); the
ledger of include/qsae_curve.h -- every function declared there is bound in _lib.CURVE_SIGNATURES with as many arguments as it
declares, exported by the product and the debug library as qsaec_*, and is either a *_bytes sizer or driven between guard
words in tests/test_sparsity_curve_gpu.py; the calls of the C ABI that return before they look at a pointer; default_ks; the
front ends' refusal of host tensors and of the four classes whose sparsity is not a k; and the kernel's own source run on
the CPU (tests/emu, tests/emu_util.py: threads as lanes, real barriers), which must equal the restatement bit for bit, twice on
one poisoned workspace, also in a stand-alone build with AddressSanitizer where every operand is a heap block of exactly
its size."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sparsity_curve_util as U
import test_sparsity_curve_gpu as G
from quantizedsae_amd import _lib, build, inference, ops, torch_ops
from quantizedsae_amd.inference import SparsityCurve, default_ks
from quantizedsae_amd.sae import (BaselineSparseAutoencoder, BinaryLatentSAE, BinarySAE, QuantizedMatryoshkaSAE,
                                  ResidualQuantizedSAE, TernarySparseAutoencoder)
from emu_util import CSRC, ROOT, compile_emu, run_emu


# ---- the restatement, by hand -----------------------------------------------------------------------------------------
def _hand():
    # H = 3 atoms over D = 4 columns; the list of every row is (unit 2, unit 0) with values (2, 1)
    table = np.array([[1, 0, 0, 0], [9, 9, 9, 9], [0, 1, 0, 0]], dtype=np.float32)
    idx = np.array([[2, 0]] * 5, dtype=np.int32)
    val = np.array([[2, 1]] * 5, dtype=np.float32)
    x = np.zeros((5, 4), dtype=np.float32)
    return table, idx, val, x


def test_restatement_by_hand():
    table, idx, val, x = _hand()
    # k' = 0: nothing; 1: unit 2 alone -> (0, 2, 0, 0); 2: both -> (1, 2, 0, 0).  Errors against x = 0: 0, 4, 5 per row
    sums, counts, recons = U.prefix_errors(x, idx, val, [0, 1, 2], ("table", table, 1.0), None, 2)
    assert recons[:, 0].tolist() == [[0, 0, 0, 0], [0, 2, 0, 0], [1, 2, 0, 0]]
    assert sums.tolist() == [0.0, 20.0, 25.0] and counts.tolist() == [5, 0]
    # a scale and a bias: 0.5 * chain + bias
    bias = np.array([1, 1, 1, 1], dtype=np.float32)
    sums, _, recons = U.prefix_errors(x, idx, val, [2], ("table", table, 0.5), bias, 2)
    assert recons[0, 0].tolist() == [1.5, 2, 1, 1] and sums.tolist() == [5 * (2.25 + 4 + 1 + 1)]


def test_restatement_skips_a_nan_group_and_takes_a_short_last_group():
    table, idx, val, x = _hand()
    x[2, 1] = np.nan                                          # groups of 2: rows (0, 1), (2, 3), (4); the middle one is skipped
    sums, counts, recons = U.prefix_errors(x, idx, val, [1], ("table", table, 1.0), None, 2)
    assert sums.tolist() == [12.0] and counts.tolist() == [3, 2]
    assert recons.shape == (1, 5, 4) and recons[0, 2].tolist() == [0, 2, 0, 0]       # reconstructions of flagged rows too
    # two calls cut at a multiple of group_rows continue the same state
    s1, c1, _ = U.prefix_errors(x[:2], idx[:2], val[:2], [1], ("table", table, 1.0), None, 2)
    s2, c2, _ = U.prefix_errors(x[2:], idx[2:], val[2:], [1], ("table", table, 1.0), None, 2, s1, c1)
    assert s2.tolist() == [12.0] and c2.tolist() == [3, 2]


def test_restatement_ks_zero_gives_the_bias_or_plus_zero():
    table, idx, val, x = _hand()
    _, _, recons = U.prefix_errors(x, idx, val, [0], ("table", table, 0.5), None, 4)
    assert not recons.view(np.uint32).any()                   # +0, not -0
    bias = np.array([-1, 2, 0, 3], dtype=np.float32)
    sums, _, recons = U.prefix_errors(x, idx, val, [0], ("table", table, 0.5), bias, 4)
    assert (recons[0] == bias).all() and sums.tolist() == [5 * 14.0]


def test_restatement_drops_ids_outside_the_dictionary_and_never_touches_later_ranks():
    table, idx, val, x = _hand()
    idx[:, 0] = 7                                             # outside [0, 3): only unit 0 is left
    _, _, recons = U.prefix_errors(x, idx, val, [1, 2], ("table", table, 1.0), None, 4)
    assert not recons[0].any() and recons[1, 0].tolist() == [1, 0, 0, 0]
    table, idx, val, x = _hand()
    table[0, 3] = np.inf                                      # unit 0 has rank 1: the point k' = 1 never sees it
    _, _, recons = U.prefix_errors(x, idx, val, [1, 2], ("table", table, 1.0), None, 4)
    assert np.isfinite(recons[0]).all() and np.isinf(recons[1, :, 3]).all()


def test_row_sum_order_is_the_butterfly_over_octet_slots():
    # D = 1028: octet 128 (columns 1024 .. 1027) shares slot 0 with octets 0 and 64
    # slot 0 in ascending column order: 1 first, then four terms of 2^-54, each below half an ulp of 1 -> exactly 1;
    # any order that adds the small ones to each other first gives 1 + 2^-52
    t = np.zeros((1, 1, 1028), dtype=np.float32)
    t[0, 0, 0] = 1.0
    for d in (1, 512, 1024, 1025):
        t[0, 0, d] = 2.0 ** -54
    rs = U.row_sums(np.sqrt(t), np.zeros((1, 1028), np.float32))
    assert rs[0, 0] == 1.0
    t[0, 0, 0], t[0, 0, 1027] = 0.0, 1.0                     # the 1 last: the small ones have joined to 2^-52 by then
    rs = U.row_sums(np.sqrt(t), np.zeros((1, 1028), np.float32))
    assert rs[0, 0] == 1.0 + 2.0 ** -52
    t[0, 0, 8] = 0.25                                        # another slot joins through the butterfly
    assert U.row_sums(np.sqrt(t), np.zeros((1, 1028), np.float32))[0, 0] == 1.25 + 2.0 ** -52


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_curve.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_curve.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert declared and sorted(declared) == sorted(_lib.CURVE_SIGNATURES)
    assert all(n.startswith("qsaec_") for n in declared)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    for name, n_params in declared.items():
        assert len(_lib.CURVE_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaec_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    sizers = {n for n in declared if n.endswith("_bytes")}
    guarded = {entry for entry, *_ in G.GUARD_CASES.values()}
    assert sizers | guarded == set(declared) and not sizers & guarded
    assert all(n + "_workspace_bytes" in sizers for n in guarded)            # every guarded call has its sizer
    assert "sparsity_curve.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in (ROOT / "include" / "qsae_curve.h").read_text()


# ---- calls that need no device ----------------------------------------------------------------------------------------
def _ks(*v):
    return (C.c_int * len(v))(*v)


def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()
    null3 = (None, None, None)

    def binary(B, K, H, D, n_bits, ks, n_ks, group_rows=4):
        return lib.qsaec_prefix_errors_binary(*null3, B, K, None, H, D, n_bits, 1.0, None, ks, n_ks, group_rows, None, None, None,
                                              None, 0, None)

    def table(B, K, H, D, ks, n_ks, group_rows=4):
        return lib.qsaec_prefix_errors_table(*null3, B, K, None, H, D, 1.0, None, ks, n_ks, group_rows, None, None, None, None, 0,
                                             None)
    good = _ks(1, 2, 4)
    for call, name in ((lambda *a, **k: binary(*a[:4], 4, *a[4:], **k), b"qsaec_prefix_errors_binary"),
                       (table, b"qsaec_prefix_errors_table")):
        assert call(0, 8, 64, 16, good, 3) == _lib.OK                                       # B == 0: nothing launched
        assert call(5, 8, 64, 16, _ks(1, 4, 2), 3) == _lib.ERR_INVALID_ARG                  # ks not ascending
        assert name in lib.qsae_last_error()
        assert call(5, 8, 64, 16, _ks(2, 2), 2) == _lib.ERR_INVALID_ARG                     # ks not distinct
        assert call(5, 8, 64, 16, _ks(-1, 2), 2) == _lib.ERR_INVALID_ARG
        assert call(5, 8, 64, 16, _ks(1, 9), 2) == _lib.ERR_INVALID_ARG                     # beyond K
        assert call(5, 8, 64, 16, None, 17) == _lib.ERR_UNSUPPORTED                         # n_ks = 17: ks is not read
        assert call(5, 8, 64, 16, None, 0) == _lib.ERR_UNSUPPORTED
        assert call(5, 257, 512, 16, good, 3) == _lib.ERR_UNSUPPORTED                       # K = 257
        assert call(5, 8, 64, 6, good, 3) == _lib.ERR_UNSUPPORTED                           # D = 6
        assert call(5, 8, 64, 0, good, 3) == _lib.ERR_UNSUPPORTED
        assert call(5, 8, 64, 4100, good, 3) == _lib.ERR_UNSUPPORTED
        assert call(-1, 8, 64, 16, good, 3) == _lib.ERR_INVALID_ARG
        assert call(5, 8, 0, 16, good, 3) == _lib.ERR_INVALID_ARG                           # H = 0
        assert call(5, 8, 64, 16, good, 3, group_rows=0) == _lib.ERR_INVALID_ARG
        assert call(5, 8, 64, 16, good, 3) == _lib.ERR_INVALID_ARG                          # null pointers, before any launch
        assert b"null" in lib.qsae_last_error()
    for bits in (0, 9):
        assert binary(5, 8, 64, 16, bits, good, 3) == _lib.ERR_UNSUPPORTED
    for size in (lib.qsaec_prefix_errors_binary_workspace_bytes, lib.qsaec_prefix_errors_table_workspace_bytes):
        assert size(0, 3, 4) == 0 and size(5, 0, 4) == 0 and size(5, 17, 4) == 0 and size(5, 3, 0) == 0
        # 10 rows x 3 points x 8 -> 256, 10 flags -> 256, 3 groups x 3 x 8 -> 256, 3 flags -> 256
        assert size(10, 3, 4) == 1024
        assert size(10, 3, 4) <= size(11, 3, 4) <= size(11, 4, 4) and size(4096, 16, 1) >= size(4096, 16, 2)


def test_default_ks():
    assert default_ks(65) == [1, 2, 4, 8, 16, 32, 64, 65, 128, 256]
    assert default_ks(32) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert default_ks(0) == [1, 2, 4, 8, 16, 32, 64, 128, 256] == default_ks(300)
    assert default_ks(3) == [1, 2, 3, 4, 8, 16, 32, 64, 128, 256]
    assert {"SparsityCurve", "default_ks", "sparsity_curve"} <= set(dir(inference))


def test_front_ends_refuse_host_tensors():
    x, idx, val = torch.zeros(2, 4), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2)
    sums, counts = torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.int64)
    for mod in (ops, torch_ops):
        for decoder in (("table", torch.zeros(8, 4), 1.0), ("packed", torch.zeros(8, 4, dtype=torch.uint8), 4, 0.5)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                mod.prefix_errors(x, idx, val, [2], decoder, None, 4, sums, counts)
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        curve = SparsityCurve(model, ks=[1, 2])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            curve.add(x)
        with pytest.raises(ValueError, match="no row was added"):
            curve.finish()


def test_front_end_refuses_the_classes_whose_sparsity_is_not_a_k():
    others = (TernarySparseAutoencoder(4, 8), QuantizedMatryoshkaSAE(4, 32, top_k=2, n_bits=4),
              ResidualQuantizedSAE(4, 32, top_k=2, n_bits=4), BinaryLatentSAE(4, 8))
    for model in others:
        with pytest.raises(TypeError, match="not a k") as e:
            SparsityCurve(model)
        assert "compute_reconstruction_error_by_level" in str(e.value)


def test_front_end_validates_ks():
    model = BaselineSparseAutoencoder(4, 512)
    assert SparsityCurve(model).ks == [1, 2, 4, 8, 16, 32, 64, 128, 256] and SparsityCurve(model).model_k == 32
    assert SparsityCurve(BaselineSparseAutoencoder(4, 8)).ks == [1, 2, 4, 8]               # cut at hidden_dim
    for bad in ([], [2, 1], [1, 1], [-1, 2], [1, 257], list(range(17))):
        with pytest.raises(ValueError):
            SparsityCurve(model, ks=bad)
    with pytest.raises(ValueError, match="group_rows"):
        SparsityCurve(model, group_rows=0)
    with pytest.raises(ValueError, match="hidden_dim"):
        SparsityCurve(BaselineSparseAutoencoder(4, 8), ks=[1, 9])


# ---- the kernel's own source on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sparsity_curve_emu")


@pytest.fixture(scope="module")
def emu(build_dir):
    return compile_emu(build_dir, "sparsity_curve_emu.cpp", "curve_emu", include=(CSRC,))


@pytest.fixture(scope="module")
def emu_asan(build_dir):
    return compile_emu(build_dir, "sparsity_curve_emu.cpp", "curve_emu_asan", include=(CSRC,), asan=True)


def _run(exe: Path, d: Path, case, xoff=0, split=0, want_recon=True):
    x, idx, val, ks, decoder, bias, group_rows = case
    B, D = x.shape
    K = idx.shape[1]
    x.tofile(d / "x.bin")
    idx.tofile(d / "idx.bin")
    val.tofile(d / "val.bin")
    np.ascontiguousarray(decoder[1]).tofile(d / "dict.bin")
    if bias is not None:
        bias.tofile(d / "bias.bin")
    packed = decoder[0] == "packed"
    cmd = ["p" if packed else "t", "x.bin", B, D, "idx.bin", "val.bin", K, "dict.bin", decoder[1].shape[0],
           decoder[3] if packed else 0, repr(float(decoder[-1])), "-" if bias is None else "bias.bin", ",".join(str(k) for k in ks),
           group_rows, xoff, split, "sums.bin", "counts.bin", "recon.bin" if want_recon else "-"]
    run_emu(exe, cmd, d, 900)
    recon = np.fromfile(d / "recon.bin", np.float32).reshape(len(ks), B, D) if want_recon and not split else None
    return np.fromfile(d / "sums.bin", np.float64), np.fromfile(d / "counts.bin", np.int64), recon


def _same(got, want):
    (gs, gc, gr), (ws, wc, wr) = got, want
    assert gc.tolist() == wc.tolist()
    assert np.array_equal(gs.view(np.uint64), ws.view(np.uint64))
    if gr is not None:
        assert np.array_equal(gr.view(np.uint32), wr.view(np.uint32))


def _want(case):
    x, idx, val, ks, decoder, bias, group_rows = case
    return U.prefix_errors(x, idx, val, ks, decoder, bias, group_rows)


@pytest.mark.parametrize("name", U.EMU_CASES)
def test_kernel_source_on_the_host_equals_the_restatement(emu, build_dir, name):
    case = U.build_case(name)
    _same(_run(emu, build_dir, case, xoff=1 if "D36" in name else 0), _want(case))


@pytest.mark.parametrize("name", ["packed_B10_nan", "table_B10_nan"])
def test_two_calls_cut_at_a_group_boundary_on_the_host(emu, build_dir, name):
    case = U.build_case(name)
    _same(_run(emu, build_dir, case, split=4), _want(case))


@pytest.mark.parametrize("name", sorted(U.SPECIAL_CASES))
def test_special_values_on_the_host(emu, build_dir, name):
    case = U.special_case(name)
    got = _run(emu, build_dir, case)
    _same(got, _want(case))
    U.check_special(name, case, got[2])


@pytest.mark.parametrize("name", ["packed_D48_n4", "table_D36_s0.5_b0", "packed_D36_n3", "packed_D512_n8"])
def test_sanitizer_build_runs_clean(emu_asan, build_dir, name):
    """The same program with AddressSanitizer: x starts 4 bytes off a 16-byte boundary in a block of exactly its size."""
    case = U.build_case(name)
    _same(_run(emu_asan, build_dir, case, xoff=1), _want(case))


def test_sanitizer_build_with_ids_outside_the_dictionary(emu_asan, build_dir):
    for name in ("packed_ids_outside", "table_ids_outside"):
        case = U.special_case(name)
        _same(_run(emu_asan, build_dir, case), _want(case))
