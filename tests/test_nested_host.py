"""The nested-dictionary objective without a GPU: hand-worked cases of the numpy restatement (tests/nested_util.py); the ledger
of include/qsae_nested.h -- every function declared there is bound in _lib.NESTED_SIGNATURES with as many arguments as it
declares, exported by the product and the debug library as qsaen_*, and is either a *_bytes sizer or driven between guard words
in tests/test_nested_gpu.py; the calls of the C ABI that return before they look at a pointer; default_nested_bounds; the front
ends' refusal of host tensors, of bad bounds and of the four classes without a top-k; and the kernels' own source run on the
CPU (tests/emu, tests/emu_util.py: threads as lanes, real barriers), which must equal the restatement bit for bit, twice on poisoned
outputs, also in a stand-alone build with AddressSanitizer where every operand is a heap block of exactly its size."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import nested_util as U
import test_nested_gpu as G
from quantizedsae_amd import _lib, build, inference, ops, torch_ops, training
from quantizedsae_amd.inference import nested_errors
from quantizedsae_amd.sae import (BaselineSparseAutoencoder, BinaryLatentSAE, BinarySAE, QuantizedMatryoshkaSAE,
                                  ResidualQuantizedSAE, TernarySparseAutoencoder)
from quantizedsae_amd.sae.topk import TopKCore
from quantizedsae_amd.training import Trainer, default_nested_bounds, nested_loss
from sparsity_curve_util import gaussian
from emu_util import CSRC, ROOT, compile_emu, run_emu


# ---- the restatement, by hand -----------------------------------------------------------------------------------------
def _hand():
    # H = 4 atoms over D = 4 columns; the list of every row is (unit 2, unit 0, unit 3) with values (2, 1, 4)
    table = np.array([[1, 0, 0, 0], [9, 9, 9, 9], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
    idx = np.array([[2, 0, 3]] * 2, dtype=np.int32)
    val = np.array([[2, 1, 4]] * 2, dtype=np.float32)
    return table, idx, val


def test_restatement_by_hand_with_a_bound_of_one_unit_and_a_level_without_an_entry():
    table, idx, val = _hand()
    # bounds [1, 2, 3, 4]: unit 0 alone -> (1, 0, 0, 0); nothing new below 2 (unit 1 is not selected); + unit 2; + unit 3
    r = U.nested_recons(idx, val, [1, 2, 3, 4], ("table", table, 1.0), None)
    assert r[:, 0].tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [1, 2, 0, 0], [1, 2, 4, 0]]
    # a scale and a bias: 0.5 * chain + bias; a first level that holds no entry gives the bias
    bias = np.array([1, 1, 1, 1], dtype=np.float32)
    idx[:, 1] = 1                                            # (2, 1, 3): nothing below 1
    r = U.nested_recons(idx, val, [1, 4], ("table", table, 0.5), bias)
    assert r[0, 0].tolist() == [1, 1, 1, 1] and r[1, 0].tolist() == [5.5, 6.5, 7.5, 5.5]
    assert U.levels_of([0, 1, 2, 3], [1, 4]).tolist() == [0, 1, 1, 1]
    assert U.levels_of([0, 32, 33, 63, 64, 511], [1, 33, 64, 512]).tolist() == [0, 1, 2, 2, 3, 3]


def test_restatement_never_touches_an_entry_behind_a_bound():
    table, idx, val = _hand()
    table[3, 3] = np.inf                                      # unit 3 lies behind the bounds 1 and 3
    r = U.nested_recons(idx, val, [1, 3, 4], ("table", table, 1.0), None)
    assert np.isfinite(r[:2]).all() and np.isinf(r[2, :, 3]).all()
    table[3, 3] = np.nan
    val[:, 2] = 0.0                                           # a multiplication by zero would still give NaN
    r = U.nested_recons(idx, val, [1, 3, 4], ("table", table, 1.0), None)
    assert np.isfinite(r[:2]).all() and np.isnan(r[2, :, 3]).all()


def test_restatement_minus_zero_and_ids_out_of_range():
    table, idx, val = _hand()
    val[:] = -0.0
    r = U.nested_recons(idx, val, [1, 4], ("table", table, -0.5), None)
    assert not r.view(np.uint32).any()                        # (+0) + (-0) = +0 at every step: never -0
    table, idx, val = _hand()
    idx[:, 0], idx[:, 2] = 4, -1                              # outside [0, 4): only unit 0 is left
    r = U.nested_recons(idx, val, [1, 4], ("table", table, 1.0), None)
    assert r[0, 0].tolist() == [1, 0, 0, 0] == r[1, 0].tolist()


def test_suffix_sums_skip_absent_levels():
    g = [np.full((1, 4), v, np.float32) for v in (1, 2, 4, 8)]
    assert U.suffix_sums(g, 1, 4)[:, 0, 0].tolist() == [15, 14, 12, 8]
    assert U.suffix_sums([g[0], None, g[2], None], 1, 4)[:, 0, 0].tolist() == [5, 4, 4, 0]
    assert not U.suffix_sums([None] * 4, 1, 4).view(np.uint32).any()
    # fp32, from the last level down: with t = 0.75 * 2^-24, 1 + (t + t) rounds up and (1 + t) + t does not
    tiny = np.full((1, 4), 0.75 * 2.0 ** -24, np.float32)
    one = np.ones((1, 4), np.float32)
    assert U.suffix_sums([one, tiny, tiny], 1, 4)[0, 0, 0] == np.float32(1.0 + 2.0 ** -23)
    assert U.suffix_sums([tiny, tiny, one], 1, 4)[0, 0, 0] == np.float32(1.0)


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_nested.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_nested.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 7 and sorted(declared) == sorted(_lib.NESTED_SIGNATURES)
    assert all(n.startswith("qsaen_") for n in declared)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.CURVE_SIGNATURES))
    for name, n_params in declared.items():
        assert len(_lib.NESTED_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaen_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    sizers = {n for n in declared if n.endswith("_bytes")}
    guarded = {entry for entry, *_ in G.GUARD_CASES.values()}
    assert sizers | guarded == set(declared) and not sizers & guarded
    assert all(n[:-len("_workspace_bytes")] in guarded for n in sizers)      # every sizer belongs to a guarded call
    assert "nested.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in (ROOT / "include" / "qsae_nested.h").read_text()
    assert "qsae_nested.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()


# ---- calls that need no device ----------------------------------------------------------------------------------------
def _ints(*v):
    return (C.c_int * len(v))(*v)


def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()

    def binary(B, k, H, D, bounds, L, n_bits=4):
        return lib.qsaen_decode_nested_binary(None, None, B, k, None, H, D, n_bits, 1.0, None, bounds, L, None, None)

    def table(B, k, H, D, bounds, L):
        return lib.qsaen_decode_nested_table(None, None, B, k, None, H, D, 1.0, None, bounds, L, None, None)

    def row(B, k, H, D, bounds, L):
        g = (C.c_void_p * 8)()
        return lib.qsaen_row_grad_nested(None, B, k, None, H, D, 1.0, g, bounds, L, None, 0, None, None, None, None, None)

    def unit(B, k, H, D, bounds, L, n_bits=4):
        return lib.qsaen_train_unit_grad_nested(None, None, None, None, B, k, None, None, bounds, L, None, H, D, n_bits, 1.0, None,
                                                None, None, None, None, 0, None)

    def table_unit(B, k, H, D, bounds, L):
        return lib.qsaen_train_table_unit_grad_nested(None, None, None, None, B, k, None, None, bounds, L, H, D, None, None, None,
                                                      H, None, 0, None)
    good = _ints(1, 8, 64)
    for call, name in ((binary, b"qsaen_decode_nested_binary"), (table, b"qsaen_decode_nested_table"),
                       (row, b"qsaen_row_grad_nested"), (unit, b"qsaen_train_unit_grad_nested"),
                       (table_unit, b"qsaen_train_table_unit_grad_nested")):
        assert call(5, 8, 64, 16, _ints(1, 64, 8), 3) == _lib.ERR_INVALID_ARG                # bounds not ascending
        assert name in lib.qsae_last_error()
        assert call(5, 8, 64, 16, _ints(8, 8, 64), 3) == _lib.ERR_INVALID_ARG                # not distinct
        assert call(5, 8, 64, 16, _ints(0, 8, 64), 3) == _lib.ERR_INVALID_ARG                # bounds[0] == 0
        assert call(5, 8, 64, 16, _ints(1, 8, 63), 3) == _lib.ERR_INVALID_ARG                # the last bound is not H
        assert call(5, 8, 64, 16, None, 3) == _lib.ERR_INVALID_ARG                           # bounds is null
        assert call(5, 8, 64, 16, None, 9) == _lib.ERR_UNSUPPORTED                           # 9 levels: bounds is not read
        assert call(5, 8, 64, 16, None, 0) == _lib.ERR_UNSUPPORTED
        assert call(5, 257, 512, 16, good, 3) == _lib.ERR_UNSUPPORTED                        # k = 257
        assert call(5, 8, 64, 6, good, 3) == _lib.ERR_UNSUPPORTED                            # D = 6
        assert call(5, 8, 64, 0, good, 3) == _lib.ERR_UNSUPPORTED
        assert call(5, 8, 64, 4100, good, 3) == _lib.ERR_UNSUPPORTED
        assert call(1 << 23, 256, 64, 16, good, 3) == _lib.ERR_UNSUPPORTED                   # B * k = 2^31
        assert call(-1, 8, 64, 16, good, 3) == _lib.ERR_INVALID_ARG
        assert call(5, 8, 0, 16, _ints(0), 1) == _lib.ERR_INVALID_ARG                        # H = 0
        assert call(5, 8, 64, 16, good, 3) == _lib.ERR_INVALID_ARG                           # null pointers, before any launch
        assert b"null" in lib.qsae_last_error()
    for call in (binary, table, row):
        assert call(0, 8, 64, 16, good, 3) == _lib.OK                                        # B == 0: nothing launched
    for bits in (0, 9):
        assert binary(5, 8, 64, 16, good, 3, n_bits=bits) == _lib.ERR_UNSUPPORTED
        assert unit(5, 8, 64, 16, good, 3, n_bits=bits) == _lib.ERR_UNSUPPORTED
    for size, plain in ((lib.qsaen_train_unit_grad_nested_workspace_bytes, lib.qsae_train_unit_grad_workspace_bytes),
                        (lib.qsaen_train_table_unit_grad_nested_workspace_bytes, lib.qsae_train_table_unit_grad_workspace_bytes)):
        assert size(7, 6, 512, 48) == plain(7, 6, 512, 48) > 0                               # the layout of the calls they extend
        assert size(7, 6, 512, 6) == 0 and size(7, 257, 512, 48) == 0 and size(7, 6, 0, 48) == 0


def test_default_nested_bounds():
    assert default_nested_bounds(32768) == [4096, 8192, 16384, 32768] == TopKCore.default_nested_bounds(32768, levels=4)
    assert default_nested_bounds(512, 1) == [512] and default_nested_bounds(512, 8) == [4, 8, 16, 32, 64, 128, 256, 512]
    assert BinarySAE.default_nested_bounds(24, 3) == [6, 12, 24] == BaselineSparseAutoencoder.default_nested_bounds(24, 3)
    for H, levels in ((512, 0), (512, 9), (4, 4), (0, 1)):   # too many levels, or a first prefix without a unit
        with pytest.raises(ValueError):
            default_nested_bounds(H, levels)
    assert {"nested_loss", "default_nested_bounds"} <= set(training.__all__) and "nested_errors" in dir(inference)
    assert ops.nested_bounds((1, 2, 8), 8) == [1, 2, 8] == torch_ops.nested_bounds([1, 2, 8], 8)
    for bad in ([], [0, 8], [2, 2, 8], [4, 2, 8], [2, 4], [2, 9], list(range(1, 10)), [1.5, 8], None):
        with pytest.raises(ValueError, match="bounds|levels"):
            ops.nested_bounds(bad, 8)


def test_front_ends_refuse_host_tensors_and_bad_bounds():
    idx, val, x = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2), torch.zeros(2, 4)
    table, packed = torch.zeros(8, 4), torch.zeros(8, 4, dtype=torch.uint8)
    off, ent = torch.zeros(9, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for mod in (ops, torch_ops):
        for call in (lambda: mod.decode_nested_table(idx, val, table, 1.0, None, [4, 8]),
                     lambda: mod.decode_nested_binary(idx, val, packed, 4, 8, 0.5, None, [4, 8]),
                     lambda: mod.train_row_grad_nested(idx, table, 1.0, [None, None], [4, 8], None, None),
                     lambda: mod.train_unit_grad_nested(off, ent, val, val, x, None, [4, 8], torch.zeros(8, 16), 4, 0.5, None),
                     lambda: mod.train_table_unit_grad_nested(off, ent, val, val, x, None, [4, 8])):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        for call in (lambda: model.forward_nested(x, [4, 8]), lambda: model.forward_train_nested(x, [4, 8]),
                     lambda: nested_errors(model, [x], [4, 8])):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
        with pytest.raises(ValueError, match="empty loader"):
            nested_errors(model, [], [4, 8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nested_loss("baseline_sae", (None, (x,)), x, {})


def test_front_ends_refuse_the_four_classes_without_a_top_k(tmp_path):
    others = (TernarySparseAutoencoder(4, 8), QuantizedMatryoshkaSAE(4, 32, top_k=2, n_bits=4),
              ResidualQuantizedSAE(4, 32, top_k=2, n_bits=4), BinaryLatentSAE(4, 8))
    for model in others:
        assert not hasattr(model, "forward_nested") and not hasattr(model, "forward_train_nested")
        with pytest.raises(TypeError, match="not a k") as e:
            nested_errors(model, [torch.zeros(2, 4)])
        assert "compute_reconstruction_error_by_level" in str(e.value)
    config = {"input_dim": 4, "n_bits": 4, "hidden_dim": 32, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 2,
              "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 8}
    for sae_type in ("t_sae", "bl_sae", "q_sae", "rq_sae"):
        with pytest.raises(ValueError, match="two top-k models"):
            Trainer(config, sae_type, True, True, dataset_dir=str(tmp_path), save_dir=str(tmp_path), nested_bounds="default")
        with pytest.raises(ValueError, match="two top-k models"):
            nested_loss(sae_type, (None, ()), torch.zeros(2, 4), config)
    for bad in ("levels", [8, 8, 32], [8, 16], []):
        with pytest.raises(ValueError, match="bounds|levels"):
            Trainer(config, "baseline_sae", False, True, model=BaselineSparseAutoencoder(4, 32), dataset_dir=str(tmp_path),
                    save_dir=str(tmp_path), nested_bounds=bad)


# ---- the kernels' own source on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("nested_emu")


@pytest.fixture(scope="module")
def emu(build_dir):
    return compile_emu(build_dir, "nested_emu.cpp", "nested_emu", include=(CSRC,))


@pytest.fixture(scope="module")
def emu_asan(build_dir):
    return compile_emu(build_dir, "nested_emu.cpp", "nested_emu_asan", include=(CSRC,), asan=True)


def _run(exe: Path, d: Path, case):
    idx, val, bounds, decoder, bias = case
    B, k = idx.shape
    np.ascontiguousarray(idx).tofile(d / "idx.bin")
    np.ascontiguousarray(val).tofile(d / "val.bin")
    np.ascontiguousarray(decoder[1]).tofile(d / "dict.bin")
    if bias is not None:
        bias.tofile(d / "bias.bin")
    packed = decoder[0] == "packed"
    D = decoder[2] if packed else decoder[1].shape[1]
    cmd = ["p" if packed else "t", "idx.bin", "val.bin", B, k, "dict.bin", decoder[1].shape[0], D, decoder[3] if packed else 0,
           repr(float(decoder[-1])), "-" if bias is None else "bias.bin", ",".join(str(b) for b in bounds), "recon.bin"]
    run_emu(exe, cmd, d, 900)
    return np.fromfile(d / "recon.bin", np.float32).reshape(len(bounds), B, D)


def _same(got, want):
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", U.EMU_CASES)
def test_kernel_source_on_the_host_equals_the_restatement(emu, build_dir, name):
    case = U.build_case(name)
    _same(_run(emu, build_dir, case), U.nested_recons(*case))


@pytest.mark.parametrize("name", sorted(U.SPECIAL_CASES))
def test_special_values_on_the_host(emu, build_dir, name):
    case = U.special_case(name)
    got = _run(emu, build_dir, case)
    _same(got, U.nested_recons(*case))
    U.check_special(name, got)


def test_an_empty_list_on_the_host(emu, build_dir):
    idx, val, bounds, decoder, bias = U.build_case("table_D48_s1.0")
    got = _run(emu, build_dir, (idx[:, :0], val[:, :0], bounds, decoder, bias))
    assert np.array_equal(got, np.broadcast_to(np.float32(0) + bias, got.shape))


def _run_row_grad(exe: Path, d: Path, idx, table, step, g, present, bounds, g_latent, W):
    B, k = idx.shape
    H, D = table.shape
    np.ascontiguousarray(idx).tofile(d / "idx.bin")
    table.tofile(d / "table.bin")
    np.ascontiguousarray(np.stack(g)).tofile(d / "g.bin")
    g_latent.tofile(d / "glat.bin")
    W.tofile(d / "wenc.bin")
    cmd = ["g", "idx.bin", B, k, "table.bin", H, D, repr(float(step)), ",".join(str(b) for b in bounds), "g.bin",
           ",".join(str(int(p)) for p in present), "glat.bin", "wenc.bin", "G.bin", "gv.bin", "dx.bin"]
    run_emu(exe, cmd, d, 900)
    return (np.fromfile(d / "G.bin", np.float32).reshape(len(bounds), B, D), np.fromfile(d / "gv.bin", np.float32).reshape(B, k),
            np.fromfile(d / "dx.bin", np.float32).reshape(B, D))


@pytest.mark.parametrize("asan", [False, True])
@pytest.mark.parametrize("present", [(1, 1, 1, 1), (1, 0, 1, 0), (0, 0, 0, 0)])
def test_row_gradient_source_on_the_host(emu, emu_asan, build_dir, present, asan):
    """G bit for bit against the restatement; gv and dx within 1e-5 of fp64 on the same G (the order of their sums is that of
    qsae_train_row_grad, which the GPU tests compare bit for bit)."""
    idx, val, bounds, _, _ = U.build_case("table_D48_s1.0")
    B, k = idx.shape
    H, D = 512, 48
    table, W = gaussian(71, H, D), gaussian(72, H, D)
    g = [gaussian(80 + l, B, D) for l in range(4)]
    g_latent = gaussian(73, B, H)
    G, gv, dx = _run_row_grad(emu_asan if asan else emu, build_dir, idx, table, 0.5, g, present, bounds, g_latent, W)
    want_G = U.suffix_sums([t if p else None for t, p in zip(g, present)], B, D)
    _same(G, want_G)
    sel = np.take_along_axis(g_latent, idx.astype(np.int64), axis=1)
    w = U.grads64(np.zeros((B, D), np.float32), W, table, 0.5, idx, val, want_G, bounds, sel, want_dx=True)
    assert _close(gv, w["gv"]) and _close(dx, w["x"])


def _close(got, want) -> bool:
    want = want.numpy()
    return float(np.abs(got.astype(np.float64) - want).max()) <= 1e-5 * float(np.abs(want).max())


@pytest.mark.parametrize("name", ["packed_D48_n4", "table_D520_s0.5_nobias", "packed_D4_n1", "packed_k256", "packed_eight_levels"])
def test_sanitizer_build_runs_clean(emu_asan, build_dir, name):
    """The same program with AddressSanitizer: every operand is a heap block of exactly its size."""
    case = U.build_case(name)
    _same(_run(emu_asan, build_dir, case), U.nested_recons(*case))


def test_sanitizer_build_with_ids_outside_the_dictionary(emu_asan, build_dir):
    for name in ("packed_ids_outside", "table_ids_outside"):
        case = U.special_case(name)
        _same(_run(emu_asan, build_dir, case), U.nested_recons(*case))
