"""The dense JumpReLU encoder without a GPU: hand-worked rows of the numpy restatement (tests/jump_dense_util.py); the ledger of
include/qsae_jump_dense.h -- every function declared there is bound in _lib.JUMP_DENSE_SIGNATURES with as many arguments as it
declares, exported by the product and the debug library as qsaed_*, and is either a *_bytes sizer or driven between guard words
in tests/test_jump_dense_gpu.py; the calls of the C ABI that return before they look at a pointer, in the order the header
states; the refusals of the front ends, the models and the Trainer; and the kernels' own source run on the CPU (tests/emu,
tests/emu_util.py: threads as lanes, real barriers, the fp32 MFMA as an fmaf chain), which must equal the restatement bit for
bit, twice on poisoned outputs and a poisoned workspace of exactly the sizer's bytes, also in a stand-alone build with
AddressSanitizer where every operand is a heap block of exactly its size.  The source lines that cannot compile for a host are
rewritten as in tests/test_auxk_emu_host.py."""
import re

import numpy as np
import pytest
import torch

import jump_dense_util as U
import test_jump_dense_gpu as G
from quantizedsae_amd import _lib, build, ops, torch_ops
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinaryLatentSAE, BinarySAE, TernarySparseAutoencoder
from quantizedsae_amd.training import JumpReLU, Trainer
from emu_util import CSRC, ROOT, compile_emu, rewrite, run_emu

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _f(*v):
    return np.array(v, dtype=np.float32)


def _bits(a):
    return U.bits(a)


# ---- the restatement, by hand -----------------------------------------------------------------------------------------
# D = 4, H = 6: units 0 and 1 read x[0] (a tie in value across units), units 2, 3, 4 read x[1], x[2], x[3], unit 5 reads nothing
HAND_W = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]], dtype=np.float32)
HAND_THETA = _f(1.0, 1.0, 2.0, NAN, 0.5, -0.0)               # a NaN threshold; -0 under unit 5, whose pre-activation is +0
HAND_X = np.array([[3, 1, 5, 0.75],                          # K + 1 units fire: 0 and 1 (tied at 3), 4; unit 3 has no threshold
                   [1, 2.125, 0, 0.5],                       # z == theta in units 0, 1 and 4: not selected, in the band
                   [NAN, 0, 0, 0],                           # a NaN in x: NaN * 0 is NaN, the whole row is
                   [2, 0, 0, 0.5]], dtype=np.float32)        # exactly K units fire
HAND_K, HAND_EPS = 2, np.float32(0.5)                        # half_eps = 0.25


def test_rows_by_hand():
    z = U.preact(HAND_X, HAND_W, None)
    assert _bits(z[0]).tolist() == _bits(_f(3, 3, 1, 5, 0.75, 0)).tolist() and np.isnan(z[2]).all()
    sel, band = U.predicates(z, HAND_THETA, HAND_EPS)
    assert sel.tolist() == [[True, True, False, False, True, False], [False, False, True, False, False, False],
                            [False] * 6, [True, True, False, False, False, False]]
    # |0.75 - 0.5| == 0.25 is not in the band; |+0 - -0| = 0 is, though +0 > -0 is false: a band entry that is not selected
    assert band.tolist() == [[False, False, False, False, False, True], [True, True, True, False, True, True],
                             [False] * 6, [False, False, False, False, True, True]]
    idx_sel, val_sel, counts, idx_band, counts_band, l0, report = U.encode_jump(HAND_X, HAND_W, None, HAND_THETA, HAND_K, HAND_EPS)
    # row 0: three fire, the two largest are kept, the tie goes to the smaller unit; row 1: one fires, -1 / +0 behind it
    assert idx_sel.tolist() == [[0, 1], [2, -1], [-1, -1], [0, 1]] and counts.tolist() == [2, 1, 0, 2]
    assert _bits(val_sel).tolist() == _bits(np.array([[3, 3], [2.125, 0], [0, 0], [2, 2]], np.float32)).tolist()
    # row 1's band holds five units -- 2 (2.125), 0 and 1 (1), 4 (0.5), 5 (0) -- of which the first two are listed
    assert idx_band.tolist() == [[5, -1], [2, 0], [-1, -1], [4, 5]] and counts_band.tolist() == [1, 2, 0, 2]
    assert l0 == np.float32(1.5)                             # (3 + 1 + 0 + 2) / 4: the uncapped counts
    assert report.tolist() == [5, 5, 1, 1, 1, 6] and len(U.REPORT_NAMES) == U.REPORT_WORDS == len(report)
    # a bias seeds the chain: -0 + (+0) is +0, and a unit whose pre-activation is its bias fires against a negative threshold
    zb = U.preact(HAND_X[3:], HAND_W, _f(0, 0, 0, 0, 0, -0.0))
    assert _bits(zb[0, 5]) == 0
    got = U.encode_jump(HAND_X[3:], HAND_W, _f(0, 0, 0, 0, 0, -1.5), _f(9, 9, 9, 9, 9, -2.0), 1, HAND_EPS)
    assert got[0].tolist() == [[5]] and got[1].tolist() == [[-1.5]] and got[6].tolist() == [1, 0, 0, 0, 0, 1]
    # -0 and +0 are one value in the rank order: the smaller unit comes first
    order = U.rank_order(_f(0.0, -0.0, 1.0, -0.0), [0, 1, 2, 3])
    assert order.tolist() == [2, 0, 1, 3]


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_jump_dense.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_jump_dense.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 2 and sorted(declared) == sorted(_lib.JUMP_DENSE_SIGNATURES)
    assert all(n.startswith("qsaed_") for n in declared)
    others = (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.CURVE_SIGNATURES, _lib.NESTED_SIGNATURES, _lib.BATCH_SIGNATURES,
              _lib.NESTED_BATCH_SIGNATURES, _lib.MULTIK_SIGNATURES, _lib.JUMP_SIGNATURES)
    assert not any(set(declared) & set(t) for t in others)
    assert not any(n.startswith("qsaed_") for t in others for n in t)
    for name, n_params in declared.items():
        assert len(_lib.JUMP_DENSE_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaed_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    sizers = {n for n in declared if n.endswith("_bytes")}
    guarded = {entry for entry, *_ in G.GUARD_CASES.values()}
    assert sizers | guarded == set(declared) and not sizers & guarded
    assert all(n[:-len("_workspace_bytes")] in guarded for n in sizers)      # every sizer belongs to a guarded call
    assert "jump_dense.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in (ROOT / "include" / "qsae_jump_dense.h").read_text()
    assert "qsae_jump_dense.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()
    assert ops.JUMP_DENSE_MAX_K == torch_ops.JUMP_DENSE_MAX_K == 256 and ops.JUMP_DENSE_REPORT_WORDS == U.REPORT_WORDS
    assert JumpReLU.REPORT_NAMES_DENSE == U.REPORT_NAMES and hasattr(torch.ops.qsae, "encode_jump")


# ---- calls that need no device ----------------------------------------------------------------------------------------
def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()

    def call(B, D, H, K, eps=0.25, ldx=None, ldw=None):
        return lib.qsaed_encode_jump(None, D if ldx is None else ldx, None, D if ldw is None else ldw, None, None, B, D, H, K, eps,
                                     0.5 * eps, None, None, None, None, None, None, None, None, 0, None)

    # sizes that make no sense come first (invalid), then the bandwidth, then what the kernels do not take (unsupported)
    assert call(-1, 8, 64, 8) == _lib.ERR_INVALID_ARG and b"qsaed_encode_jump" in lib.qsae_last_error()
    assert call(5, 8, 64, 0) == _lib.ERR_INVALID_ARG and call(5, 8, 0, 8) == _lib.ERR_INVALID_ARG
    assert call(-1, 8, 64, 257) == _lib.ERR_INVALID_ARG and call(-1, 6, 64, 8) == _lib.ERR_INVALID_ARG
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        assert call(5, 8, 64, 8, eps) == _lib.ERR_INVALID_ARG and b"eps" in lib.qsae_last_error()
        assert call(5, 6, 64, 257, eps) == _lib.ERR_INVALID_ARG                             # ... before anything unsupported
    assert call(5, 8, 512, 257) == _lib.ERR_UNSUPPORTED and b"K <= 256" in lib.qsae_last_error()
    assert call(5, 8, 64, 65) == _lib.ERR_UNSUPPORTED and b"K <= H" in lib.qsae_last_error()
    assert call(5, 6, 512, 257) == _lib.ERR_UNSUPPORTED and b"K <= 256" in lib.qsae_last_error()     # K before D
    for D in (6, 0, -4):
        assert call(5, D, 64, 8) == _lib.ERR_UNSUPPORTED and b"multiple of 4" in lib.qsae_last_error()
    assert call(1 << 23, 8, 512, 256) == _lib.ERR_UNSUPPORTED and b"B * K" in lib.qsae_last_error()
    assert call(1 << 23, 6, 512, 256) == _lib.ERR_UNSUPPORTED and b"multiple of 4" in lib.qsae_last_error()   # D before B * K
    assert call(0, 8, 64, 8) == _lib.OK                                                      # B == 0: nothing launched
    assert call(0, 6, 64, 8) == _lib.ERR_UNSUPPORTED                                         # ... but only for a shape it takes
    # then the strides and the pointers, before any launch
    assert call(5, 8, 64, 8, ldx=4) == _lib.ERR_INVALID_ARG and b"stride" in lib.qsae_last_error()
    assert call(5, 8, 64, 8, ldw=10) == _lib.ERR_INVALID_ARG and b"stride" in lib.qsae_last_error()
    assert call(5, 8, 64, 8) == _lib.ERR_INVALID_ARG and b"null" in lib.qsae_last_error()
    size = lib.qsaed_encode_jump_workspace_bytes
    assert size(7, 8, 512, 6) > 0 and size(0, 8, 512, 6) > 0 and size(8192, 512, 32768, 256) >= size(8191, 512, 32768, 256)
    for refused in ((7, 8, 512, 257), (7, 8, 4, 6), (7, 6, 512, 6), (7, 0, 512, 6), (-1, 8, 512, 6), (7, 8, 0, 6), (7, 8, 512, 0),
                    (1 << 23, 8, 512, 256)):
        assert size(*refused) == 0, refused


def test_front_ends_models_and_trainer_refuse(tmp_path):
    x, W, b, theta = torch.zeros(2, 4), torch.zeros(8, 4), torch.zeros(8), torch.ones(8)
    for mod in (ops, torch_ops):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod.encode_jump(x, W, b, theta, 2, 0.25)
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        jr = JumpReLU(model)
        assert jr.report_names == JumpReLU.REPORT_NAMES
        for call in (lambda: model.forward_jumprelu_dense(x, jr), lambda: model.forward_train_jumprelu_dense(x, jr)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    for other in (TernarySparseAutoencoder(4, 8), BinaryLatentSAE(4, 8)):
        assert not hasattr(other, "forward_jumprelu_dense") and not hasattr(other, "forward_train_jumprelu_dense")
    config = {"input_dim": 4, "n_bits": 4, "hidden_dim": 32, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 2,
              "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 8}

    def trainer(**kw):
        return Trainer(config, "baseline_sae", False, True, model=BaselineSparseAutoencoder(4, 32), dataset_dir=str(tmp_path),
                       save_dir=str(tmp_path), **kw)
    with pytest.raises(ValueError, match="jumprelu_dense needs jumprelu=True"):
        trainer(jumprelu_dense=True)
    assert trainer(jumprelu=True, jumprelu_l0_coef=0.1, jumprelu_dense=True).jumprelu_dense is True
    assert trainer(jumprelu=True, jumprelu_l0_coef=0.1).jumprelu_dense is False           # the default stays the capped path
    assert trainer().jumprelu_dense is False and trainer().jumprelu is None
    # the summary names the dense report's words
    jr = JumpReLU(BaselineSparseAutoencoder(4, 8))
    jr.record(torch.zeros(4, dtype=torch.int32), torch.tensor([5, 6, 1, 1, 0, 9]), dense=True)
    assert jr.summary() == {"selected": 5, "band_entries": 6, "truncated_rows": 1, "empty_rows": 1, "band_truncated_rows": 0,
                            "firing": 9, "l0": 2.25}
    jr.record(torch.zeros(4, dtype=torch.int32), torch.tensor([5, 6, 1, 1, 0, 0x3F000000]))
    assert jr.summary()["uncertified_rows"] == 0 and jr.summary()["theta_min"] == 0.5 and jr.report_names == JumpReLU.REPORT_NAMES


# ---- the kernels' own source on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("jump_dense_emu")
    gemm = (CSRC / "gemm_mfma_f32.h").read_text()
    gemm = rewrite(gemm, 'asm volatile("s_nop 4\\n\\tglobal_load_dwordx4 %0, %1, %2" : "=v"(r[P][i]) : "v"(voff[i]), "s"(base) : "memory");',
                   "r[P][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + voff[i]);")
    gemm = rewrite(gemm, "extern __shared__ __attribute__((aligned(16))) float smem[];", "float* smem = reinterpret_cast<float*>(g_lds);")
    gemm, n = re.subn(r'asm volatile\("s_waitcnt vmcnt\((?:%0|0)\)" ::[^;]*;', ";", gemm)
    assert n == 5
    assert gemm.count('"+v"') == 3
    gemm = gemm.replace('"+v"', '"+x"')
    gemm = rewrite(gemm, '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    src = rewrite((CSRC / "jump_dense.hip").read_text(), '#include "../../include/qsae_jump_dense.h"',
                  f'#include "{ROOT / "include" / "qsae_jump_dense.h"}"')
    (d / "gemm_mfma_f32.h").write_text(gemm)
    (d / "jump_dense_emu.hip").write_text(src)
    return d


@pytest.fixture(scope="module")
def emu(build_dir):
    return compile_emu(build_dir, "jump_dense_emu.cpp", "jump_dense_emu", include=(build_dir,))


@pytest.fixture(scope="module")
def emu_asan(build_dir):
    return compile_emu(build_dir, "jump_dense_emu.cpp", "jump_dense_emu_asan", include=(build_dir,), asan=True)


def _hex(v) -> str:
    return f"{int(_bits(np.array([v], dtype=np.float32))[0]):08x}"


def _run(exe, d, x, W, bias, theta, K, eps, with_band=True, shift=0, pad_x=0, pad_w=0):
    B, D = x.shape
    H = W.shape[0]

    def dump(a, pad, name):
        w = np.full((a.shape[0], D + pad), np.nan, np.float32)      # NaN between D and the row stride
        w[:, :D] = a
        w.tofile(d / name)
    dump(x, pad_x, "x.bin"), dump(W, pad_w, "w.bin")
    if bias is not None:
        np.ascontiguousarray(bias, np.float32).tofile(d / "bias.bin")
    np.ascontiguousarray(theta, np.float32).tofile(d / "theta.bin")
    run_emu(exe, ["x.bin", B, D + pad_x, "w.bin", H, D + pad_w, "-" if bias is None else "bias.bin", "theta.bin", D, K, _hex(eps),
                  _hex(U.half_eps(eps)), "band" if with_band else "noband", shift, "idxsel.bin", "valsel.bin", "counts.bin",
                  "idxband.bin", "countsband.bin", "l0.bin", "report.bin"], d, 900)
    return (np.fromfile(d / "idxsel.bin", np.int32).reshape(B, K), np.fromfile(d / "valsel.bin", np.float32).reshape(B, K),
            np.fromfile(d / "counts.bin", np.int32), np.fromfile(d / "idxband.bin", np.int32).reshape(B, K),
            np.fromfile(d / "countsband.bin", np.int32), np.fromfile(d / "l0.bin", np.float32)[0],
            np.fromfile(d / "report.bin", np.int64))


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), what


#: (B, D, H, K): one tile; a K tail with three splits of the units and, at K = 5 under low thresholds, regions that overflow; a
#: panel tail at 128 rows; more tiles than splits; the widest list
EMU_SHAPES = [(3, 4, 8, 1), (3, 36, 300, 5), (5, 36, 300, 64), (130, 4, 8, 5), (2, 64, 1100, 65), (3, 8, 600, 256)]


#: every shape plain; under the sanitizer all but the panel tail (its 130 rows differ from the others in the row count alone)
EMU_RUNS = [(s, False) for s in EMU_SHAPES] + [(s, True) for s in EMU_SHAPES if s[0] <= 128]


@pytest.mark.parametrize("shape,asan", EMU_RUNS, ids=lambda v: ("asan" if v else "plain") if isinstance(v, bool) else "x".join(map(str, v)))
def test_kernel_source_on_the_host_equals_the_restatement(emu, emu_asan, build_dir, shape, asan):
    exe, d = (emu_asan if asan else emu), build_dir
    B, D, H, K = shape
    for kind in U.KINDS:
        x, W, bias, theta, eps = U.case(kind, B, D, H, seed=3, quantile=G._quantile(H, K))
        want = U.encode_jump(x, W, bias, theta, K, eps)
        if (H, K) == (300, 5) and kind in ("all", "mixed"):
            assert int(want[6][2]) > B / 2                   # the rows that a region cannot hold: the resolve kernel ran
        got = _run(exe, d, x, W, bias, theta, K, eps, shift=4 if kind == "special" else 0, pad_x=4 if kind == "mixed" else 0,
                   pad_w=8 if kind == "mixed" else 0)
        for g, w, name in zip(got, want, U.NAMES):
            _same(g, w, f"{kind} {shape}: {name}")
        if kind == "special":                                # without the band lists and the bias
            want = U.encode_jump(x, W, None, theta, K, eps)
            got = _run(exe, d, x, W, None, theta, K, eps, with_band=False)
            for i in (0, 1, 2, 5, 6):
                _same(got[i], want[i], f"{kind} {shape}: {U.NAMES[i]} without band lists")
            assert (_bits(got[3]) == 0x5A5A5A5A).all() and (_bits(got[4]) == 0x5A5A5A5A).all()


def test_hand_rows_on_the_host(emu_asan, build_dir):
    want = U.encode_jump(HAND_X, HAND_W, None, HAND_THETA, HAND_K, HAND_EPS)
    for g, w, name in zip(_run(emu_asan, build_dir, HAND_X, HAND_W, None, HAND_THETA, HAND_K, HAND_EPS), want, U.NAMES):
        _same(g, w, name)
