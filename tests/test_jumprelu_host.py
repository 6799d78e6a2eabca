"""JumpReLU without a GPU: hand-worked cases of the numpy restatement (tests/jumprelu_util.py); the ledger of
include/qsae_jump.h -- every function declared there is bound in _lib.JUMP_SIGNATURES with as many arguments as it declares,
exported by the product and the debug library as qsaej_*, and is either a *_bytes sizer or driven between guard words in
tests/test_jumprelu_gpu.py; the calls of the C ABI that return before they look at a pointer, in the order the header states;
the refusals of the front ends, the controller and the Trainer; and the kernels' own source run on the CPU (tests/emu, tests/emu_util.py:
threads as lanes, real barriers), which must equal the restatement bit for bit, twice on poisoned outputs and a poisoned
workspace of exactly the sizer's bytes, also in a stand-alone build with AddressSanitizer where every operand is a heap block of
exactly its size."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import batch_topk_util as BU
import jumprelu_util as U
import test_jumprelu_gpu as G
from quantizedsae_amd import _lib, build, ops, torch_ops, training
from quantizedsae_amd.sae import (BaselineSparseAutoencoder, BinaryLatentSAE, BinarySAE, QuantizedMatryoshkaSAE,
                                  ResidualQuantizedSAE, TernarySparseAutoencoder)
from quantizedsae_amd.training import BatchTopK, JumpReLU, Trainer
from emu_util import CSRC, ROOT, compile_emu, run_emu

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _f(*v):
    return np.array(v, dtype=np.float32)


def _bits(a):
    return U.bits(a)


# ---- the restatement, by hand -----------------------------------------------------------------------------------------
def test_selection_by_hand():
    eps = np.float32(0.5)                                    # half_eps = 0.25
    theta = _f(1.0, 2.0, 0.5, NAN, INF, 0.0)
    #            = theta   NaN val  id -1  id H  above   below, in band   theta NaN   theta inf   -0 against +0
    idx = np.array([[0, 1, -1, 6, 2, 0, 3, 4, 5]], dtype=np.int32)
    val = _f(1.0, NAN, 9.0, 9.0, 0.75, 0.875, 7.0, INF, -0.0)[None]
    sel, band = U.predicates(idx, val, theta, eps)
    assert sel[0].tolist() == [False, False, False, False, True, False, False, False, False]
    #  |1 - 1| = 0 < .25; |.75 - .5| == .25 is not in the band; |.875 - 1| = .125 is; inf - inf is NaN; |-0 - 0| = 0 is
    assert band[0].tolist() == [True, False, False, False, False, True, False, False, True]
    idx_sel, val_sel, counts, idx_band, counts_band, l0, report = U.jump_select(idx, val, theta, eps)
    # an unselected entry ranked before a selected one: the selected one moves to the front, the others keep their order
    assert idx_sel[0].tolist() == [2, 0, 1, -1, 6, 0, 3, 4, 5] and counts.tolist() == [1]
    assert _bits(val_sel)[0].tolist() == [int(_bits(_f(0.75))[0])] + [0] * 8
    assert idx_band[0].tolist() == [0, 0, 5, 1, -1, 6, 2, 3, 4] and counts_band.tolist() == [3]
    assert l0 == np.float32(1.0)
    # theta_min skips the NaN: 0.0; K = 9 > H = 6, so no row is uncertified whatever its last value
    assert report.tolist() == [1, 3, 0, 0, 0, 0]


def test_theta_min_and_the_certificate_by_hand():
    assert _bits(_f(U.theta_min(_f(0.0, -0.0, 3.0))))[0] == 0x80000000       # of -0 and +0 the -0
    assert _bits(_f(U.theta_min(_f(NAN, NAN))))[0] == U.QUIET_NAN_BITS
    assert U.theta_min(_f(NAN, -INF, 2.0)) == -INF and U.theta_min(_f(INF)) == INF
    theta = _f(1.0, 0.5, 2.0, 0.75)
    idx = np.array([[0, 1], [2, 3], [1, 0]], dtype=np.int32)
    val = _f(3.0, 0.375, 3.0, 0.25, 3.0, 0.125).reshape(3, 2)
    # theta_min - half_eps = 0.5 - 0.125 = 0.375: a last value of 0.375 is not below it, 0.25 and 0.125 are
    rep = U.jump_select(idx, val, theta, np.float32(0.25))[6]
    assert rep.tolist() == [3, 0, 0, 0, 1, int(_bits(_f(0.5))[0])]
    assert U.jump_select(idx, val, _f(1.0, 0.5), np.float32(0.25))[6][4] == 0             # K == H: every row is certified
    assert U.jump_select(idx, val, _f(NAN, NAN, NAN), np.float32(0.25))[6][4] == 3         # no threshold to certify against
    sat = U.jump_select(idx, val, np.full(4, -INF, np.float32), np.float32(0.25))
    assert sat[6][:4].tolist() == [6, 0, 3, 0] and sat[5] == np.float32(2.0)
    emp = U.jump_select(idx, val, np.full(4, INF, np.float32), np.float32(0.25))
    assert emp[6][:4].tolist() == [0, 0, 0, 3] and not _bits(emp[1]).any() and np.array_equal(emp[0], idx)


def test_threshold_gradient_by_hand():
    # unit 1 is in the band in rows 0 and 2 (entries 0 * 2 + 1 = 1 and 2 * 2 + 0 = 4), unit 0 nowhere, unit 2 in row 1
    offsets = np.array([0, 0, 2, 3], dtype=np.int32)
    entries = np.array([1, 4, 2, -1, -1, -1], dtype=np.int32)
    gv = _f(9, 0.5, -2.0, 9, 0.25, 9).reshape(3, 2)
    theta = _f(5.0, 2.0, 4.0)
    d = U.threshold_grad(offsets, entries, gv, theta, np.float32(3.0), 3, np.float32(0.5))
    #   -(2 * (0.5 + 0.25) + 3 * 2 / 3) / 0.5 = -7;   -(4 * -2 + 3 * 1 / 3) / 0.5 = 14
    assert d.tolist() == [0.0, -7.0, 14.0] and not np.signbit(d[0])
    assert U.threshold_grad(offsets, entries, gv, theta, None, 3, np.float32(0.5)).tolist() == [0.0, -3.0, 16.0]
    assert U.threshold_grad(offsets, entries, None, theta, np.float32(3.0), 3, np.float32(0.5)).tolist() == [0.0, -4.0, -2.0]
    # fp64 inside, one rounding: 2^-30 survives next to 1 in the sum (an fp32 sum would lose it and give -0)
    gv2 = _f(1.0, 2.0 ** -30, -1.0).reshape(1, 3)
    d2 = U.threshold_grad(np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32), gv2, _f(1.0), None, 1, np.float32(2.0 ** -30))
    assert d2.tolist() == [-1.0]


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_jump.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_jump.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 3 and sorted(declared) == sorted(_lib.JUMP_SIGNATURES)
    assert all(n.startswith("qsaej_") for n in declared)
    others = (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.CURVE_SIGNATURES, _lib.NESTED_SIGNATURES, _lib.BATCH_SIGNATURES,
              _lib.NESTED_BATCH_SIGNATURES, _lib.MULTIK_SIGNATURES)
    assert not any(set(declared) & set(t) for t in others)
    for name, n_params in declared.items():
        assert len(_lib.JUMP_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaej_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    sizers = {n for n in declared if n.endswith("_bytes")}
    guarded = {entry for entry, *_ in G.GUARD_CASES.values()}
    assert sizers | guarded == set(declared) and not sizers & guarded
    assert all(n[:-len("_workspace_bytes")] in guarded for n in sizers)      # every sizer belongs to a guarded call
    assert "jumprelu.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in (ROOT / "include" / "qsae_jump.h").read_text()
    assert "qsae_jump.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()
    assert ops.JUMP_MAX_K == torch_ops.JUMP_MAX_K == 256 and ops.JUMP_REPORT_WORDS == U.REPORT_WORDS


# ---- calls that need no device ----------------------------------------------------------------------------------------
def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()

    def select(B, K, H, eps=0.25):
        return lib.qsaej_jump_select(None, None, B, K, None, H, eps, 0.5 * eps, None, None, None, None, None, None, None, None, 0,
                                     None)

    def grad(B, K, H, eps=0.25):
        return lib.qsaej_threshold_grad(None, None, None, None, None, B, K, H, eps, None, None)

    for call, name in ((select, b"qsaej_jump_select"), (grad, b"qsaej_threshold_grad")):
        assert call(5, 257, 64) == _lib.ERR_UNSUPPORTED                                       # K = 257
        assert name in lib.qsae_last_error()
        assert call(1 << 23, 256, 64) == _lib.ERR_UNSUPPORTED                                 # B * K = 2^31
        assert call(-1, 8, 64) == _lib.ERR_INVALID_ARG
        assert call(-1, 257, 64) == _lib.ERR_INVALID_ARG                                      # sizes that make no sense come first
        assert call(5, 0, 64) == _lib.ERR_INVALID_ARG
        assert call(5, 8, 0) == _lib.ERR_INVALID_ARG                                          # H = 0
        for eps in (0.0, -1.0, float("inf"), float("nan")):
            assert call(5, 8, 64, eps) == _lib.ERR_INVALID_ARG
            assert b"eps" in lib.qsae_last_error()
            assert call(5, 257, 64, eps) == _lib.ERR_INVALID_ARG                              # ... and so does the bandwidth
        assert call(5, 8, 64) == _lib.ERR_INVALID_ARG                                         # null pointers, before any launch
        assert b"null" in lib.qsae_last_error()
    assert select(0, 8, 64) == _lib.OK                                                        # B == 0: nothing launched
    assert grad(0, 8, 64) == _lib.ERR_INVALID_ARG and b"null" in lib.qsae_last_error()        # ... but dtheta is still written
    size = lib.qsaej_jump_select_workspace_bytes
    assert size(7, 6, 512) > 0 and size(0, 6, 512) > 0
    assert size(7, 257, 512) == 0 and size(7, 6, 0) == 0 and size(-1, 6, 512) == 0 and size(7, 0, 512) == 0
    assert size(1 << 23, 256, 512) == 0


def test_front_ends_refuse_host_tensors_and_bad_values():
    idx, val, theta = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2), torch.ones(8)
    off, ent = torch.zeros(9, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for mod in (ops, torch_ops):
        for call in (lambda: mod.jump_select(idx, val, theta, 0.25), lambda: mod.jump_threshold_grad(off, ent, val, theta, None, 2, 2, 0.25)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    assert ops.jump_half_eps(1e-3) == float(U.half_eps(1e-3)) and ops.jump_half_eps(0.5) == 0.25
    for eps in (0.0, -1.0, float("inf"), float("nan"), 1e-50):
        with pytest.raises(ValueError, match="bandwidth"):
            ops._jump_eps("jump_select", eps)
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        jr = JumpReLU(model)
        for call in (lambda: model.forward_jumprelu(val.new_zeros(2, 4), jr), lambda: model.forward_train_jumprelu(val.new_zeros(2, 4), jr),
                     lambda: jr.calibrate(val.new_zeros(2, 4), 2)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_controller_and_trainer_validation(tmp_path):
    model = BaselineSparseAutoencoder(4, 512)
    jr = JumpReLU(model)
    assert jr.cap == 256 and jr.bandwidth == 1e-3 and JumpReLU(BaselineSparseAutoencoder(4, 16)).cap == 16
    assert isinstance(jr, torch.nn.Module) and [n for n, _ in jr.named_parameters()] == ["log_threshold"]
    assert tuple(jr.log_threshold.shape) == (512,) and jr.log_threshold.dtype == torch.float32
    assert torch.allclose(jr.thresholds(), torch.full((512,), 1e-3)) and not jr.thresholds().requires_grad
    assert torch.allclose(JumpReLU(model, init_threshold=0.5).thresholds(), torch.full((512,), 0.5))
    assert "JumpReLU" in training.__all__ and "paper" in training.jumprelu.__doc__ and "normalised" in training.jumprelu.__doc__
    for kwargs, match in (({"cap": 0}, "cap"), ({"cap": 257}, "cap"), ({"cap": 600}, "cap"), ({"bandwidth": 0.0}, "bandwidth"),
                          ({"bandwidth": float("inf")}, "bandwidth"), ({"bandwidth": float("nan")}, "bandwidth"),
                          ({"init_threshold": 0.0}, "init_threshold"), ({"init_threshold": -1.0}, "init_threshold")):
        with pytest.raises(ValueError, match=match):
            JumpReLU(model, **kwargs)
    with pytest.raises(ValueError, match="cap"):
        JumpReLU(BaselineSparseAutoencoder(4, 16), cap=17)
    for other in (TernarySparseAutoencoder(4, 8), QuantizedMatryoshkaSAE(4, 32, top_k=2, n_bits=4),
                  ResidualQuantizedSAE(4, 32, top_k=2, n_bits=4), BinaryLatentSAE(4, 8)):
        assert not hasattr(other, "forward_jumprelu")
        with pytest.raises(TypeError, match="top-k"):
            JumpReLU(other)
        with pytest.raises(TypeError) as batch_wording:
            BatchTopK(other)
        with pytest.raises(TypeError) as jump_wording:
            JumpReLU(other)
        assert str(jump_wording.value) == str(batch_wording.value).replace("BatchTopK", "JumpReLU")
    with pytest.raises(ValueError, match="no selection"):
        jr.summary()
    sd = jr.state_dict()
    assert "log_threshold" in sd and not any("encoder" in k or "decoder" in k for k in sd)    # the model is not a submodule
    sd["log_threshold"] = torch.full((512,), -1.0)
    jr.load_state_dict(sd)
    assert float(jr.log_threshold.detach()[7]) == -1.0
    with pytest.raises(ValueError, match="cap"):
        JumpReLU(model, cap=16).load_state_dict(sd)
    with pytest.raises(ValueError, match="bandwidth"):
        JumpReLU(model, bandwidth=0.5).load_state_dict(sd)
    assert not any("threshold" in key for key in model.state_dict())                          # the models' keys stay the reference's
    with pytest.raises(ValueError, match="k = 300"):
        jr.calibrate(torch.zeros(2, 4), 300)
    with pytest.raises(TypeError, match="BatchTopK"):
        jr.load_from(3.0)
    # load_from: a threshold > 0 is taken over, anything else leaves the thresholds as they are (a CPU controller: torch only)
    ctl = BatchTopK(model, k=8)
    jr.load_from(ctl)
    assert float(jr.log_threshold.detach()[7]) == -1.0
    ctl.theta = torch.tensor(0.25)
    jr.load_from(ctl)
    assert torch.equal(jr.thresholds(), torch.full((512,), 0.25))

    config = {"input_dim": 4, "n_bits": 4, "hidden_dim": 32, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 2,
              "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 8}

    def trainer(sae_type="baseline_sae", **kw):
        model = {"baseline_sae": lambda: BaselineSparseAutoencoder(4, 32), "b_sae": lambda: BinarySAE(4, 32, gamma=4.0, n_bits=4)}.get(sae_type)
        return Trainer(config, sae_type, sae_type == "t_sae", True, model=model() if model else None, dataset_dir=str(tmp_path),
                       save_dir=str(tmp_path), **kw)
    for sae_type in ("t_sae", "bl_sae", "q_sae", "rq_sae"):
        with pytest.raises(ValueError, match="two top-k models"):
            trainer(sae_type, jumprelu=True, jumprelu_l0_coef=0.1)
    for kw, name in (({"batch_topk": True}, "batch_topk"), ({"nested_bounds": "default"}, "nested_bounds"),
                     ({"batch_topk": True, "batch_topk_nested_bounds": "default"}, "batch_topk"),
                     ({"multi_topk": "default"}, "multi_topk")):
        with pytest.raises(ValueError, match=f"jumprelu together with {name}"):
            trainer(jumprelu=True, jumprelu_l0_coef=0.1, **kw)
    with pytest.raises(ValueError, match="jumprelu_l0_coef"):
        trainer(jumprelu=True)                                                                # no default is invented
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="jumprelu_l0_coef"):
            trainer(jumprelu=True, jumprelu_l0_coef=bad)
    with pytest.raises(ValueError, match="jumprelu_init"):
        trainer(jumprelu=True, jumprelu_l0_coef=0.1, jumprelu_init="auto")
    with pytest.raises(ValueError, match="cap"):
        trainer(jumprelu=True, jumprelu_l0_coef=0.1, jumprelu_cap=33)
    with pytest.raises(ValueError, match="calibrate"):
        trainer(jumprelu=True, jumprelu_l0_coef=0.1, jumprelu_cap=1, jumprelu_init="calibrate")   # the model's k = 2 > cap
    for kw in ({"jumprelu_l0_coef": 0.1}, {"jumprelu_cap": 8}, {"jumprelu_init": 0.5}):
        with pytest.raises(ValueError, match="needs jumprelu=True"):
            trainer(**kw)
    for sae_type in ("baseline_sae", "b_sae"):
        t = trainer(sae_type, jumprelu=True, jumprelu_l0_coef=0.1, jumprelu_cap=8, jumprelu_bandwidth=0.5, jumprelu_init=0.25)
        assert (t.jumprelu.cap, t.jumprelu.bandwidth, t.jumprelu_l0_coef) == (8, 0.5, 0.1) and not t._jumprelu_calibrate
        assert torch.allclose(t.jumprelu.thresholds(), torch.full((32,), 0.25))
        assert trainer(sae_type, jumprelu=True, jumprelu_l0_coef=0.0, jumprelu_init="calibrate")._jumprelu_calibrate
        assert trainer(sae_type).jumprelu is None


# ---- the kernels' own source on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("jumprelu_emu")


@pytest.fixture(scope="module")
def emu(build_dir):
    return compile_emu(build_dir, "jumprelu_emu.cpp", "jumprelu_emu", include=(CSRC,))


@pytest.fixture(scope="module")
def emu_asan(build_dir):
    return compile_emu(build_dir, "jumprelu_emu.cpp", "jumprelu_emu_asan", include=(CSRC,), asan=True)


def _hex(v) -> str:
    return f"{int(_bits(np.array([v], dtype=np.float32))[0]):08x}"


def _call(exe, d, *args):
    run_emu(exe, args, d, 900)


def _run_select(exe, d, idx, val, theta, eps, with_band=True):
    B, K = idx.shape
    H = theta.shape[0]
    idx.tofile(d / "idx.bin"), val.tofile(d / "val.bin"), theta.tofile(d / "theta.bin")
    _call(exe, d, "s", "idx.bin", "val.bin", B, K, "theta.bin", H, _hex(eps), _hex(U.half_eps(eps)), "band" if with_band else "noband",
          "idxsel.bin", "valsel.bin", "counts.bin", "idxband.bin", "countsband.bin", "l0.bin", "report.bin")
    return (np.fromfile(d / "idxsel.bin", np.int32).reshape(B, K), np.fromfile(d / "valsel.bin", np.float32).reshape(B, K),
            np.fromfile(d / "counts.bin", np.int32), np.fromfile(d / "idxband.bin", np.int32).reshape(B, K),
            np.fromfile(d / "countsband.bin", np.int32), np.fromfile(d / "l0.bin", np.float32)[0],
            np.fromfile(d / "report.bin", np.int64))


def _run_grad(exe, d, offsets, entries, gv, theta, g_l0, B, K, eps):
    H = theta.shape[0]
    offsets.tofile(d / "off.bin"), entries.tofile(d / "ent.bin"), theta.tofile(d / "theta.bin")
    if gv is not None:
        gv.tofile(d / "gv.bin")
    _call(exe, d, "g", "off.bin", "ent.bin", entries.shape[0], "gv.bin" if gv is not None else "-", "theta.bin",
          _hex(g_l0) if g_l0 is not None else "-", B, K, H, _hex(eps), "dtheta.bin")
    return np.fromfile(d / "dtheta.bin", np.float32)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), what


EMU_SHAPES = [(1, 1), (1, 256), (3, 5), (70, 64), (5, 65)]
NAMES = ("idx_sel", "val_sel", "counts", "idx_band", "counts_band", "l0", "report")


@pytest.mark.parametrize("asan", [False, True], ids=["plain", "asan"])
@pytest.mark.parametrize("H", [8, 300])
def test_kernel_source_on_the_host_equals_the_restatement(emu, emu_asan, build_dir, H, asan):
    exe, d = (emu_asan if asan else emu), build_dir
    for B, K in EMU_SHAPES:
        for kind in U.KINDS:
            idx, val, theta, eps = U.case(kind, B, K, H, seed=3)
            want = U.jump_select(idx, val, theta, eps)
            got = _run_select(exe, d, idx, val, theta, eps)
            for g, w, name in zip(got, want, NAMES):
                _same(g, w, f"{kind} {B}x{K} H={H}: {name}")
            if kind == "special":                            # without the band lists: the selection and the report are the same
                got = _run_select(exe, d, idx, val, theta, eps, with_band=False)
                for i in (0, 1, 2, 5, 6):
                    _same(got[i], want[i], f"{kind} {B}x{K} H={H}: {NAMES[i]} without band lists")
                assert (_bits(got[3]) == 0x5A5A5A5A).all() and (_bits(got[4]) == 0x5A5A5A5A).all()
            # the gradient over the band lists of this selection (the restated per-unit lists of tests/batch_topk_util.py)
            off, ent = BU.csr_ragged(want[3], want[4], H)
            rng = np.random.default_rng(B * K + H)
            gv = rng.standard_normal((B, K)).astype(np.float32)
            for use_gv, g_l0 in ((True, np.float32(0.375)), (True, None), (False, np.float32(-2.5))):
                dt = _run_grad(exe, d, off, ent, gv if use_gv else None, theta, g_l0, B, K, eps)
                _same(dt, U.threshold_grad(off, ent, gv if use_gv else None, theta, g_l0, B, eps),
                      f"{kind} {B}x{K} H={H}: dtheta gv={use_gv} g_l0={g_l0}")


def test_hand_cases_on_the_host(emu_asan, build_dir):
    eps = np.float32(0.5)
    theta = _f(1.0, 2.0, 0.5, NAN, INF, 0.0)
    idx = np.array([[0, 1, -1, 6, 2, 0, 3, 4, 5]], dtype=np.int32)
    val = _f(1.0, NAN, 9.0, 9.0, 0.75, 0.875, 7.0, INF, -0.0)[None]
    for g, w, name in zip(_run_select(emu_asan, build_dir, idx, val, theta, eps), U.jump_select(idx, val, theta, eps), NAMES):
        _same(g, w, name)
    offsets, entries = np.array([0, 0, 2, 3], dtype=np.int32), np.array([1, 4, 2, -1, -1, -1], dtype=np.int32)
    gv = _f(9, 0.5, -2.0, 9, 0.25, 9).reshape(3, 2)
    got = _run_grad(emu_asan, build_dir, offsets, entries, gv, _f(5.0, 2.0, 4.0), np.float32(3.0), 3, 2, np.float32(0.5))
    assert got.tolist() == [0.0, -7.0, 14.0] and not np.signbit(got[0])
