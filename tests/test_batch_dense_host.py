"""The dense BatchTopK encoder without a GPU: hand-worked batches of the numpy restatement (tests/batch_dense_util.py) against
the capped reference it must equal for every floor; the ledger of include/qsae_batch_dense.h -- every function declared there is
bound in _lib.BATCH_DENSE_SIGNATURES with as many arguments as it declares, exported by the product and the debug library as
qsaebd_*, and is either a *_bytes sizer or driven between guard words in tests/test_batch_dense_gpu.py; the calls of the C ABI
that return before they look at a pointer, in the order the header states; the refusals of the front ends, the models, the
controller and the Trainer; and the kernels' own source run on the CPU (tests/emu, tests/emu_util.py: threads as lanes, real
barriers, the fp32 MFMA as an fmaf chain), which must equal the restatement bit for bit, twice on poisoned outputs and a poisoned
workspace of exactly the sizer's bytes, also in a stand-alone build with AddressSanitizer where every operand is a heap block of
exactly its size.  The source lines that cannot compile for a host are rewritten as in tests/test_jump_dense_host.py."""
import re

import numpy as np
import pytest
import torch

import batch_dense_util as U
import test_batch_dense_gpu as G
from quantizedsae_amd import _lib, build, ops, torch_ops
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinaryLatentSAE, BinarySAE, TernarySparseAutoencoder
from quantizedsae_amd.training import BatchTopK, Trainer
from emu_util import CSRC, ROOT, compile_emu, rewrite, run_emu

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _f(*v):
    return np.array(v, dtype=np.float32)


def _bits(a):
    return U.bits(a)


# ---- the restatement, by hand -----------------------------------------------------------------------------------------
# Four rows of six pre-activations.  Rows 0 and 1 are equal (a tie across rows); units 0 and 1 are equal in every row (a tie
# across units); row 3 holds -0 in front of +0 and nothing above zero.  K = 3: the lists are
#   row 0, row 1:  5 (unit 3), 3 (unit 0), 3 (unit 1)       row 2:  2 (unit 2), 0.5 (unit 0), 0.5 (unit 1)
#   row 3:  -0 (unit 2), +0 (unit 3), +0 (unit 5)
HAND_Z = np.array([[3, 3, 1, 5, 0.75, 0], [3, 3, 1, 5, 0.75, 0], [0.5, 0.5, 2, 0, 0, 0], [-1, -1, -0.0, 0, -2, 0]], dtype=np.float32)
HAND_K = 3
HAND_FLOORS = (-INF, np.float32(-3.0), np.float32(0.0), np.float32(0.9), np.float32(1.0), np.float32(2.9), np.float32(3.0),
               np.float32(6.0), INF, NAN)


def _hand(n_select, floor, **kw):
    return U.encode_batch_topk_from_z(HAND_Z, HAND_K, n_select, floor, **kw)


def test_batches_by_hand():
    # three of the batch: both 5s, then the tie at 3 goes to row 0 and inside it to unit 0
    idx, val, counts, report, _ = _hand(3, np.float32(1.0))
    assert idx.tolist() == [[3, 0, -1], [3, -1, -1], [-1] * 3, [-1] * 3] and counts.tolist() == [2, 1, 0, 0]
    assert _bits(val).tolist() == _bits(np.array([[5, 3, 0], [5, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)).tolist()
    # floor 1.0: rows 0 and 1 hold exactly K candidates (5, 3, 3; the 1 is not above the floor), row 2 one, row 3 none
    assert report.tolist() == [3, 0, 2, U.f32_bits(3.0), 7, 0, 0, U.f32_bits(1.0)]
    # four: the tie across units inside row 0 before row 1 is looked at
    idx, _, counts, report, _ = _hand(4, np.float32(0.9))
    assert idx.tolist() == [[3, 0, 1], [3, -1, -1], [-1] * 3, [-1] * 3] and counts.tolist() == [3, 1, 0, 0]
    # floor 0.9: rows 0 and 1 hold K + 1 candidates (the 1 as well): capped at K, counted as rows over the cap
    assert report.tolist() == [4, 1, 2, U.f32_bits(3.0), 7, 0, 2, U.f32_bits(0.9)]
    # n_select of 0, 1 and B K
    idx, val, counts, report, state = _hand(0, NAN, floor_dev=True, theta=np.float32(0.5), batches=2, lr=np.float32(0.25))
    assert (idx == -1).all() and not _bits(val).any() and report.tolist() == [0, 0, 4, 0, 0, 0, 0, U.f32_bits(NAN)]
    assert state[0] == np.float32(0.5) and state[1] == 2 and np.isnan(state[2])        # nothing selected: nothing written
    idx, _, counts, report, _ = _hand(1, np.float32(0.0))
    assert idx.tolist()[0] == [3, -1, -1] and counts.tolist() == [1, 0, 0, 0] and report[:4].tolist() == [1, 0, 3, U.f32_bits(5.0)]
    idx, val, counts, report, state = _hand(12, np.float32(0.0), floor_dev=True, theta=np.float32(0.5), batches=2,
                                            lr=np.float32(0.25))
    # everything: row 3 has nothing above the floor, so the certificate fails (9 < 12) and the second attempt brings -0, +0, +0
    assert counts.tolist() == [3, 3, 3, 3] and idx.tolist()[3] == [2, 3, 5] and _bits(val[3]).tolist() == [0x80000000, 0, 0]
    assert report.tolist() == [12, 4, 0, 0, 9, 1, 2, 0]
    assert state[0] == np.float32(0.5) and state[1] == 2 and state[2] == 0               # m = +0: neither theta nor the floor moves
    # -0 against +0: one value, so of row 3's three zeros the first list position is taken, and m is -0
    idx, val, counts, report, state = _hand(10, -INF, floor_dev=True, theta=np.float32(0.5), batches=2, lr=np.float32(0.25))
    assert counts.tolist() == [3, 3, 3, 1] and idx.tolist()[3] == [2, -1, -1] and report[:4].tolist() == [10, 3, 0, 0x80000000]
    assert report[4:].tolist() == [12, 0, 4, U.f32_bits(-INF)] and state[0] == np.float32(0.5) and state[1] == 2 and state[2] == -INF
    # m > 0 moves the threshold and, with a floor on the device, writes fl32(floor_ratio * m)
    _, _, _, report, state = _hand(7, np.float32(0.25), floor_ratio=0.75, floor_dev=True, theta=np.float32(0.5), batches=2,
                                   lr=np.float32(0.25))
    assert report[:4].tolist() == [7, 2, 1, U.f32_bits(2.0)] and state == (np.float32(0.875), 3, np.float32(1.5))
    _, _, _, _, state = _hand(7, np.float32(0.25), floor_ratio=0.75, theta=np.float32(0.0), batches=0, lr=np.float32(0.25))
    assert state == (np.float32(2.0), 1, np.float32(0.25))                               # first update; a host floor stays
    # a floor above every value, at the boundary, NaN and +-inf: the certificate, and the same answer under every floor
    for n_select in (0, 1, 3, 4, 7, 9, 10, 12):
        ref = U.capped_reference_from_z(HAND_Z, HAND_K, n_select)
        for floor in HAND_FLOORS:
            idx, val, counts, report, _ = _hand(n_select, floor)
            what = (n_select, float(floor))
            assert np.array_equal(idx, ref[0]) and np.array_equal(_bits(val), _bits(ref[1])) and np.array_equal(counts, ref[2]), what
            assert report[:4].tolist() == ref[3].tolist(), what
            with np.errstate(invalid="ignore"):
                above = int(np.minimum((HAND_Z > floor).sum(axis=1), HAND_K).sum())
            assert report[4] == above and report[5] == int(above < n_select), what
    assert _hand(3, np.float32(3.0))[3][5] == 1 and _hand(3, np.float32(2.9))[3][5] == 0  # at floor == m the strict compare fails
    assert _hand(1, np.float32(6.0))[3][4:7].tolist() == [0, 1, 0] and _hand(1, NAN)[3][5] == 1 and _hand(1, INF)[3][5] == 1
    # on full lists the ragged selection is batch_topk_util's
    val = U.BT.select_values("eight_levels", 9, 7, seed=2)
    for n in (0, 1, 20, 63):
        got, want = U.select_ragged(val, np.full(9, 7), n), U.BT.batch_select(val, n)
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    # a NaN pre-activation is never a candidate: its row's list is the top-K of the others, short when fewer than K are left
    z = HAND_Z.copy()
    z[1, :] = NAN
    z[2, :4] = NAN
    idx, _, counts, report, _ = U.encode_batch_topk_from_z(z, HAND_K, 12, -INF)
    assert counts.tolist() == [3, 0, 2, 3] and idx.tolist()[2] == [4, 5, -1] and report.tolist()[:6] == [8, 2, 1, 0, 8, 1]
    assert len(U.REPORT_NAMES) == U.REPORT_WORDS == len(report)


def test_the_seeds_of_the_gpu_cases_reach_the_paths_they_exist_for():
    """What tests/test_batch_dense_gpu.py asserts next to the device: more than half the rows of the H = 1100 cases go through
    the resolve kernel under a floor of +0, and 2 m fails the certificate"""
    for B, D, H, K, with_bias in G.SHAPES:
        x, W, bias, n_select, floor, _, _ = G.case("too_high", B, D, H, K, with_bias)
        z = U.preact(x, W, bias)
        assert U.encode_batch_topk_from_z(z, K, n_select, floor)[3][5] == 1
        assert U.encode_batch_topk_from_z(z, K, n_select, G.case("certified", B, D, H, K, with_bias)[4])[3][5] == 0
        if H == 1100:
            assert U.rows_resolved(z, 0.0).mean() > 0.5
    for B, D, H, K, with_bias in G.FLOOR_SHAPES:
        z = U.preact(*U.operands(B, D, H, 17, with_bias))
        m = U.smallest_selected(z, K, B * G.k_of(K))
        assert m > 0 and (H != 1100 or U.rows_resolved(z, 0.0).mean() > 0.5)
        for factor, second in ((0.9, 0), (1.0, 1), (2.0, 1)):
            assert U.encode_batch_topk_from_z(z, K, B * G.k_of(K), np.float32(factor) * m)[3][5] == second


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_batch_dense.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_batch_dense.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 2 and sorted(declared) == sorted(_lib.BATCH_DENSE_SIGNATURES)
    assert all(n.startswith("qsaebd_") for n in declared)
    others = (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.CURVE_SIGNATURES, _lib.NESTED_SIGNATURES, _lib.BATCH_SIGNATURES,
              _lib.NESTED_BATCH_SIGNATURES, _lib.MULTIK_SIGNATURES, _lib.JUMP_SIGNATURES, _lib.JUMP_DENSE_SIGNATURES)
    assert not any(set(declared) & set(t) for t in others)
    assert not any(n.startswith("qsaebd_") for t in others for n in t)
    for name, n_params in declared.items():
        assert len(_lib.BATCH_DENSE_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaebd_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    sizers = {n for n in declared if n.endswith("_bytes")}
    guarded = {entry for entry, *_ in G.GUARD_CASES.values()}
    assert sizers | guarded == set(declared) and not sizers & guarded
    assert all(n[:-len("_workspace_bytes")] in guarded for n in sizers)      # every sizer belongs to a guarded call
    assert "batch_dense.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in (ROOT / "include" / "qsae_batch_dense.h").read_text()
    assert "qsae_batch_dense.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()
    assert ops.BATCH_DENSE_MAX_K == torch_ops.BATCH_DENSE_MAX_K == 256 and ops.BATCH_DENSE_REPORT_WORDS == U.REPORT_WORDS
    assert BatchTopK.REPORT_NAMES_DENSE == U.REPORT_NAMES and hasattr(torch.ops.qsae, "encode_batch_topk")


# ---- calls that need no device ----------------------------------------------------------------------------------------
def test_calls_that_return_before_they_look_at_a_pointer():
    lib = _lib.load()

    def call(B, D, H, K, n_select=0, ratio=0.9, ldx=None, ldw=None):
        return lib.qsaebd_encode_batch_topk(None, D if ldx is None else ldx, None, D if ldw is None else ldw, None, B, D, H, K,
                                            n_select, None, 0.0, ratio, None, None, None, None, None, None, 0.0, None, 0, None)

    # sizes that make no sense come first (invalid), then the ratio, then what the kernels do not take (unsupported), then n_select
    assert call(-1, 8, 64, 8) == _lib.ERR_INVALID_ARG and b"qsaebd_encode_batch_topk" in lib.qsae_last_error()
    assert call(5, 8, 64, 0) == _lib.ERR_INVALID_ARG and call(5, 8, 0, 8) == _lib.ERR_INVALID_ARG
    assert call(-1, 8, 64, 257) == _lib.ERR_INVALID_ARG and call(-1, 6, 64, 8) == _lib.ERR_INVALID_ARG
    for ratio in (0.0, -1.0, 1.5, float("inf"), float("nan")):
        assert call(5, 8, 64, 8, ratio=ratio) == _lib.ERR_INVALID_ARG and b"floor_ratio" in lib.qsae_last_error()
        assert call(5, 6, 64, 257, ratio=ratio) == _lib.ERR_INVALID_ARG                     # ... before anything unsupported
    assert call(5, 8, 512, 257) == _lib.ERR_UNSUPPORTED and b"K <= 256" in lib.qsae_last_error()
    assert call(5, 8, 64, 65) == _lib.ERR_UNSUPPORTED and b"K <= H" in lib.qsae_last_error()
    assert call(5, 6, 512, 257) == _lib.ERR_UNSUPPORTED and b"K <= 256" in lib.qsae_last_error()     # K before D
    for D in (6, 0, -4):
        assert call(5, D, 64, 8) == _lib.ERR_UNSUPPORTED and b"multiple of 4" in lib.qsae_last_error()
    assert call(1 << 23, 8, 512, 256) == _lib.ERR_UNSUPPORTED and b"B * K" in lib.qsae_last_error()
    assert call(1 << 23, 6, 512, 256) == _lib.ERR_UNSUPPORTED and b"multiple of 4" in lib.qsae_last_error()   # D before B * K
    for n_select in (-1, 41):
        assert call(5, 8, 64, 8, n_select) == _lib.ERR_INVALID_ARG and b"n_select" in lib.qsae_last_error()
        assert call(5, 6, 64, 8, n_select) == _lib.ERR_UNSUPPORTED                          # ... behind what is unsupported
    assert call(0, 8, 64, 8, 1) == _lib.ERR_INVALID_ARG and b"n_select" in lib.qsae_last_error()
    assert call(0, 8, 64, 8) == _lib.OK                                                      # B == 0: nothing launched
    assert call(0, 6, 64, 8) == _lib.ERR_UNSUPPORTED                                         # ... but only for a shape it takes
    # then the strides and the pointers, before any launch
    assert call(5, 8, 64, 8, 40, ldx=4) == _lib.ERR_INVALID_ARG and b"stride" in lib.qsae_last_error()
    assert call(5, 8, 64, 8, ldw=10) == _lib.ERR_INVALID_ARG and b"stride" in lib.qsae_last_error()
    assert call(5, 8, 64, 8) == _lib.ERR_INVALID_ARG and b"null" in lib.qsae_last_error()
    size = lib.qsaebd_encode_batch_topk_workspace_bytes
    assert size(7, 8, 512, 6) > 0 and size(0, 8, 512, 6) > 0 and size(8192, 512, 32768, 256) >= size(8191, 512, 32768, 256)
    for refused in ((7, 8, 512, 257), (7, 8, 4, 6), (7, 6, 512, 6), (7, 0, 512, 6), (-1, 8, 512, 6), (7, 8, 0, 6), (7, 8, 512, 0),
                    (1 << 23, 8, 512, 256)):
        assert size(*refused) == 0, refused


def test_front_ends_models_controller_and_trainer_refuse(tmp_path):
    x, W, b = torch.zeros(2, 4), torch.zeros(8, 4), torch.zeros(8)
    for mod in (ops, torch_ops):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod.encode_batch_topk(x, W, b, 2, 2, 0.25)
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        ctl = BatchTopK(model, k=2, dense=True)
        assert ctl.dense and ctl.floor_ratio == BatchTopK.DEFAULT_FLOOR_RATIO and not ctl.floor_seeded and bool(torch.isnan(ctl.floor))
        for call in (lambda: model.forward_batch_topk_dense(x, ctl), lambda: model.forward_train_batch_topk_dense(x, ctl),
                     lambda: model.forward_nested_batch_topk_dense(x, ctl, [4, 8]),
                     lambda: model.forward_train_nested_batch_topk_dense(x, ctl, [4, 8])):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
        capped = BatchTopK(model, k=2)
        assert not capped.dense and "dense_floor" not in capped.state_dict() and "dense_floor" in ctl.state_dict()
        ctl.load_state_dict(capped.state_dict())             # a state saved without the floor loads; the floor stays unseeded
        assert not ctl.floor_seeded
        ctl.floor.fill_(0.5)
        ctl.floor_seeded = True
        other = BatchTopK(model, k=2, dense=True)
        other.load_state_dict(ctl.state_dict())
        assert other.floor_seeded and float(other.floor) == 0.5
        capped.load_state_dict(ctl.state_dict())             # ... and a capped controller ignores a saved floor
        with pytest.raises(ValueError, match="floor_ratio needs dense=True"):
            BatchTopK(model, k=2, floor_ratio=0.5)
        for ratio in (0.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match="floor_ratio"):
                BatchTopK(model, k=2, dense=True, floor_ratio=ratio)
        # the eight words are recorded next to the four every consumer reads
        ctl.record(torch.zeros(4, dtype=torch.int32), torch.tensor([5, 0, 1, 0x3F000000, 40, 1, 2, 0x3E800000]))
        assert ctl.report.tolist() == [5, 0, 1, 0x3F000000] and ctl.summary()["selected"] == 5
        assert ctl.dense_summary() == {"candidates": 40, "candidates_per_row": 10.0, "second_attempt": 1, "rows_over_cap": 2,
                                       "second_attempts": 1, "dense_selections": 1}
    for other in (TernarySparseAutoencoder(4, 8), BinaryLatentSAE(4, 8)):
        assert not hasattr(other, "forward_batch_topk_dense") and not hasattr(other, "forward_train_nested_batch_topk_dense")
    config = {"input_dim": 4, "n_bits": 4, "hidden_dim": 32, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 2,
              "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 8}

    def trainer(**kw):
        return Trainer(config, "baseline_sae", False, True, model=BaselineSparseAutoencoder(4, 32), dataset_dir=str(tmp_path),
                       save_dir=str(tmp_path), **kw)
    with pytest.raises(ValueError, match="batch_topk_dense needs batch_topk=True"):
        trainer(batch_topk_dense=True)
    with pytest.raises(ValueError, match="batch_topk_floor_ratio needs batch_topk_dense=True"):
        trainer(batch_topk=True, batch_topk_floor_ratio=0.9)
    t = trainer(batch_topk=True, batch_topk_dense=True, batch_topk_floor_ratio=0.95)
    assert t.batch_topk_dense is True and t.batch_topk.dense and t.batch_topk.floor_ratio == 0.95
    assert trainer(batch_topk=True, batch_topk_dense=True, batch_topk_nested_bounds="default").nested_bounds is not None
    assert trainer(batch_topk=True).batch_topk_dense is False and not trainer(batch_topk=True).batch_topk.dense   # default: capped
    assert trainer().batch_topk_dense is False and trainer().batch_topk is None


# ---- the kernels' own source on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_dense_emu")
    gemm = (CSRC / "gemm_mfma_f32.h").read_text()
    gemm = rewrite(gemm, 'asm volatile("s_nop 4\\n\\tglobal_load_dwordx4 %0, %1, %2" : "=v"(r[P][i]) : "v"(voff[i]), "s"(base) : "memory");',
                   "r[P][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + voff[i]);")
    gemm = rewrite(gemm, "extern __shared__ __attribute__((aligned(16))) float smem[];", "float* smem = reinterpret_cast<float*>(g_lds);")
    gemm, n = re.subn(r'asm volatile\("s_waitcnt vmcnt\((?:%0|0)\)" ::[^;]*;', ";", gemm)
    assert n == 5
    assert gemm.count('"+v"') == 3
    gemm = gemm.replace('"+v"', '"+x"')
    gemm = rewrite(gemm, '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    src = rewrite((CSRC / "batch_dense.hip").read_text(), '#include "../../include/qsae_batch_dense.h"',
                  f'#include "{ROOT / "include" / "qsae_batch_dense.h"}"')
    (d / "gemm_mfma_f32.h").write_text(gemm)
    (d / "batch_dense_emu.hip").write_text(src)
    return d


@pytest.fixture(scope="module")
def emu(build_dir):
    return compile_emu(build_dir, "batch_dense_emu.cpp", "batch_dense_emu", include=(build_dir,))


@pytest.fixture(scope="module")
def emu_asan(build_dir):
    return compile_emu(build_dir, "batch_dense_emu.cpp", "batch_dense_emu_asan", include=(build_dir,), asan=True)


def _hex(v) -> str:
    return f"{U.f32_bits(v):08x}"


def _run(exe, d, x, W, bias, K, n_select, floor, floor_dev=False, ratio=1.0, theta=None, batches=0, lr=0.0, shift=0, pad_x=0,
         pad_w=0):
    B, D = x.shape
    H = W.shape[0]

    def dump(a, pad, name):
        w = np.full((a.shape[0], D + pad), np.nan, np.float32)      # NaN between D and the row stride
        w[:, :D] = a
        w.tofile(d / name)
    dump(x, pad_x, "x.bin"), dump(W, pad_w, "w.bin")
    if bias is not None:
        np.ascontiguousarray(bias, np.float32).tofile(d / "bias.bin")
    run_emu(exe, ["x.bin", B, D + pad_x, "w.bin", H, D + pad_w, "-" if bias is None else "bias.bin", D, K, n_select, _hex(floor),
                  "device" if floor_dev else "host", _hex(ratio), "-" if theta is None else _hex(theta), batches, _hex(lr), shift,
                  "idxsel.bin", "valsel.bin", "counts.bin", "report.bin", "state.bin"], d, 900)
    state = np.fromfile(d / "state.bin", np.uint8)
    return (np.fromfile(d / "idxsel.bin", np.int32).reshape(B, K), np.fromfile(d / "valsel.bin", np.float32).reshape(B, K),
            np.fromfile(d / "counts.bin", np.int32), np.fromfile(d / "report.bin", np.int64),
            (state[:4].view(np.float32)[0], int(state[8:].view(np.int64)[0]), state[4:8].view(np.float32)[0]))


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), what


def _check(got, want, floor_dev, with_state, what):
    for g, w, name in zip(got[:4], want[:4], U.NAMES):
        _same(g, w, f"{what}: {name}")
    if with_state:
        _same(np.float32(got[4][0]), np.float32(want[4][0]), f"{what}: theta")
        assert got[4][1] == want[4][1], what
    if floor_dev:
        _same(np.float32(got[4][2]), np.float32(want[4][2]), f"{what}: the floor word")


#: (B, D, H, K): one tile; a K tail with three splits of the units and, under a floor of +0, regions that overflow; a panel tail
#: at 128 rows; more tiles than splits and rows of more than 512 candidates; the widest list
EMU_SHAPES = [(3, 4, 8, 1), (3, 36, 300, 5), (5, 36, 300, 64), (130, 4, 8, 5), (2, 64, 1100, 65), (3, 8, 600, 256)]
#: every shape plain; under the sanitizer all but the panel tail (its 130 rows differ from the others in the row count alone)
EMU_RUNS = [(s, False) for s in EMU_SHAPES] + [(s, True) for s in EMU_SHAPES if s[0] <= 128]


@pytest.mark.parametrize("shape,asan", EMU_RUNS, ids=lambda v: ("asan" if v else "plain") if isinstance(v, bool) else "x".join(map(str, v)))
def test_kernel_source_on_the_host_equals_the_restatement(emu, emu_asan, build_dir, shape, asan):
    exe, d = (emu_asan if asan else emu), build_dir
    B, D, H, K = shape
    for kind in G.KINDS:
        x, W, bias, n_select, floor, floor_dev, with_state = G.case(kind, B, D, H, K, kind != "zero")
        theta, batches, lr = G.STATE if with_state else (None, 0, 0.0)
        z = U.preact(x, W, bias)
        want = U.encode_batch_topk_from_z(z, K, n_select, floor, floor_ratio=0.75, floor_dev=floor_dev, theta=theta, batches=batches,
                                          lr=lr)
        if kind == "zero" and H in (300, 1100):
            assert U.rows_resolved(z, floor).mean() > 0.5      # the rows that the regions cannot hold: the resolve kernel ran
        if kind in ("certified", "too_high"):
            assert want[3][5] == (kind == "too_high")
        got = _run(exe, d, x, W, bias, K, n_select, floor, floor_dev, 0.75, theta, batches, lr, shift=4 if kind == "special" else 0,
                   pad_x=4 if kind == "zero" else 0, pad_w=8 if kind == "zero" else 0)
        _check(got, want, floor_dev, with_state, f"{kind} {shape}")
        if kind != "special":                                  # (no NaN): what the header promises for every floor
            ref = U.capped_reference_from_z(z, K, n_select)
            for g, w, name in zip(got[:3], ref[:3], U.NAMES):
                _same(g, w, f"{kind} {shape}: {name} against the capped reference")
            assert got[3][:4].tolist() == ref[3].tolist()


def test_hand_batches_on_the_host(emu_asan, build_dir):
    """HAND_Z as pre-activations: x = the rows, W = the identity (D = H = 8, the last two units and columns zero)"""
    x = np.zeros((4, 8), np.float32)
    x[:, :6] = HAND_Z
    W = np.eye(8, dtype=np.float32)
    z = U.preact(x, W, None)
    assert np.array_equal(z[:, :6], HAND_Z)                    # (as values: the chain turns the -0 into +0)
    for n_select, floor in ((3, 1.0), (4, 0.9), (0, NAN), (12, 0.0), (10, -INF), (3, 3.0), (1, 6.0), (7, NAN)):
        want = U.encode_batch_topk_from_z(z, HAND_K, n_select, floor, floor_ratio=0.75, floor_dev=True, theta=np.float32(0.5), batches=2,
                                          lr=np.float32(0.25))
        got = _run(emu_asan, build_dir, x, W, None, HAND_K, n_select, floor, True, 0.75, np.float32(0.5), 2, np.float32(0.25))
        _check(got, want, True, True, f"n_select {n_select} floor {floor}")
