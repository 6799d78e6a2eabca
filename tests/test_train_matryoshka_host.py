"""QuantizedMatryoshkaSAE training without a GPU: the C-ABI surface, the refused shapes, the ValueErrors of forward_train,
and the fp64 restatement (train_matryoshka_util) pinned to the reference's fixtures on the CPU."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantizedsae_amd import QuantizedMatryoshkaSAE, ResidualQuantizedSAE, _lib, torch_ops
from quantizedsae_amd.sae.quantized_matryoshka import nested_sizes

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_matryoshka_util as U  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-5

NEW_SYMBOLS = ["qsae_transpose_rows", "qsae_train_pre_bits", "qsae_train_matryoshka_sign_rows", "qsae_train_matryoshka_dpre", "qsae_train_gemm_tn",
               "qsae_train_matryoshka_dsum_dense", "qsae_train_bits_csr_workspace_bytes", "qsae_train_bits_csr",
               "qsae_train_matryoshka_dsum_lists_workspace_bytes", "qsae_train_matryoshka_dsum_lists",
               "qsae_train_matryoshka_finish", "qsae_train_matryoshka_secant"]


def test_new_symbols_declared_exported_and_bound():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.load().qsae_abi_version() == _lib.ABI_VERSION == 4
    for name in ("train_matryoshka_dpre", "train_gemm_tn", "train_matryoshka_dsum_dense", "train_bits_csr",
                 "train_matryoshka_dsum_lists", "train_matryoshka_finish", "train_matryoshka_secant", "transpose_rows"):
        assert callable(getattr(torch_ops, name))


def test_workspace_sizes_and_refused_shapes():
    lib = _lib.load()
    assert lib.qsae_train_bits_csr_workspace_bytes(8192, 32768) > 2 * 32768 * 256 * 4
    for B, H in [(0, 1024), (24, 1000), (24, 0), (65536, 32768)]:          # no row, H % 32, no unit, B * H = 2^31
        assert lib.qsae_train_bits_csr_workspace_bytes(B, H) == 0
    assert lib.qsae_train_matryoshka_dsum_lists_workspace_bytes(8192, 1 << 20, 32768, 512) > 0
    for B, n, H, D in [(0, 10, 256, 64), (24, -1, 256, 64), (24, 1 << 31, 256, 64), (24, 10, 0, 64), (24, 10, 256, 66),
                       (24, 10, 256, 4100)]:
        assert lib.qsae_train_matryoshka_dsum_lists_workspace_bytes(B, n, H, D) == 0
    # argument validation happens before any HIP call
    p = ctypes.c_void_p(16)
    sizes = (ctypes.c_int32 * 4)(32, 32, 64, 128)
    sp = ctypes.cast(sizes, ctypes.c_void_p)
    assert lib.qsae_train_matryoshka_dpre(p, p, p, p, 8, 66, 256, 4, sp, p, 256, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_matryoshka_dpre(p, p, p, p, 8, 4100, 256, 4, sp, p, 256, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_matryoshka_dpre(p, p, p, p, 0, 64, 256, 4, sp, p, 256, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_matryoshka_dpre(p, p, p, p, 8, 64, 512, 4, sp, p, 512, None) == _lib.ERR_INVALID_ARG   # sizes != H
    odd = (ctypes.c_int32 * 4)(31, 33, 64, 128)
    assert lib.qsae_train_matryoshka_dpre(p, p, p, p, 8, 64, 256, 4, ctypes.cast(odd, ctypes.c_void_p), p, 256,
                                          None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_pre_bits(p, 1000, 8, 1000, p, 32, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_pre_bits(None, 256, 0, 256, None, 8, None) == 0                       # no row: nothing to do
    assert lib.qsae_train_gemm_tn(p, 256, p, 64, 8, 250, 64, p, 64, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_gemm_tn(p, 256, p, 64, 0, 256, 64, p, 64, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_matryoshka_dsum_dense(p, 8, p, 8, 4100, 256, 4, sp, p, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_bits_csr(p, 1024, 65536, 32768, p, p, 0, p, 1 << 40, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_matryoshka_finish(p, p, None, p, p, 256, 66, p, p, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_matryoshka_secant(p, 1.0, p, None, p, p, 256, 66, p, p, None) == _lib.ERR_UNSUPPORTED
    assert torch_ops.train_matryoshka_supported(4096) and not torch_ops.train_matryoshka_supported(4100)
    assert not torch_ops.train_matryoshka_supported(66) and not torch_ops.train_matryoshka_supported(0)
    assert torch_ops.train_bits_csr_supported(8192, 32768) and not torch_ops.train_bits_csr_supported(65536, 32768)


def test_forward_train_refuses_before_any_launch():
    m = QuantizedMatryoshkaSAE(64, 256, 32, n_bits=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_train(torch.zeros(2, 64))
    with pytest.raises(RuntimeError, match="forward_train"):
        m.decoder.apply_secant_grad()
    with pytest.raises(RuntimeError):
        ResidualQuantizedSAE(64, 256, 32, n_bits=4).forward_train(torch.zeros(2, 64))
    # the limits are refused before the device is asked for anything, naming the limit
    with pytest.raises(ValueError, match="multiple of 4 up to 4096"):
        QuantizedMatryoshkaSAE(66, 256, 32, n_bits=4).forward_train(torch.zeros(2, 66))
    with pytest.raises(ValueError, match="multiple of 4 up to 4096"):
        QuantizedMatryoshkaSAE(4100, 64, 32, n_bits=2).forward_train(torch.zeros(2, 4100))
    with pytest.raises(ValueError, match=r"expected \[batch, 64\]"):
        m.forward_train(torch.zeros(2, 32))
    m.decoder_grad_path = "csr"
    with pytest.raises(ValueError, match="decoder_grad_path"):
        m.forward_train(torch.zeros(2, 64))


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_fp64_restatement_matches_reference_fixtures(name):
    """The util is what the full-size GPU tests are measured against: here it is held to the reference's own autograd and
    apply_secant_grad() on the CPU (fp32 reference against fp64 table: <= 9e-7 measured, 1e-5 asserted)."""
    meta, z = U.load_fixture(name)
    sd, x_np = U.case_inputs(meta, meta["seed"])
    assert z["min_abs_pre"] >= meta["min_abs_pre"]
    D, H, n, B, lam = meta["D"], meta["H"], meta["n_bits"], meta["B"], meta["lam"]
    if meta["kind"] == "q":
        stages = [("", H, n, meta["allow_bias"], lam)]
    else:
        stages = [(f"saes.{i}.", h, 1, i == 0, lam * U.RQ_STAGE_WEIGHTS[i]) for i, h in enumerate(nested_sizes(H, n))]
    residual = torch.from_numpy(x_np).double()
    loss = 0.0
    for i, (pre, h, nb, allow_bias, lam_i) in enumerate(stages):
        zb = torch.from_numpy(np.unpackbits(z[f"z.{i}"], axis=1, bitorder="little")[:, :h].astype(bool))
        P = {k: sd[pre + k] for k in U.PARAM_KEYS}
        groups, levels = U.forward64(zb, P["decoder.weight"], P["decoder.weight_mirror"], P["decoder.bias"], nb, allow_bias)
        if meta["kind"] == "q":
            assert U.max_rel_err(levels, z["levels"]) <= TOL and U.max_rel_err(groups, z["groups"]) <= TOL
        else:
            assert U.max_rel_err(levels[0], z["levels"][i]) <= TOL
        loss += U.trainer_loss64(residual, levels, groups, lam_i)
        G, gg = U.trainer_incoming(residual, levels, nb, lam_i)
        g = U.grads64(residual, P["encoder.0.weight"], P["encoder.0.bias"], P["decoder.weight"], P["decoder.weight_mirror"],
                      zb, G, gg, nb, allow_bias)
        for key in U.PARAM_KEYS:
            want = z["grad." + pre + key]
            if key == "decoder.bias" and not allow_bias:
                assert g[key] is None and want.size == 0                    # no gradient, as in the reference
                continue
            err = U.max_rel_err(g[key], want)
            assert err <= TOL, f"{name} {pre}{key}: {err:.3g}"
        for key in ("decoder.weight", "decoder.weight_mirror"):
            err = U.max_rel_err(g["secant." + key], z["secant." + pre + key])
            assert err <= TOL, f"{name} secant {pre}{key}: {err:.3g}"
        residual = (residual - levels[-1]) * 2
    assert abs(loss - float(z["loss"])) <= TOL * abs(float(z["loss"]))


def test_loop_fixture_is_consistent():
    meta, z = U.load_fixture(U.LOOP_FIXTURE)
    assert set(meta["cases"]) == set(U.LOOP_CASES)
    for name, c in meta["cases"].items():
        l32, l64 = z[f"{name}.loss32"], z[f"{name}.loss64"]
        assert len(l32) == len(l64) == meta["steps"] == 30
        gap = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
        assert gap == pytest.approx(c["gap"]) and c["bound"] == pytest.approx(max(10 * gap, 1e-5))
        assert l32[-1] < l32[0]
