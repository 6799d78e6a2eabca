"""BinaryLatentSAE training without a GPU: the C-ABI surface, the refused shapes (every refusal answers before any HIP call),
the errors of forward_train on a host model, and the fp64 restatement of train_blatent_util pinned to the reference's
fixtures on the CPU."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantizedsae_amd import _lib, torch_ops
from quantizedsae_amd.sae import BinaryLatentSAE

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_blatent_util as U  # noqa: E402
from golden_util import NEAR_TIE_EPS  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-5

NEW_SYMBOLS = ["qsae_blatent_binarize", "qsae_train_blatent_dpre", "qsae_train_blatent_dweight"]


def test_new_symbols_declared_exported_and_bound():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    from quantizedsae_amd.build import DEBUG_LIB
    declared = ge.declared_symbols()
    lib, dbg = ctypes.CDLL(str(_lib.LIB_PATH)), ctypes.CDLL(str(DEBUG_LIB))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(lib, name) and hasattr(dbg, name), name
    assert _lib.load().qsae_abi_version() == _lib.ABI_VERSION == 4
    for name in ("train_blatent_supported", "blatent_binarize", "train_blatent_dpre", "train_blatent_dweight"):
        assert callable(getattr(torch_ops, name))
    assert hasattr(BinaryLatentSAE, "forward_train")


def test_refused_shapes_answer_without_a_device():
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    odd = ctypes.c_void_p(20)
    cut = U.CUTOFF
    UNS, INV = _lib.ERR_UNSUPPORTED, _lib.ERR_INVALID_ARG
    # binarize(pre, B, H, cutoff, latent, zbits, stream)
    assert lib.qsae_blatent_binarize(p, 8, 100, cut, p, p, None) == UNS               # H % 32
    assert lib.qsae_blatent_binarize(p, 0, 256, cut, p, p, None) == INV               # B < 1
    assert lib.qsae_blatent_binarize(p, 65536, 32768, cut, p, p, None) == UNS         # B * H = 2^31
    assert lib.qsae_blatent_binarize(None, 8, 256, cut, p, p, None) == INV
    assert lib.qsae_blatent_binarize(p, 8, 256, cut, p, None, None) == INV
    assert lib.qsae_blatent_binarize(odd, 8, 256, cut, p, p, None) == INV             # alignment
    # dpre(g_recon, w_dec, B, D, H, pre, stream)
    assert lib.qsae_train_blatent_dpre(p, p, 8, 66, 256, p, None) == UNS              # D % 4
    assert lib.qsae_train_blatent_dpre(p, p, 8, 4100, 256, p, None) == UNS            # D > 4096
    assert lib.qsae_train_blatent_dpre(p, p, 8, 64, 100, p, None) == UNS              # H % 32
    assert lib.qsae_train_blatent_dpre(p, p, 0, 64, 256, p, None) == INV              # B < 1
    assert lib.qsae_train_blatent_dpre(p, p, 65536, 64, 32768, p, None) == UNS        # B * H = 2^31
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.qsae_train_blatent_dpre(args[0], args[1], 8, 64, 256, args[2], None) == INV
    assert lib.qsae_train_blatent_dpre(odd, p, 8, 64, 256, p, None) == INV
    # dweight(g_recon, zbits, words_ld, B, D, H, dweight, stream)
    assert lib.qsae_train_blatent_dweight(p, p, 8, 8, 66, 256, p, None) == UNS
    assert lib.qsae_train_blatent_dweight(p, p, 8, 8, 4100, 256, p, None) == UNS
    assert lib.qsae_train_blatent_dweight(p, p, 4, 8, 64, 100, p, None) == UNS
    assert lib.qsae_train_blatent_dweight(p, p, 8, 0, 64, 256, p, None) == INV
    assert lib.qsae_train_blatent_dweight(p, p, 1024, 65536, 64, 32768, p, None) == UNS
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.qsae_train_blatent_dweight(args[0], args[1], 8, 8, 64, 256, args[2], None) == INV
    assert lib.qsae_train_blatent_dweight(p, p, 7, 8, 64, 256, p, None) == INV        # words_ld < H / 32
    assert torch_ops.train_blatent_supported(4096, 32) and torch_ops.train_blatent_supported(4, 32768)
    assert not torch_ops.train_blatent_supported(4100, 256) and not torch_ops.train_blatent_supported(66, 256)
    assert not torch_ops.train_blatent_supported(64, 100) and not torch_ops.train_blatent_supported(0, 256)


def test_forward_train_refuses_on_the_host():
    m = BinaryLatentSAE(64, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_train(torch.zeros(2, 64))
    assert sorted(m.state_dict()) == ["decoder.bias", "decoder.weight", "encoder.0.bias", "encoder.0.weight"]


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_fp64_table_matches_reference_fixtures(name):
    """The util is what the GPU tests are measured against: here it is held to the reference's own autograd on the CPU (fp32
    reference against the fp64 table; 1e-5 asserted, the figures are printed).  No element is excluded: the generator kept
    every pre-activation NEAR_TIE_EPS away from the cutoff."""
    meta, fx = U.load_fixture(name)
    D, H, B = meta["D"], meta["H"], meta["B"]
    assert (D, H, B) == tuple(U.CASES[name][k] for k in ("D", "H", "B"))
    sd, x_np = U.case_inputs(meta, meta["seed"])
    assert np.array_equal(x_np, fx["x"])
    assert meta["excluded"] == 0 and float(fx["min_cutoff_distance"]) >= NEAR_TIE_EPS
    W_e, b_e, W_d, b_d = (sd[k] for k in U.PARAM_KEYS)
    z = U.unpack_latent(fx["binary_latent"], H)
    pre64 = torch.from_numpy(x_np).double() @ torch.from_numpy(W_e).double().t() + torch.from_numpy(b_e).double()
    assert float((pre64 - U.CUTOFF).abs().min()) >= 0.9 * NEAR_TIE_EPS
    assert np.array_equal((pre64 >= U.CUTOFF).numpy(), z != 0)                      # every bit, nothing left out
    recon = U.forward64(z, W_d, b_d)
    err = U.max_rel_err(recon, fx["recon"])
    print(f"{name} recon: {err:.3g}")
    assert err <= TOL
    loss = float(((recon - torch.from_numpy(x_np).double()) ** 2).mean())
    assert abs(loss - float(fx["loss"])) <= TOL * abs(float(fx["loss"]))
    g = U.grads64(x_np, W_e, b_e, W_d, z, U.trainer_incoming(x_np, recon, B, D))
    for key in U.PARAM_KEYS + ("x",):
        err = U.max_rel_err(g[key], fx["grad." + key])
        print(f"{name} {key}: {err:.3g}")
        assert err <= TOL, f"{name} {key}: {err:.3g}"


def test_loop_fixture_is_consistent():
    meta, fx = U.load_fixture(U.LOOP_FIXTURE)
    l32, l64 = fx["loss32"], fx["loss64"]
    assert len(l32) == len(l64) == meta["steps"] and 2 <= meta["steps"] <= 20
    assert (meta["D"], meta["H"], meta["B"], meta["lr"]) == (64, 1024, 256, 1e-3)
    gap = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
    assert gap == pytest.approx(meta["gap"]) and gap <= 1e-2 and meta["bound"] == pytest.approx(max(10 * gap, 1e-5))
    assert l32[-1] < l32[0] and l64[-1] < l64[0]
    assert meta["same_bits_fp32_fp64"] is True and meta["band_margin"] > 0
