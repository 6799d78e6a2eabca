"""TernarySparseAutoencoder training without a GPU: the C-ABI surface, the refused shapes, the errors of forward_train and of
the mask methods on a host model, and the restatements of train_ternary_util (the gradient table in fp64, the mask rules as
exact integer logic) pinned to the reference's fixtures on the CPU."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantizedsae_amd import TernarySparseAutoencoder, _lib, torch_ops

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_ternary_util as U  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-5

NEW_SYMBOLS = ["qsae_train_ternary_rows", "qsae_train_ternary_dpre", "qsae_train_ternary_dweight",
               "qsae_train_mask_workspace_bytes", "qsae_train_mask_init", "qsae_train_mask_update"]


def test_new_symbols_declared_exported_and_bound():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.load().qsae_abi_version() == _lib.ABI_VERSION == 4
    for name in ("train_ternary_rows", "train_ternary_dpre", "train_ternary_dweight", "train_mask_init", "train_mask_update"):
        assert callable(getattr(torch_ops, name))


def test_workspace_sizes_and_refused_shapes():
    lib = _lib.load()
    assert 0 < lib.qsae_train_mask_workspace_bytes(512, 32768) < (1 << 20)        # histograms and counters only
    for D, H in [(0, 256), (64, 0), (65536, 32768), (3, 5)]:                       # nothing, 2^31 elements, not a multiple of 4
        assert lib.qsae_train_mask_workspace_bytes(D, H) == 0
    # argument validation happens before any HIP call
    p = ctypes.c_void_p(16)
    big = 1 << 20
    assert lib.qsae_train_mask_init(p, p, 65536, 32768, 10, p, big, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_mask_init(p, p, 3, 5, 1, p, big, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_mask_init(p, p, 64, 256, -1, p, big, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_mask_init(p, p, 64, 256, 64 * 256 + 1, p, big, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_mask_init(p, ctypes.c_void_p(20), 64, 256, 1, p, big, None) == _lib.ERR_INVALID_ARG   # alignment
    assert lib.qsae_train_mask_init(p, p, 64, 256, 1, p, 16, None) == _lib.ERR_WORKSPACE
    assert lib.qsae_train_mask_update(p, p, p, p, 65536, 32768, 10, p, big, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_mask_update(p, p, p, p, 64, 256, 64 * 256 + 1, p, big, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_mask_update(p, p, p, None, 64, 256, 10, p, big, None) == _lib.ERR_INVALID_ARG          # a without delta
    assert lib.qsae_train_mask_update(None, p, p, p, 64, 256, 10, p, big, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_ternary_rows(p, 64, 1002, p, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_ternary_rows(None, 64, 256, p, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_ternary_dpre(p, p, p, p, 8, 66, 256, p, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_ternary_dpre(p, p, p, p, 8, 4100, 256, p, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_ternary_dpre(p, p, p, p, 0, 64, 256, p, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_ternary_dpre(p, None, p, p, 8, 64, 256, p, None) == _lib.ERR_INVALID_ARG              # G without T
    assert lib.qsae_train_ternary_dweight(p, p, p, 8, 66, 256, p, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_ternary_dweight(p, p, p, 8, 64, 1002, p, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_ternary_dweight(p, p, None, 8, 64, 256, p, None) == _lib.ERR_INVALID_ARG
    assert torch_ops.train_ternary_supported(4096, 1000) and not torch_ops.train_ternary_supported(4100, 1000)
    assert not torch_ops.train_ternary_supported(66, 256) and not torch_ops.train_ternary_supported(64, 1002)
    assert torch_ops.train_mask_supported(512, 32768) and not torch_ops.train_mask_supported(65536, 32768)


def test_forward_train_and_mask_methods_refuse_on_the_host():
    m = TernarySparseAutoencoder(64, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_train(torch.zeros(2, 64))
    for call in (lambda: m.decoder.init_mask(0.7), lambda: m.decoder.update_mask(0.1), lambda: m.decoder.update_mask(0.1, 0.7, check=True),
                 lambda: m.decoder.mask_grad()):
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            call()
    assert m.decoder.activation_mean is None and m.decoder.output_grad_mean is None
    assert sorted(m.state_dict()) == ["decoder.mask", "decoder.weight", "encoder.0.bias", "encoder.0.weight"]


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_fp64_table_matches_reference_fixtures(name):
    """The util is what the full-size GPU tests are measured against: here it is held to the reference's own autograd on
    the CPU (fp32 reference against the fp64 table; 1e-5 asserted, the figures are printed)."""
    meta, z = U.load_fixture(name)
    sd, x_np = U.masked_params(meta, meta["seed"])
    D, H, B = meta["D"], meta["H"], meta["B"]
    assert z["min_abs_pre"] >= 3e-5
    assert np.array_equal(U.unpack_mask(z["mask"], D, H), sd["decoder.mask"])
    W, b, w, m = (sd[k] for k in ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.mask"))
    recon, min_abs = U.forward64(x_np, W, b, w)
    assert min_abs == pytest.approx(float(z["min_abs_pre"]), rel=1e-3)
    assert U.max_rel_err(recon, z["recon"]) <= TOL
    G = U.trainer_incoming(x_np, recon, B, D)
    gh = U.l1_incoming(x_np, W, b, meta["l1"]) if meta["l1"] > 0 else None
    g = U.grads64(x_np, W, b, w, m, G, gh, want_dx=True)
    for key in U.PARAM_KEYS + ("x",):
        err = U.max_rel_err(g[key], z["grad." + key])
        print(f"{name} {key}: {err:.3g}")
        assert err <= TOL, f"{name} {key}: {err:.3g}"
    # (the mse target is detached in the generator, so grad.x is the encoder path alone)
    assert U.max_rel_err(g["a"], z["a"]) <= TOL and U.max_rel_err(G.mean(0), z["delta"]) <= TOL
    assert np.all(z["grad.decoder.weight"][sd["decoder.mask"] == 0] == 0)


@pytest.mark.parametrize("name", sorted(U.MASK_CASES))
def test_mask_restatement_matches_reference_fixtures(name):
    """init_mask and update_mask as exact integer logic against the reference's masks and weights, bit for bit."""
    meta, z = U.load_fixture(name)
    D, H = meta["D"], meta["H"]
    w0, a, delta = U.mask_case_inputs(meta, meta["seed"])
    w1, m1 = U.init_mask_ref(torch.from_numpy(w0), U.SPARSITY)
    assert meta["init_key"] != meta["init_next_key"]
    assert np.array_equal(m1.numpy(), U.unpack_mask(z["mask_init"], D, H))
    n = U.update_n(D * H, meta["f_decay"])
    assert n == meta["n"]
    if meta["ties"]:
        w1 = U.plant_drop_ties(w1, m1, n)
    assert np.array_equal(w1.numpy().view(np.int32), z["weight_before"].view(np.int32))
    w2, m2, info = U.update_mask_ref(w1, m1, None if a is None else torch.from_numpy(a),
                                     None if delta is None else torch.from_numpy(delta), n)
    assert np.array_equal(m2.numpy(), U.unpack_mask(z["mask_after"], D, H))
    assert np.array_equal(w2.numpy().view(np.int32), z["weight_after"].view(np.int32))
    assert int(info["dropped"].sum()) == meta["dropped"] and int(info["grown"].sum()) == meta["grown"]
    if meta["ties"]:
        assert meta["dropped"] > n                       # the <= rule takes every tie at the threshold
    if meta["stats"] and n > 0:
        assert meta["grow_key"] != meta["grow_next_key"] and meta["grown"] == n
    if not meta["stats"]:
        assert meta["grown"] == 0 and meta["active_after"] == int(m1.sum()) - meta["dropped"]


def test_loop_fixture_is_consistent():
    meta, z = U.load_fixture(U.LOOP_FIXTURE)
    l32, l64 = z["loss32"], z["loss64"]
    assert len(l32) == len(l64) == meta["steps"] == 30
    gap = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
    assert gap == pytest.approx(meta["gap"]) and gap <= 1e-2 and meta["bound"] == pytest.approx(max(10 * gap, 1e-5))
    assert l32[-1] < l32[0]
    assert int(U.unpack_mask(z["mask_final"], meta["D"], meta["H"]).sum()) == meta["active_final"]
    assert meta["mask_diff_fp32_fp64"] == 0
