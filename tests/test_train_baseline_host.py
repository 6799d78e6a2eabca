"""BaselineSparseAutoencoder training: the fp64 restatement against the reference's own gradients, the C-ABI surface, the
dispatcher schemas and the no-CPU-fallback contract (no GPU needed)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantizedsae_amd import BaselineSparseAutoencoder, _lib, torch_ops  # noqa: F401  (registers torch.ops.qsae.*)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_baseline_util as U  # noqa: E402

SYMBOLS = ("qsae_train_table_unit_grad_workspace_bytes", "qsae_train_table_unit_grad", "qsae_normalize_columns_table")
OPS = ("train_table_unit_grad", "normalize_columns_table")
TOL = 1e-5


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_restatement_matches_reference_gradients(name):
    meta, z = U.load_fixture(name)
    sd, x = U.case_inputs(meta, meta["seed"])
    assert z["gap"] >= meta["min_gap"]
    val, recon = U.forward64(x, sd["encoder.0.weight"], sd["encoder.0.bias"], sd["decoder.weight"], sd["decoder.bias"],
                             z["idx"])
    assert np.allclose(val.numpy(), z["val"], rtol=1e-5, atol=1e-6)
    assert abs(U.loss64(x, recon, val, meta["mu"]) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    gR, gL = U.trainer_loss_grads(x, recon, val, meta["mu"])
    g = U.grads64(x, sd["encoder.0.weight"], sd["decoder.weight"], z["idx"], val, gR, gL, want_dx=meta["x_grad"])
    if meta["x_grad"]:
        g["x"] = g["x"] - gR            # the loss reads x directly too (the mse target): d/dx mse = -g_recon
    keys = list(U.GRAD_KEYS) + (["x"] if meta["x_grad"] else [])
    for key in keys:
        err = U.max_rel_err(g[key], z["grad." + key])
        print(f"{name} {key}: {err:.3g}")
        assert err <= TOL, f"{name} {key}: {err:.3g}"


def test_restated_normalisation_matches_the_reference():
    meta, z = U.load_fixture(U.NORMALIZED_CASE)
    sd, _ = U.case_inputs(meta, meta["seed"])
    want = U.normalize64(sd["decoder.weight"])
    err = float((torch.from_numpy(z["normalized.decoder.weight"]).double() - want).abs().max())
    print(f"reference fp32 normalisation vs fp64: {err:.3g}")
    assert err <= 1e-5
    assert float((want.norm(dim=0) - 1).abs().max()) <= 1e-12


def test_fixture_sizes_and_schema():
    assert sorted(U.CASES) == ["train_baseline_d32_k32", "train_baseline_d64", "train_baseline_d64_l1"]
    for name, case in U.CASES.items():
        path = U.GOLDEN / f"{name}.npz"
        assert path.stat().st_size <= 600 * 1024
        meta, z = U.load_fixture(name)
        assert {k: meta[k] for k in case} == case and meta["min_gap"] == 1e-4        # no seed had to be advanced
        B, k, H, D = meta["B"], meta["k"], meta["H"], meta["D"]
        assert z["idx"].shape == (B, k) and z["idx"].dtype == np.int32
        assert z["val"].shape == (B, k) and z["val"].dtype == np.float32
        assert z["gap"].shape == () and z["loss"].shape == ()
        assert z["grad.encoder.0.weight"].shape == (H, D) and z["grad.encoder.0.bias"].shape == (H,)
        assert z["grad.decoder.weight"].shape == (D, H) and z["grad.decoder.bias"].shape == (D,)
        assert ("grad.x" in z) == meta["x_grad"]
        assert ("normalized.decoder.weight" in z) == (name == U.NORMALIZED_CASE)
    assert U.load_fixture(U.NORMALIZED_CASE)[1]["normalized.decoder.weight"].shape == (64, 256)


def test_symbols_declared_exported_and_bound():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    dbg = ctypes.CDLL(str(_lib.DEBUG_LIB_PATH))
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s) and hasattr(dbg, s), s
    assert _lib.ABI_VERSION == 4 and _lib.load().qsae_abi_version() == 4


def test_argument_checks_before_any_device_work():
    lib = _lib.load()
    for fn in (lib.qsae_train_table_unit_grad_workspace_bytes, lib.qsae_train_unit_grad_workspace_bytes):
        assert fn(8192, 32, 32768, 514) == 0                                          # D % 4 != 0
        assert fn(8192, 32, 32768, 8192) == 0                                         # D > 4096
        assert fn(8192, 32, 32768, 512) > 0
    ws = lib.qsae_train_table_unit_grad_workspace_bytes
    assert ws(8192, 257, 32768, 512) == 0                                             # k > 256
    assert ws(1 << 24, 256, 32768, 512) == 0                                          # B k >= 2^31
    # the [H][D] block of per-unit sums rides on top of the binary kernels' layout
    assert ws(8192, 32, 32768, 512) >= lib.qsae_train_unit_grad_workspace_bytes(8192, 32, 32768, 512) + 32768 * 512 * 4
    p = ctypes.c_void_p(256)
    big = ctypes.c_size_t(1 << 40)
    U_ = _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_table_unit_grad(p, p, p, p, 4, 8, p, p, 64, 50, p, p, p, 64, p, big, None) == U_       # D % 4
    assert lib.qsae_train_table_unit_grad(p, p, p, p, 4, 8, p, p, 64, 4100, p, p, p, 64, p, big, None) == U_     # D > 4096
    assert lib.qsae_train_table_unit_grad(p, p, p, p, 4, 300, p, p, 64, 64, p, p, p, 64, p, big, None) == U_     # k > 256
    assert lib.qsae_train_table_unit_grad(p, p, p, p, 1 << 24, 256, p, p, 64, 64, p, p, p, 64, p, big, None) == U_
    assert lib.qsae_train_table_unit_grad(p, p, p, p, 4, 8, p, p, 64, 64, p, p, p, 64, p, 16, None) == _lib.ERR_WORKSPACE
    assert lib.qsae_train_table_unit_grad(p, p, p, p, 4, 8, p, p, 64, 64, p, p, p, 32, p, big, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_normalize_columns_table(p, 64, 66, p, None) == U_                                            # H % 4
    assert lib.qsae_normalize_columns_table(None, 64, 64, p, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_normalize_columns_table(ctypes.c_void_p(260), 64, 64, p, None) == _lib.ERR_INVALID_ARG       # alignment
    assert lib.qsae_normalize_columns_table(p, 0, 64, p, None) == _lib.ERR_INVALID_ARG


def test_ops_have_schemas_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in OPS:
        assert str(getattr(torch.ops.qsae, name).default._schema).startswith(f"qsae::{name}(")
    schema = str(torch.ops.qsae.normalize_columns_table.default._schema)
    assert "Tensor(a0!) W" in schema, schema                                         # the mutation of W is declared
    Q = torch.ops.qsae
    with FakeTensorMode():
        B, D, H, k = 96, 512, 4096, 8
        idx = torch.empty(B, k, dtype=torch.int32)
        off, ent = Q.train_csr(idx, H)
        gR, x, val, gv = torch.empty(B, D), torch.empty(B, D), torch.empty(B, k), torch.empty(B, k)
        dW, db, dWd = Q.train_table_unit_grad(off, ent, val, gv, x, gR, True, True)
        assert dW.shape == (H, D) and db.shape == (H,) and dWd.shape == (D, H)
        assert dW.dtype == db.dtype == dWd.dtype == torch.float32
        dW, db, dWd = Q.train_table_unit_grad(off, ent, val, gv, x, None, False, True)
        assert dW.shape == (0, D) and db.shape == (0,) and dWd.shape == (D, H)
        dW, db, dWd = Q.train_table_unit_grad(off, ent, val, gv, x, gR, True, False)
        assert dW.shape == (H, D) and dWd.shape == (D, 0)
        W = torch.empty(D, H)
        assert Q.normalize_columns_table(W, True).shape == (H, D)
        assert Q.normalize_columns_table(W, False).shape == (0, D)


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from quantizedsae_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.normalize_columns_table(torch.randn(8, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.train_table_unit_grad(torch.zeros(65, dtype=torch.int32), torch.zeros(32, dtype=torch.int32), torch.zeros(4, 8),
                                  torch.zeros(4, 8), torch.zeros(4, 16), None)
    assert ops.normalize_columns_supported(32768) and not ops.normalize_columns_supported(66)


def test_forward_train_refuses_cpu_tensors():
    model = BaselineSparseAutoencoder(64, 1024)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_train(torch.randn(8, 64))


def test_packed_cache_put_replaces_the_value_for_the_current_state():
    from quantizedsae_amd.sae.base import PackedCache
    w = torch.zeros(4, 4)
    cache = PackedCache()
    assert cache.get((w,), lambda: {"t": 1})["t"] == 1
    cache.put((w,), {"t": 2})
    assert cache.get((w,), lambda: {"t": 3})["t"] == 2           # same state: the installed value is served
    w.add_(1.0)                                                  # a version bump still invalidates it
    assert cache.get((w,), lambda: {"t": 3})["t"] == 3


def test_cpu_model_normalisation_keeps_the_torch_path():
    """normalize_decoder_weights() on a model that is not on the GPU (or whose hidden_dim is not a multiple of 4) is the
    reference's three torch ops, as before."""
    meta, z = U.load_fixture(U.NORMALIZED_CASE)
    sd, _ = U.case_inputs(meta, meta["seed"])
    model = BaselineSparseAutoencoder(meta["D"], meta["H"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.normalize_decoder_weights()
    got = model.decoder.weight.detach().double()
    assert float((got - U.normalize64(sd["decoder.weight"])).abs().max()) <= 1e-5
    assert float((got - torch.from_numpy(z["normalized.decoder.weight"]).double()).abs().max()) <= 1e-5
