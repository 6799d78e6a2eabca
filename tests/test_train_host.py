"""BinarySAE training: the fp64 restatement against the reference's own gradients, the C-ABI surface, the dispatcher
schema and the no-CPU-fallback contract (no GPU needed)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantizedsae_amd import BinarySAE, _lib, torch_ops  # noqa: F401  (registers torch.ops.qsae.*)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_util as U  # noqa: E402

SYMBOLS = ("qsae_binary_soft_table_polarize_workspace_bytes", "qsae_binary_soft_table_polarize",
           "qsae_train_csr_workspace_bytes", "qsae_train_csr", "qsae_train_row_grad",
           "qsae_train_unit_grad_workspace_bytes", "qsae_train_unit_grad", "qsae_train_col_sum_workspace_bytes",
           "qsae_train_col_sum")
OPS = ("binary_soft_table_polarize", "train_csr", "train_row_grad", "train_unit_grad", "train_col_sum")
TOL = 1e-5


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_restatement_matches_reference_gradients(name):
    meta, z = U.load_fixture(name)
    sd, x = U.case_inputs(meta, meta["seed"])
    assert z["gap"] >= meta["min_gap"]
    n, gamma = meta["n_bits"], meta["gamma"]
    val, recon, pol = U.forward64(x, sd["encoder.0.weight"], sd["encoder.0.bias"], sd["decoder.weight"],
                                  sd["decoder.bias"], n, gamma, z["idx"])
    assert np.allclose(val.numpy(), z["val"], rtol=1e-5, atol=1e-6)
    assert abs(pol - float(z["polarize"])) <= 1e-6 * abs(float(z["polarize"]))
    gR, gL, gP = U.trainer_loss_grads(x, recon, val, meta["lam"], meta["mu"])
    g = U.grads64(x, sd["encoder.0.weight"], sd["decoder.weight"], n, gamma, z["idx"], val, gR, gL, gP,
                  want_dx=meta["x_grad"])
    if meta["x_grad"]:
        g["x"] = g["x"] - gR            # the loss reads x directly too (the mse target): d/dx 0.5 mse = -g_recon
    keys = list(U.GRAD_KEYS) + (["x"] if meta["x_grad"] else [])
    for key in keys:
        err = U.max_rel_err(g[key], z["grad." + key])
        assert err <= TOL, f"{name} {key}: {err:.3g}"


def test_fixture_sizes_and_schema():
    for name in U.CASES:
        path = U.GOLDEN / f"{name}.npz"
        assert path.stat().st_size <= 600 * 1024
        meta, z = U.load_fixture(name)
        B, k, H, D, n = meta["B"], meta["k"], meta["H"], meta["D"], meta["n_bits"]
        assert z["idx"].shape == (B, k) and z["idx"].dtype == np.int32 and z["val"].shape == (B, k)
        assert z["grad.decoder.weight"].shape == (H, D * n) and z["grad.encoder.0.weight"].shape == (H, D)
        assert ("grad.x" in z) == meta["x_grad"]


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
    assert lib.qsae_train_unit_grad_workspace_bytes(8192, 65, 32768, 514) == 0        # D % 4 != 0
    assert lib.qsae_train_unit_grad_workspace_bytes(8192, 65, 32768, 8192) == 0       # D > 4096
    assert lib.qsae_train_unit_grad_workspace_bytes(8192, 65, 32768, 512) > 0
    assert lib.qsae_train_csr_workspace_bytes(8192, 65, 0) == 0
    p = ctypes.c_void_p(256)
    assert lib.qsae_train_row_grad(p, 4, 8, p, 64, 50, 1.0, None, None, 0, None, p, None, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_row_grad(p, 4, 300, p, 64, 64, 1.0, None, None, 0, None, p, None, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_train_csr(p, 4, 8, 64, p, p, p, 16, None) == _lib.ERR_WORKSPACE
    assert lib.qsae_binary_soft_table_polarize(p, 64, 64, 9, p, p, p, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_train_col_sum(p, 4, 64, p, p, 0, None) == _lib.ERR_WORKSPACE


def test_ops_have_schemas_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in OPS:
        assert str(getattr(torch.ops.qsae, name).default._schema).startswith(f"qsae::{name}(")
    Q = torch.ops.qsae
    with FakeTensorMode():
        B, D, H, k, n = 96, 512, 4096, 8, 4
        logits = torch.empty(H, D * n)
        table, pol = Q.binary_soft_table_polarize(logits, D, n)
        assert table.shape == (H, D) and table.dtype == torch.float32 and pol.shape == () and pol.dtype == torch.float32
        idx = torch.empty(B, k, dtype=torch.int32)
        off, ent = Q.train_csr(idx, H)
        assert off.shape == (H + 1,) and ent.shape == (B * k,) and off.dtype == ent.dtype == torch.int32
        gR, x = torch.empty(B, D), torch.empty(B, D)
        gv, dx = Q.train_row_grad(idx, table, 0.5, gR, None, torch.empty(H, D), True)
        assert gv.shape == (B, k) and gv.dtype == torch.float32 and dx.shape == (B, D)
        assert Q.train_row_grad(idx, table, 0.5, gR, None, None, False)[1].shape == (0, D)
        dW, db, dl = Q.train_unit_grad(off, ent, torch.empty(B, k), gv, x, gR, logits, n, 0.5, torch.empty(()), True, True)
        assert dW.shape == (H, D) and db.shape == (H,) and dl.shape == (H, D * n) and dl.dtype == torch.float32
        dW, db, dl = Q.train_unit_grad(off, ent, torch.empty(B, k), gv, x, None, logits, n, 0.5, None, False, True)
        assert dW.shape == (0, D) and db.shape == (0,) and dl.shape == (H, D * n)
        assert Q.train_col_sum(gR).shape == (D,)


def test_forward_train_refuses_cpu_tensors():
    model = BinarySAE(64, 1024, gamma=4.0, n_bits=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_train(torch.randn(8, 64))
