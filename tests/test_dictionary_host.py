"""Decoder-dictionary comparison: the C-ABI surface, the dispatcher schema and the fixtures (no GPU needed)."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from quantizedsae_amd import _lib, torch_ops  # noqa: F401  (registers torch.ops.qsae.*)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import dictionary_util as U  # noqa: E402

SYMBOLS = ("qsae_atom_inv_norms", "qsae_cosine_compare_workspace_bytes", "qsae_cosine_compare")
GOLDENS = sorted(p.stem for p in (ROOT / "tests" / "golden").glob("dictionary_*.npz"))


def test_symbols_declared_and_exported():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    dbg = ctypes.CDLL(str(_lib.DEBUG_LIB_PATH))
    assert all(hasattr(dbg, s) for s in SYMBOLS)


def test_argument_checks_before_any_device_work():
    lib = _lib.load()
    assert lib.qsae_cosine_compare_workspace_bytes(0, 10, 0) == 0
    ws = lib.qsae_cosine_compare_workspace_bytes(32768, 32768, 0)
    assert 2 * 32768 * 4 < ws < 2 * 32768 * 4 + 4096 * 16 + 4096
    assert lib.qsae_cosine_compare_workspace_bytes(32768, 1, 1) < ws          # triangle: fewer workgroups
    p = ctypes.c_void_p(256)
    args = [p, 512, 100, p, 512, 100, 512, 0, None, 0, 0, p, p, p, p, None, None, None, 0, p, 1 << 30, None]
    bad = list(args)
    bad[6] = 0                                                  # D == 0
    assert lib.qsae_cosine_compare(*bad) == _lib.ERR_INVALID_ARG
    bad = list(args)
    bad[9] = 9                                                  # 9 thresholds
    assert lib.qsae_cosine_compare(*bad) == _lib.ERR_INVALID_ARG
    bad = list(args)
    bad[10] = 4097                                              # bins
    assert lib.qsae_cosine_compare(*bad) == _lib.ERR_INVALID_ARG
    bad = list(args)
    bad[3], bad[4], bad[6] = p, 102, 102                        # D % 4 != 0
    bad[1] = 102
    assert lib.qsae_cosine_compare(*bad) == _lib.ERR_UNSUPPORTED
    bad = list(args)
    bad[20] = 16                                                # workspace too small
    assert lib.qsae_cosine_compare(*bad) == _lib.ERR_WORKSPACE
    assert lib.qsae_atom_inv_norms(None, 64, 0, 64, None, None) == 0
    assert lib.qsae_atom_inv_norms(None, 64, 4, 64, None, None) == _lib.ERR_INVALID_ARG


def test_cosine_compare_schema_and_fake_shapes():
    op = torch.ops.qsae.cosine_compare
    schema = str(op.default._schema)
    assert "Tensor A" in schema and "Tensor? B" in schema and "float[] thresholds" in schema
    assert "Int bins" in schema and "bool want_matrix" in schema
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        A = torch.empty((777, 100), device="cuda" if torch.cuda.is_available() else "meta")
        B = torch.empty((1000, 100), device=A.device)
        out = op(A, B, [0.5, 0.9, 0.1], 64, True)
        assert [tuple(t.shape) for t in out] == [(777,), (1000,), (2,), (2,), (3,), (64,), (777, 1000)]
        assert [t.dtype for t in out] == [torch.int64] * 2 + [torch.float64] + [torch.int64] * 3 + [torch.float32]
        out = op(A, None, [], 0, False)
        assert [tuple(t.shape) for t in out] == [(777,), (0,), (2,), (2,), (0,), (0,), (0, 0)]


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_agrees_with_fp64_restatement(name):
    z = np.load(ROOT / "tests" / "golden" / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    a = U.atoms_np(meta["lhs"], meta["D"], meta["H"])
    b = U.atoms_np(meta["rhs"], meta["D"], meta["H"])
    m = U.cosine_f64(a, b)
    assert z["row_max"].shape == (a.shape[0],) and z["col_max"].shape == (b.shape[0],)
    np.testing.assert_allclose(z["row_max"], m.max(1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(z["col_max"], m.max(0), rtol=0, atol=1e-5)
    rows = np.arange(a.shape[0])
    assert np.all(m.max(1) - m[rows, z["row_argmax"]] <= 2e-5)
    cols = np.arange(b.shape[0])
    assert np.all(m.max(0) - m[z["col_argmax"], cols] <= 2e-5)
    assert abs(float(z["mean"]) - m.mean()) <= 1e-6
    k = min(100, b.shape[0])
    assert abs(float(z["mean_top"]) - np.sort(m.max(1))[-k:].mean()) <= 1e-5
    np.testing.assert_allclose(z["matrix_rows"], m[z["rows"]], rtol=0, atol=1e-5)
    if meta["lhs"].get("zero_atom") is not None:
        zi = meta["lhs"]["zero_atom"]
        assert np.all(z["matrix_rows"][list(z["rows"]).index(zi)] == 0) if zi in z["rows"] else z["row_max"][zi] == 0
    assert len(GOLDENS) == 6
