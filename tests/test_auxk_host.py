"""AuxK without a GPU: hand-worked cases of the two numpy restatements (tests/auxk_util.py), the ledger of the extension
header -- every function declared in include/qsae_ext.h is bound in _lib.EXT_SIGNATURES with as many arguments as it
declares, is exported by the built library as qsaex_*, and is either a *_bytes sizer or driven between guard words in
tests/test_auxk_gpu.py -- the Trainer's argument validation, the front ends' refusal of host tensors, and the calls of the
C ABI that return before they look at a pointer."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import auxk_util as U
import test_auxk_gpu as G
from quantizedsae_amd import _lib, build, ops, torch_ops, training
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE
from quantizedsae_amd.training import Trainer, aux_k_loss

ROOT = Path(__file__).resolve().parents[1]
CONFIG = {"input_dim": 16, "n_bits": 4, "hidden_dim": 64, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 4,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 32}


# ---- the restatements, by hand ----------------------------------------------------------------------------------------
def test_subset_topk_by_hand():
    x = np.array([[1, 2, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    W = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 1, 0, 0], [9, 9, 9, 9]], dtype=np.float32)
    bias = np.array([0.5, 0, -1, 0, 100], dtype=np.float32)
    # row 0: units 0..3 give 1.5, 2, 2, 2 -- the tie at 2 goes to the lower unit; unit 4 is not listed
    # row 1: the biases 0.5, 0, -1, 0
    idx, val = U.subset_topk(x, W, bias, [0, 1, 2, 3], 3)
    assert idx.tolist() == [[1, 2, 3], [0, 1, 3]]
    assert val.tolist() == [[2, 2, 2], [0.5, 0, 0]]
    # entries outside [0, 5) are no candidates; fewer inside than k leaves (-1, +0)
    idx, val = U.subset_topk(x, W, bias, [-2, 0, 2, 5], 3)
    assert idx.tolist() == [[2, 0, -1], [0, 2, -1]] and val.tolist() == [[2, 1.5, 0], [0.5, -1, 0]]


def test_key_order_by_hand():
    v = np.array([-np.inf, -1, -0.0, 0.0, 1e-45, 1, np.inf, np.nan], dtype=np.float32)
    m = U.mono(v).astype(np.int64)
    assert (np.diff(m) >= 0).all() and m[2] == m[3] and m[-1] == 0xFFFFFFFF and m[-2] < m[-1]      # NaN above +inf, -0 == +0
    back = U.key_value(U.mono(v))
    assert np.array_equal(back[[0, 1, 3, 4, 5, 6]], v[[0, 1, 3, 4, 5, 6]]) and np.isnan(back[-1])
    assert back.view(np.uint32)[2] == 0                                       # a -0.0 comes back as +0.0


def test_loss_by_hand():
    # e = (2, 0), m = 1, Dn = 2; q = aux - e = (-1, 1), N = 2: loss = 0.5 * 2 / 2, s = 2 * 0.5 / 2
    x, recon, aux = (np.array(v, dtype=np.float32).reshape(2, 1) for v in ([3, 1], [1, 1], [1, 1]))
    loss, grad, sums = U.auxk_loss(x, recon, aux, 0.5)
    assert loss == 0.5 and grad.reshape(-1).tolist() == [-0.5, 0.5] and sums.tolist() == [2.0, 2.0]
    # two columns, each with its own mean: e = [[1, 4], [3, 0]], m = (2, 2), Dn = 1 + 4 + 1 + 4 = 10; aux = 0: N = 26
    x = np.array([[1, 4], [3, 0]], dtype=np.float32)
    loss, grad, sums = U.auxk_loss(x, np.zeros_like(x), np.zeros_like(x), 1.0)
    assert sums.tolist() == [26.0, 10.0] and loss == np.float32(2.6)
    assert np.array_equal(grad, (np.float32(0.2) * -x).astype(np.float32))
    # one row: e equals its own mean, Dn = 0 -> loss 0, grad 0
    loss, grad, sums = U.auxk_loss(np.ones((1, 3), np.float32), np.zeros((1, 3), np.float32), np.full((1, 3), 5, np.float32), 1.0)
    assert loss == 0 and not grad.any() and sums.tolist() == [48.0, 0.0]


def test_loss_restatement_is_close_to_plain_fp64():
    x, recon, aux = U.gaussian(1, 70, 300), U.gaussian(2, 70, 300), U.gaussian(3, 70, 300)
    loss, grad, sums = U.auxk_loss(x, recon, aux, 1 / 32)
    e = x.astype(np.float64) - recon
    N, Dn = ((aux - e) ** 2).sum(), ((e - e.mean(0)) ** 2).sum()
    assert abs(sums[0] - N) < 1e-6 * N and abs(sums[1] - Dn) < 1e-6 * Dn
    assert abs(loss - N / Dn / 32) < 1e-6 * loss
    np.testing.assert_allclose(grad, (aux - e) / Dn / 16, rtol=1e-5, atol=1e-12)


# ---- the extension ledger ---------------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_ext.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_ext.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_extension_is_bound_exported_and_guarded():
    declared = _declared()
    assert declared and sorted(declared) == sorted(_lib.EXT_SIGNATURES)
    assert all(n.startswith("qsaex_") and not n.startswith("qsae_") for n in declared)
    assert not set(declared) & set(_lib.SIGNATURES)
    for name, n_params in declared.items():
        assert len(_lib.EXT_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaex_")) == sorted(declared)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    sizers = {n for n in declared if n.endswith("_bytes")}
    guarded = {entry for entry, _ in G.GUARD_CASES.values()}
    assert sizers | guarded == set(declared) and not sizers & guarded
    assert all(n + "_workspace_bytes" in sizers for n in guarded)            # every guarded call has its sizer
    assert "auxk.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    header = (ROOT / "include" / "qsae_ext.h").read_text()
    assert "join qsae.h" in header


# ---- calls that need no device ----------------------------------------------------------------------------------------
def test_calls_that_launch_nothing_and_shapes_the_sizers_refuse():
    lib = _lib.load()
    topk, size = lib.qsaex_encode_topk_units, lib.qsaex_encode_topk_units_workspace_bytes
    null = [None] * 3

    def call(B, D, H, n, k):
        return topk(None, D, None, D, None, B, D, H, None, n, k, None, None, None, 0, None)
    assert call(0, 16, 64, 8, 4) == _lib.OK and call(5, 16, 64, 0, 4) == _lib.OK          # B == 0, n_units == 0
    assert call(-1, 16, 64, 8, 4) == _lib.ERR_INVALID_ARG
    for B, D, H, n, k in ((5, 16, 64, 8, 0), (5, 16, 64, 100, 65), (5, 16, 64, 8, 9), (5, 18, 64, 8, 4), (5, 0, 64, 8, 4)):
        assert call(B, D, H, n, k) == _lib.ERR_UNSUPPORTED, (B, D, H, n, k)
        assert b"qsaex_encode_topk_units" in lib.qsae_last_error()
        assert size(B, D, n, k) == 0
    assert size(5, 16, 8, 4) > 0 and size(0, 16, 8, 4) == 0 and size(5, 16, 0, 4) == 0
    assert call(5, 16, 64, 8, 4) == _lib.ERR_INVALID_ARG                                  # null pointers, found before any launch
    # monotone in B, n_units and k
    assert size(129, 36, 131, 64) <= size(130, 36, 131, 64) <= size(130, 36, 132, 64) and size(130, 36, 131, 7) <= size(130, 36, 131, 8)
    loss, lsize = lib.qsaex_auxk_loss, lib.qsaex_auxk_loss_workspace_bytes
    assert loss(*null, 0, 16, 1.0, None, None, None, None, 0, None) == _lib.OK             # B == 0
    assert loss(*null, -1, 16, 1.0, None, None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert loss(*null, 4, 0, 1.0, None, None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert loss(*null, 4, 16, 1.0, None, None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert lsize(0, 16) == 0 and lsize(4, 0) == 0 and lsize(257, 36) == 3072


def test_front_ends_refuse_host_tensors():
    x, W, b = torch.zeros(2, 4), torch.zeros(8, 4), torch.zeros(8)
    units = torch.arange(4, dtype=torch.int32)
    for mod in (ops, torch_ops):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod.encode_topk_units(x, W, b, units, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod.auxk_loss(x, x, x, 1.0)
    for model in (BaselineSparseAutoencoder(4, 8), BinarySAE(4, 8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_aux(x, units, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            aux_k_loss(model, x, x, units, 2)
    assert "aux_k_loss" in training.__all__


# ---- Trainer arguments ------------------------------------------------------------------------------------------------
def test_trainer_accepts_and_validates_aux_k(tmp_path):
    t = Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path))
    assert t.aux_k is None and t.activity is None
    for bad in (0, -3, 65):
        with pytest.raises(ValueError, match="aux_k"):
            Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), activity_window=100, aux_k=bad)
    with pytest.raises(ValueError, match="64"):
        Trainer(CONFIG, "b_sae", False, True, dataset_dir=str(tmp_path), activity_window=100, aux_k=65)
    with pytest.raises(ValueError, match="aux_k needs activity_window"):
        Trainer(CONFIG, "b_sae", False, True, dataset_dir=str(tmp_path), aux_k=4)
    for st in ("q_sae", "rq_sae", "bl_sae", "t_sae"):
        with pytest.raises(ValueError, match="baseline_sae and b_sae"):
            Trainer(CONFIG, st, st == "t_sae", True, dataset_dir=str(tmp_path), activity_window=100, aux_k=4)
    with pytest.raises(ValueError, match="aux_refresh"):
        Trainer(CONFIG, "b_sae", False, True, dataset_dir=str(tmp_path), activity_window=100, aux_k=4, aux_refresh=0)
    for st in ("baseline_sae", "b_sae"):
        t = Trainer(CONFIG, st, False, True, dataset_dir=str(tmp_path), activity_window=100, aux_k=4, log_every=7)
        assert t.aux_k == 4 and t.aux_coef == 1 / 32 and t.aux_refresh == 7 and t.model.activity is t.activity
        t = Trainer(CONFIG, st, False, True, dataset_dir=str(tmp_path), activity_window=100, aux_k=64, aux_coef=0.5, aux_refresh=3,
                    resample_every=4)
        assert t.aux_k == 64 and t.aux_coef == 0.5 and t.aux_refresh == 3 and t.resample_every == 4
