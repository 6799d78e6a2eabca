"""Strongest activations per feature without a GPU: the numpy restatement against a brute-force loop, the C ABI's
symbols and argument checks (answered before any HIP call -- the only reason these calls can be made without a device),
the workspace sizes, the Python front-end's own checks, the unchanged ``top_examples=None`` path of the dataset analysis,
and the inspector's overview / sensitivity / specificity against what the reference's own methods recorded
(tests/golden/inspector_overview.npz, tools/gen_golden_inspector_overview.py)."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import top_examples_util as U
from quantizedsae_amd import BinarySAE, QuantizedMatryoshkaSAE, _lib, build
from quantizedsae_amd.inference import DictionaryInspector, FeatureOverview, TopExamples, examples_to_python
from quantizedsae_amd.inference import analysis as A
from quantizedsae_amd.inference import framework as F

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("qsae_top_examples_compact_workspace_bytes", "qsae_top_examples_compact", "qsae_top_examples_dense_workspace_bytes",
         "qsae_top_examples_dense", "qsae_top_examples_decode")


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_key_order_is_value_descending_then_position_ascending():
    v = np.array([2.0, 2.0, 1.0, 1e-30, np.inf, 0.0, -0.0, -1.0, -np.inf], np.float32)
    p = np.array([7, 3, 0, 0, 9, 1, 1, 0, 0])
    keys = U.full_key(v, p)
    assert keys[4] > keys[1] > keys[0] > keys[2] > keys[3] > keys[5] > keys[7] > keys[8] > 0
    assert keys[5] == keys[6]                                   # -0.0 as +0.0
    assert np.array_equal(U.key_value(keys)[[0, 2, 4, 7]], v[[0, 2, 4, 7]]) and np.array_equal(U.key_position(keys), p)
    assert U.full_key(np.float32([1.0]), [2 ** 32 - 1])[0] & np.uint64(0xFFFFFFFF) == 0


@pytest.mark.parametrize("seed,B,k,H,n,floor", [(1, 9, 3, 7, 2, 0.0), (2, 20, 4, 6, 64, 0.0), (3, 15, 2, 5, 3, 0.4), (4, 1, 1, 3, 1, 0.0)])
def test_restatement_equals_a_brute_force_loop(seed, B, k, H, n, floor):
    idx, val = U.compact_case(seed, B, k, H)
    base = 1000
    triples = [(int(idx[r, j]), val[r, j], base + r) for r in range(B) for j in range(k) if 0 <= idx[r, j] < H and val[r, j] == val[r, j]]
    want = U.restate_loop(H, n, triples, floor)
    got = U.restate(H, n, *U.candidates_compact(idx, val, H, base, floor))
    assert np.array_equal(got, want)
    # any cut into batches, each joined with the state so far, gives the same keys; so does the dense form
    state = None
    for a, b in zip(U.splits(B, 3)[:-1], U.splits(B, 3)[1:]):
        state = U.restate(H, n, *U.candidates_compact(idx[a:b], val[a:b], H, base + a, floor), old=state)
    assert np.array_equal(state, want)
    lat = np.full((B, H + 2), np.nan, np.float32)
    lat[:, :H] = -1.0
    for r in range(B):
        for j in range(k):
            if 0 <= idx[r, j] < H:
                lat[r, idx[r, j]] = val[r, j]
    assert np.array_equal(U.restate(H, n, *U.candidates_dense(lat, H, base, max(floor, 0.0))), want)
    values, positions, counts = U.decode(want)
    assert ((positions >= base) == (want != 0)).all() and (counts == (want != 0).sum(1)).all()
    assert (np.diff(want.astype(object), axis=1) <= 0).all()    # descending, 0-padded


def test_planted_cases_hold_what_they_promise():
    for B, k, H, n in U.COMPACT_CASES:
        idx, val = U.compact_case(11 + B, B, k, H)
        ok = (idx >= 0) & (idx < H)
        assert (idx[:, 0] == 0).all() and not (idx == H - 1).any()
        for r in range(B):
            u = idx[r][ok[r]]
            assert len(set(u.tolist())) == len(u)              # distinct units per row
        if k >= 2:
            assert (~ok).any() and np.isnan(val).any() and (val < 0).any() and (val == 0).any() and np.signbit(val[val == 0]).any()
        if k >= 2 and H >= 4 and B >= 5:
            assert (val[idx == 2] == 0.5).sum() >= 2 or np.isnan(val[idx == 2]).any()
    for B, H, ld, n in U.DENSE_CASES:
        lat = U.dense_case(21 + B, B, H, ld)
        assert np.isnan(lat[:, H:]).all() and (H < 2 or not (lat[:, H - 1] > 0).any())


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "qsae.h").read_text()
    lib = _lib.load()
    assert _lib.DEBUG_LIB_PATH.exists(), "build with `python -m quantizedsae_amd.build`"
    for exported in (build.exported_symbols(_lib.LIB_PATH), build.exported_symbols(_lib.DEBUG_LIB_PATH)):
        for name in NAMES:
            assert re.search(rf"\b{name}\(", header)
            assert name in _lib.SIGNATURES and name in exported
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "top_examples.hip" in build.SOURCES
    assert lib.qsae_abi_version() == _lib.ABI_VERSION == 4     # an additive change
    src = (ROOT / "quantizedsae_amd" / "csrc" / "topk_lists.h").read_text()
    assert f"kTopkListMaxK = {U.MAX_N};" in src


def test_workspaces_are_monotone_and_zero_for_invalid_shapes():
    lib = _lib.load()
    compact, dense = lib.qsae_top_examples_compact_workspace_bytes, lib.qsae_top_examples_dense_workspace_bytes
    grid = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4500, 32768, 65536)
    for fixed in (1, 65, 1025):
        b = [compact(v, fixed, fixed) for v in grid]
        k = [compact(fixed, v, fixed) for v in grid]
        h = [compact(fixed, fixed, v) for v in grid[1:]]
        assert b == sorted(b) and k == sorted(k) and h == sorted(h) and b[0] > 0 and k[0] > 0 and h[0] > 0
        for n in (1, 8, 64):
            b = [dense(v, fixed, n) for v in grid]
            h = [dense(fixed, v, n) for v in grid[1:]]
            assert b == sorted(b) and h == sorted(h)
        ns = [dense(fixed, fixed, n) for n in range(1, 65)]
        assert ns == sorted(ns)
    assert dense(64, 4096, 8) == 0 and dense(65, 4096, 8) >= 2 * 4096 * 8 * 8        # one chunk is never split
    assert dense(8192, 32768, 64) >= 2 * 32768 * 64 * 8                              # two splits of the flagship width
    for bad in ((-1, 4, 8), (4, -1, 8), (4, 4, 0), (4, 4, -1), (65536, 32768, 8), (2 ** 30, 2, 8)):
        assert compact(*bad) == 0, bad
    for bad in ((-1, 8, 4), (4, 0, 4), (4, -1, 4), (4, 8, 0), (4, 8, 65), (4, 8, -1)):
        assert dense(*bad) == 0, bad


def _compact(lib, *, idx=0x1000, val=0x2000, B=8, k=3, H=16, n=4, floor=0.0, base=0, keys=0x3000, ws=0x6000, ws_bytes=1 << 20):
    """Dummy non-null pointers: a call that got as far as a kernel launch would not return an argument error."""
    return lib.qsae_top_examples_compact(idx, val, B, k, H, n, floor, base, keys, ws, ws_bytes, None)


def _dense(lib, *, latent=0x1000, ld=16, B=80, H=16, n=4, floor=0.0, base=0, keys=0x3000, ws=0x6000, ws_bytes=1 << 20):
    return lib.qsae_top_examples_dense(latent, ld, B, H, n, floor, base, keys, ws, ws_bytes, None)


@pytest.mark.parametrize("bad", [dict(idx=None), dict(keys=None), dict(B=-1), dict(k=-1), dict(H=0), dict(H=-3), dict(n=0), dict(n=-1),
                                 dict(floor=float("nan")), dict(base=2 ** 32 - 7), dict(ws=0x6004)])
def test_compact_refuses_invalid_arguments_before_any_hip_call(bad):
    lib = _lib.load()
    assert _compact(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_top_examples_compact" in lib.qsae_last_error()


@pytest.mark.parametrize("bad", [dict(latent=None), dict(keys=None), dict(B=-1), dict(H=0), dict(n=0), dict(ld=15),
                                 dict(floor=float("nan")), dict(base=2 ** 32 - 79), dict(ws=0x6004)])
def test_dense_refuses_invalid_arguments_before_any_hip_call(bad):
    lib = _lib.load()
    assert _dense(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_top_examples_dense" in lib.qsae_last_error()


def test_limits_workspace_and_nothing_to_do():
    lib = _lib.load()
    assert _compact(lib, n=65) == _lib.ERR_UNSUPPORTED and _dense(lib, n=65) == _lib.ERR_UNSUPPORTED
    assert _compact(lib, n=65, B=0) == _lib.ERR_UNSUPPORTED                          # also when there is nothing to do
    assert _compact(lib, B=65536, k=32768) == _lib.ERR_UNSUPPORTED                   # B * k = 2^31
    need = lib.qsae_top_examples_compact_workspace_bytes(8, 3, 16)
    assert _compact(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and _compact(lib, ws=None) == _lib.ERR_WORKSPACE
    need = lib.qsae_top_examples_dense_workspace_bytes(80, 16, 4)
    assert need > 0 and _dense(lib, ws_bytes=2 * 16 * 4 * 8 - 1) == _lib.ERR_WORKSPACE and _dense(lib, ws=None) == _lib.ERR_WORKSPACE
    # nothing to do: no pointer is looked at
    assert _compact(lib, B=0, idx=None, val=None, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _compact(lib, k=0, idx=None, val=None, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _dense(lib, B=0, latent=None, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _compact(lib, B=0, base=2 ** 32 - 1 + 1 - 1) == _lib.OK                    # base + 0 <= 2^32
    dec = lib.qsae_top_examples_decode
    assert dec(None, 4, 2, 0x1000, 0x2000, 0x3000, None) == _lib.ERR_INVALID_ARG
    assert dec(0x1000, 0, 2, 0x1000, 0x2000, 0x3000, None) == _lib.ERR_INVALID_ARG
    assert dec(0x1000, 4, 0, 0x1000, 0x2000, 0x3000, None) == _lib.ERR_INVALID_ARG
    assert dec(0x1000, 4, 65, 0x1000, 0x2000, 0x3000, None) == _lib.ERR_UNSUPPORTED


# ---- the Python front-end ----------------------------------------------------------------------------------------------
def test_top_examples_rejects_bad_n_and_positions_past_32_bits():
    for n in (0, -1, 65, 1000):
        with pytest.raises(ValueError, match="n must lie in 1 .. 64"):
            TopExamples(16, n, "cpu")
    with pytest.raises(ValueError, match="H must be positive"):
        TopExamples(0, 4, "cpu")
    with pytest.raises(ValueError, match="NaN"):
        TopExamples(16, 4, "cpu", floor=float("nan"))
    te = TopExamples(16, 4, "cpu")
    assert te.keys.shape == (16, 4) and te.keys.dtype == torch.int64 and not te.keys.any()
    idx = torch.zeros((8, 2), dtype=torch.int32)
    for base in (2 ** 32 - 7, 2 ** 32, -1):
        with pytest.raises(ValueError, match="base"):
            te.add_compact(idx, None, base)
        with pytest.raises(ValueError, match="base"):
            te.add_dense(torch.zeros((8, 16)), base)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # base + B == 2^32 passes the check and reaches the op
        te.add_compact(idx, None, 2 ** 32 - 8)


def test_examples_to_python():
    res = {"values": torch.tensor([[3.0, 1.5], [0.0, 0.0], [2.0, 0.0]]), "positions": torch.tensor([[7, 2], [-1, -1], [5, -1]]),
           "counts": torch.tensor([2, 0, 1], dtype=torch.int32)}
    token_ids = torch.arange(100, 112).reshape(4, 3)
    assert examples_to_python(res, token_ids, 3) == [[(3.0, 2, 1, 107), (1.5, 0, 2, 102)], [], [(2.0, 1, 2, 105)]]


def test_analysis_without_top_examples_returns_todays_keys_and_threshold_models_refuse():
    sae = F.SAEWrapper(F.SAE_REGISTRY["b_sae"], BinarySAE(64, 1024, gamma=4.0, n_bits=4), "cpu")
    kw = dict(token_ids=torch.zeros((1, 1), dtype=torch.long), tokens_per_context=1)
    st = A.analyze_dataset(sae, [], **kw)                       # an empty loader: nothing is computed
    assert set(st) == {"mse_final", "mse_per_level", "l0_per_level", "activation_counts", "coactivation", "tokens_per_feature"}
    st = A.compute_activation_stats(sae, [], coactivation=None, **kw)
    assert set(st) == {"activation_counts", "coactivation", "tokens_per_feature"}
    q = F.SAEWrapper(F.SAE_REGISTRY["q_sae"], QuantizedMatryoshkaSAE(64, 1024, top_k=8, abs_range=4, n_bits=4), "cpu")
    for fn in (A.analyze_dataset, A.compute_activation_stats):
        with pytest.raises(TypeError, match="one bit per unit"):
            fn(q, [], top_examples=8, **kw)
        with pytest.raises(ValueError, match="n must lie"):
            fn(sae, [], top_examples=65, **kw)


# ---- the inspector against the reference's own methods -------------------------------------------------------------------
def _golden():
    z = np.load(ROOT / "tests" / "golden" / "inspector_overview.npz")
    return z, json.loads(bytes(z["meta"]).decode())


def test_overview_sensitivity_and_specificity_equal_the_reference():
    z, meta = _golden()
    fa = z["feature_activations"]
    H, tokens = meta["H"], meta["tokens"]
    assert fa.shape == (meta["lines"], tokens) and z["counts"][meta["dead"]] == 0       # a feature that never wins
    # the fixture's CSR is the restatement of the reference's loop: per feature the flat positions in ascending order
    flat = fa.reshape(-1)
    order = np.argsort(flat, kind="stable")
    assert np.array_equal(z["positions"], order) and np.array_equal(z["counts"], np.bincount(flat, minlength=H))
    ov = FeatureOverview(torch.from_numpy(z["counts"]), torch.from_numpy(z["offsets"]), torch.from_numpy(z["positions"]).int(), tokens)
    d = ov.to_python()
    assert set(d) == set(np.unique(flat).tolist()) and meta["dead"] not in d
    for f, e in d.items():
        assert e["cnt"] == int((flat == f).sum())
        assert e["pos"] == [(int(g) // tokens, int(g) % tokens) for g in np.nonzero(flat == f)[0]]
    toks = z["tokens"]
    for i, (f, targets) in enumerate(meta["pairs"]):
        mask = np.array([[any(t in tok for t in targets) for tok in row] for row in toks.tolist()])
        assert np.array_equal(mask, z["match_masks"][i])        # the mask is the caller's job; this is the reference's way
        m = torch.from_numpy(z["match_masks"][i])
        assert DictionaryInspector.check_sensitivity(torch.from_numpy(fa), m, f) == z["sensitivity"][i]
        assert DictionaryInspector.check_sensitivity(fa.tolist(), m, f) == z["sensitivity"][i]
        assert DictionaryInspector.check_specificity(ov, m, f) == z["specificity"][i]
    assert z["specificity"][2] == 0.0 and z["match_masks"][2].any()                     # a target that never meets a win
    with pytest.raises(KeyError):
        DictionaryInspector.check_specificity(ov, torch.from_numpy(z["match_masks"][0]), meta["dead"])
    with pytest.raises(ZeroDivisionError):
        DictionaryInspector.check_sensitivity(fa.tolist(), torch.zeros(fa.shape, dtype=torch.bool), 3)
    with pytest.raises(ValueError, match="match_mask"):
        DictionaryInspector.check_sensitivity(fa.tolist(), torch.zeros((2, 2), dtype=torch.bool), 3)
