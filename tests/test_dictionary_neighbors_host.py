"""The nearest-atom query without a GPU: qsae_nearest_atoms_i8 is declared, bound and exported and answers every bad
argument before any HIP call (the only reason these calls can be made without a device); the numpy restatement of the
arithmetic contract is within its derived bound of real arithmetic; the restatement and the torch
one-liners of DictionaryInspector agree with what the reference's own inspector class recorded."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import dictionary_neighbors_util as U
from quantizedsae_amd import _lib, build
from quantizedsae_amd.inference import DictionaryInspector, integer_atoms, nearest_atoms

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("qsae_nearest_atoms_i8_workspace_bytes", "qsae_nearest_atoms_i8")
GOLDENS = sorted(U.GOLDEN_CASES)


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "qsae.h").read_text()
    exported = build.exported_symbols(_lib.LIB_PATH)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header)
        assert name in _lib.SIGNATURES and name in exported
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "dictionary_neighbors.hip" in build.SOURCES
    assert lib.qsae_abi_version() == _lib.ABI_VERSION == 4     # an additive change


def test_workspace_is_monotone_and_zero_for_invalid_shapes():
    size = _lib.load().qsae_nearest_atoms_i8_workspace_bytes
    grid = (1, 5, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4500, 32768)
    for fixed in (1, 130, 2049, 32768):
        for k in (1, 10, 64):
            a = [size(v, fixed, 64, k) for v in grid]
            b = [size(fixed, v, 64, k) for v in grid]
            assert a == sorted(a) and b == sorted(b) and a[0] > 0 and b[0] > 0
        ks = [size(fixed, fixed, 64, k) for k in range(1, 65)]
        assert ks == sorted(ks) and ks[0] > 0
    assert size(300, 200, 64, 10) == size(300, 200, 4096, 10)      # rows are read in place: D costs nothing
    for bad in ((0, 4, 64, 10), (4, 0, 64, 10), (-1, 4, 64, 10), (4, -1, 64, 10), (4, 4, 0, 10), (4, 4, 48, 10),
                (4, 4, 4128, 10), (4, 4, 64, 0), (4, 4, 64, 65), (4, 4, -32, 10)):
        assert size(*bad) == 0, bad


def _call(lib, *, a=0x1000, a_ld=64, Na=8, b=0x3000, b_ld=64, Nb=8, D=64, k=10, exclude_self=0, keys=0x5000, dup=None,
          ws=0x6000, ws_bytes=1 << 20):
    """Dummy non-null pointers: a call that got as far as a kernel launch would not return an argument error."""
    return lib.qsae_nearest_atoms_i8(a, a_ld, Na, b, b_ld, Nb, D, k, exclude_self, keys, dup, ws, ws_bytes, None)


@pytest.mark.parametrize("bad", [
    dict(a=None), dict(keys=None), dict(Na=-1), dict(Nb=-1), dict(a_ld=32), dict(b_ld=32), dict(a_ld=72), dict(b_ld=72),
    dict(a=0x1004), dict(b=0x3008), dict(ws=0x6004), dict(exclude_self=1), dict(dup=0x7000),
    dict(b=None, a_ld=72), dict(b=None, a=0x1004), dict(b=None, Na=-1),
])
def test_invalid_arguments_are_refused_before_any_hip_call(bad):
    lib = _lib.load()
    assert _call(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_nearest_atoms_i8" in lib.qsae_last_error()


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=65), dict(k=-1), dict(D=0), dict(D=16), dict(D=48), dict(D=4128),
                                 dict(D=8192, a_ld=8192, b_ld=8192)])
def test_shapes_outside_the_limits_are_unsupported(bad):
    lib = _lib.load()
    assert _call(lib, **bad) == _lib.ERR_UNSUPPORTED
    assert _call(lib, Na=0, **bad) == _lib.ERR_UNSUPPORTED     # also when there is nothing to do
    assert _call(lib, b=None, **bad) == _lib.ERR_UNSUPPORTED


def test_small_workspace_and_empty_sides():
    lib = _lib.load()
    need = lib.qsae_nearest_atoms_i8_workspace_bytes(8, 8, 64, 10)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert _call(lib, ws=None) == _lib.ERR_WORKSPACE
    # nothing to do: no pointer is looked at
    assert _call(lib, Na=0, a=None, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _call(lib, Nb=0, a=None, b=0x3004, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _call(lib, Na=0, a=None, b=None, keys=None, dup=None, ws=None, ws_bytes=0, exclude_self=1) == _lib.OK


def test_python_argument_errors():
    a = torch.zeros((4, 64), dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nearest_atoms(a)
    with pytest.raises(TypeError, match="int8"):
        integer_atoms(torch.zeros((4, 64)))
    with pytest.raises(TypeError, match="compare_decoders"):
        integer_atoms(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="different sizes"):
        nearest_atoms(a, torch.zeros((4, 96), dtype=torch.int8))
    with pytest.raises(ValueError, match="self mode"):
        nearest_atoms(a, a.clone(), include_self=False)
    assert integer_atoms(torch.ones((3, 40), dtype=torch.int8)).shape == (3, 64)
    assert int(integer_atoms(torch.ones((3, 40), dtype=torch.int8))[:, 40:].abs().sum()) == 0


# ---- the restatement against real arithmetic -------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", sorted(U.RECIPES))
@pytest.mark.parametrize("D", [64, 512, 4096])
def test_restatement_is_within_1e6_of_fp64(recipe, D):
    """Five roundings of relative size 2^-24 at most (int -> fp32, two inverse norms, their product, the final
    product), |c| <= 1: absolute error <= 3e-7; compared at 1e-6.  Neighbour sets agree wherever the fp64 k-th and
    (k+1)-th cosines are further apart than 2e-6."""
    N, k = 192, 10
    a = U.RECIPES[recipe](7 + D, N, D)
    c64 = U.cosines_f64(a)
    err = float(np.abs(U.cosines(a).astype(np.float64) - c64).max())
    print(f"{recipe} D={D}: max |c - c64| = {err:.3g}")
    assert err <= 1e-6
    sim, idx = U.decode_keys(U.reference_keys(a, None, k))
    assert np.abs(sim.astype(np.float64) - np.take_along_axis(c64, idx, 1)).max() <= 1e-6
    desc = -np.sort(-c64, axis=1)
    clear = desc[:, k - 1] - desc[:, k] > 2e-6
    top = np.argsort(-c64, axis=1, kind="stable")[:, :k]
    assert clear.any()
    for i in np.nonzero(clear)[0]:
        assert set(idx[i].tolist()) == set(top[i].tolist())


def test_restatement_edge_cases():
    a = np.zeros((5, 32), dtype=np.int8)
    a[1, :3] = (1, -1, 1)
    a[3] = a[1]
    a[4, 0] = -128
    sim, idx = U.decode_keys(U.reference_keys(a, None, 7))
    assert idx[0].tolist() == [0, 1, 2, 3, 4, -1, -1] and sim[0, :5].tolist() == [0.0] * 5 and np.isinf(sim[0, 5])
    assert idx[3, :2].tolist() == [1, 3]                       # the duplicate with the lower index comes first
    assert idx[4, 0] == 4 and sim[4, 0] == 1.0
    sim, idx = U.decode_keys(U.reference_keys(a, None, 5, exclude_self=True))
    assert (idx[:, 4] == -1).all() and not (idx == np.arange(5)[:, None]).any()
    assert U.reference_duplicate_of(a).tolist() == [0, 1, 0, 1, 4] and U.n_duplicate_groups(U.reference_duplicate_of(a)) == 2


# ---- against what the reference's inspector recorded -----------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_matches_the_reference_inspector(name):
    g = U.load_golden(name)
    spec = g["meta"]["recipe"]
    a = U.golden_atoms(spec)
    assert np.array_equal(a, g["atoms"])                       # the recipe still gives the atoms the reference saw
    k = g["meta"]["k"]
    sim, idx = U.decode_keys(U.reference_keys(a, None, k))
    share = U.check_against_golden(g, np.maximum(np.float32(1.0) - sim, 0), idx)
    assert share >= 0.9
    dup = U.reference_duplicate_of(a)
    assert U.n_duplicate_groups(dup) == int(g["count_duplicates"])


@pytest.mark.parametrize("name", GOLDENS)
def test_inspector_one_liners_on_cpu_tensors(name):
    g = U.load_golden(name)
    ins = DictionaryInspector(torch.from_numpy(g["atoms"]))
    assert ins.zero_entries() == int(g["zero_entries"])
    assert ins.sparsity_rate() == pytest.approx(float(g["sparsity_rate"]), abs=1e-12)
    assert ins.analyze_ternary_distribution() == dict(zip(g["values"].tolist(), g["value_counts"].tolist()))
    assert torch.equal(ins.get_feature(5), torch.from_numpy(g["atoms"][5]))
    tol = float(g["ref_fp64_maxdev"]) + 3e-7
    for (f1, f2), dc, de in zip(g["meta"]["pairs"], g["pair_cosine"], g["pair_euclidean"]):
        assert abs(float(ins.distance(f1, f2, "cosine")) - dc) <= tol
        assert abs(float(ins.distance(f1, f2, "euclidean")) - de) <= 1e-6
    pos = []
    for s, count in zip(g["meta"]["same"], g["same_count"]):
        c, p = ins.check_same_entries(s)
        assert c == int(count)
        pos.append(p[0].numpy())
    assert np.array_equal(np.concatenate(pos), g["same_pos"])
    assert ins.check_same_entries([3]) == []
    with pytest.raises(ValueError):
        ins.distance(0, 1, "manhattan")
    with pytest.raises(ValueError):
        ins.calculate_k_nearest_features_cluster(5, "manhattan")
    if int(g["zero_entries"]):
        with pytest.raises(ValueError, match="all-zero"):
            ins.calculate_k_nearest_features_cluster(5, "euclidean")
