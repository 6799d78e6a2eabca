"""The fp32 nearest-atom query without a GPU: qsae_nearest_atoms_f32 is declared, bound and exported and answers every
bad argument before any HIP call (the only reason these calls can be made without a device); the numpy restatement of
the arithmetic contract is within its derived bound of real arithmetic, equals the int8 path's
restatement on integer-valued atoms, and agrees with what the reference's decoder comparison followed by torch.topk
recorded."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import dictionary_neighbors_util as NU
import neighbors_f32_util as U
from quantizedsae_amd import _lib, build, ops
from quantizedsae_amd.inference import DictionaryInspector, integer_atoms, nearest_atoms

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("qsae_nearest_atoms_f32_workspace_bytes", "qsae_nearest_atoms_f32")
GOLDENS = sorted(U.GOLDEN_CASES)


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "qsae.h").read_text()
    exported = build.exported_symbols(_lib.LIB_PATH)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header)
        assert name in _lib.SIGNATURES and name in exported
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "dictionary_neighbors_f32.hip" in build.SOURCES
    assert lib.qsae_abi_version() == _lib.ABI_VERSION == 4     # an additive change


def test_workspace_is_monotone_and_zero_for_invalid_shapes():
    size = _lib.load().qsae_nearest_atoms_f32_workspace_bytes
    grid = (1, 5, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4500, 32768)
    for fixed in (1, 130, 1025, 32768):
        for k in (1, 10, 64):
            a = [size(v, fixed, 64, k) for v in grid]
            b = [size(fixed, v, 64, k) for v in grid]
            assert a == sorted(a) and b == sorted(b) and a[0] > 0 and b[0] > 0
        ks = [size(fixed, fixed, 64, k) for k in range(1, 65)]
        assert ks == sorted(ks) and ks[0] > 0
    assert size(300, 200, 4, 10) == size(300, 200, 4096, 10)       # rows are read in place: D costs nothing
    for bad in ((0, 4, 64, 10), (4, 0, 64, 10), (-1, 4, 64, 10), (4, -1, 64, 10), (4, 4, 0, 10), (4, 4, 6, 10),
                (4, 4, 63, 10), (4, 4, 64, 0), (4, 4, 64, 65), (4, 4, -4, 10)):
        assert size(*bad) == 0, bad


def _call(lib, *, a=0x1000, a_ld=64, Na=8, b=0x3000, b_ld=64, Nb=8, D=64, k=10, exclude_self=0, keys=0x5000, ws=0x6000,
          ws_bytes=1 << 20):
    """Dummy non-null pointers: a call that got as far as a kernel launch would not return an argument error."""
    return lib.qsae_nearest_atoms_f32(a, a_ld, Na, b, b_ld, Nb, D, k, exclude_self, keys, ws, ws_bytes, None)


@pytest.mark.parametrize("bad", [
    dict(a=None), dict(keys=None), dict(Na=-1), dict(Nb=-1), dict(a_ld=60), dict(b_ld=60), dict(a_ld=66), dict(b_ld=66),
    dict(a=0x1004), dict(b=0x3008), dict(ws=0x6004), dict(exclude_self=1),
    dict(b=None, a_ld=66), dict(b=None, a=0x1004), dict(b=None, Na=-1),
])
def test_invalid_arguments_are_refused_before_any_hip_call(bad):
    lib = _lib.load()
    assert _call(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_nearest_atoms_f32" in lib.qsae_last_error()


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=65), dict(k=-1), dict(D=0), dict(D=-4), dict(D=6), dict(D=63)])
def test_shapes_outside_the_limits_are_unsupported(bad):
    lib = _lib.load()
    assert _call(lib, **bad) == _lib.ERR_UNSUPPORTED
    assert _call(lib, Na=0, **bad) == _lib.ERR_UNSUPPORTED     # also when there is nothing to do
    assert _call(lib, b=None, **bad) == _lib.ERR_UNSUPPORTED


def test_small_workspace_and_empty_sides():
    lib = _lib.load()
    need = lib.qsae_nearest_atoms_f32_workspace_bytes(8, 8, 64, 10)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert _call(lib, ws=None) == _lib.ERR_WORKSPACE
    # nothing to do: no pointer is looked at
    assert _call(lib, Na=0, a=None, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _call(lib, Nb=0, a=None, b=0x3004, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _call(lib, Na=0, a=None, b=None, keys=None, ws=None, ws_bytes=0, exclude_self=1) == _lib.OK


def test_python_argument_errors():
    f = torch.zeros((4, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nearest_atoms_f32(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nearest_atoms(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nearest_atoms(torch.zeros((4, 64), dtype=torch.int8), f)   # a mixed pair goes through fp32
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nearest_atoms(torch.zeros((4, 64), dtype=torch.int8), atoms="fp32")
    with pytest.raises(ValueError, match="different sizes"):
        nearest_atoms(f, torch.zeros((4, 96)))
    with pytest.raises(ValueError, match="self mode"):
        nearest_atoms(f, f.clone(), include_self=False)
    with pytest.raises(ValueError, match="atoms must be"):
        nearest_atoms(f, atoms="int8")
    with pytest.raises(TypeError, match="fp32 or int8"):
        nearest_atoms(torch.zeros((4, 64), dtype=torch.float64))
    with pytest.raises(TypeError, match="fp32 or int8"):
        nearest_atoms(torch.zeros((64,)))
    ins = DictionaryInspector(torch.ones((3, 40)))
    assert ins.atoms.dtype == torch.float32 and ins.atoms.shape == (3, 40)
    with pytest.raises(TypeError, match="fp32"):
        ins.analyze_ternary_distribution()
    # the int8 route is what it was: every assertion of the int8 host test's test_python_argument_errors
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


def test_inspector_one_liners_on_fp32_cpu_tensors():
    a = U.baseline_like(9, 40, 12).copy()
    a[7] = 0.0
    a[30] = a[3]
    a[31] = a[3]
    a[33] = a[5]
    ins = DictionaryInspector(torch.from_numpy(a))
    assert ins.zero_entries() == 1
    assert ins.count_duplicates() == 2
    assert ins.sparsity_rate() == pytest.approx(float((a == 0).sum()) / a.size, abs=1e-12)
    assert torch.equal(ins.get_feature(5), torch.from_numpy(a[5]))
    c64, _ = U.cosines_f64(a)
    assert abs(float(ins.distance(1, 2)) - (1 - c64[1, 2])) <= 1e-6
    assert float(ins.distance(3, 30, "euclidean")) <= 1e-6
    count, pos = ins.check_same_entries([3, 30, 31])
    assert count == 12 and pos[0].tolist() == list(range(12))
    with pytest.raises(ValueError, match="all-zero"):
        ins.calculate_k_nearest_features_cluster(5, "euclidean")


# ---- the restatement against real arithmetic -------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", sorted(U.RECIPES))
@pytest.mark.parametrize("D", [64, 512, 4096])
def test_restatement_is_within_the_derived_bound_of_fp64(recipe, D):
    """|c - c64| <= (D + 5) * 2^-24 * sum_d |a_d b_d| / (|a| |b|): the forward error of a D-term fma chain plus the five
    roundings of the scaling."""
    a = U.RECIPES[recipe](7 + D, 96, D)
    c64, bound = U.cosines_f64(a)
    err = np.abs(U.cosines(a).astype(np.float64) - c64)
    ratio = (err[bound > 0] / bound[bound > 0]).max()
    print(f"{recipe} D={D}: max |c - c64| = {err.max():.3g}, max of the bound = {bound.max():.3g}, "
          f"largest err / bound = {ratio:.3g}")
    assert (err <= bound).all()


def test_inverse_norms_follow_the_kernels_order():
    a = U.gaussian(3, 50, 200)
    a[4] = 0.0
    inv = U.inv_norms(a)
    assert inv.dtype == np.float32 and inv[4] == np.float32(1e12)
    exact = 1.0 / np.sqrt((a.astype(np.float64) ** 2).sum(1)[np.arange(50) != 4])
    assert np.abs(inv[np.arange(50) != 4] / exact - 1).max() <= 2.0 ** -24 + 1e-12
    c = U.cosines(a)
    assert not c[4].any() and not np.signbit(c[4]).any()      # an all-zero atom: +0 with everything, itself included
    assert np.array_equal(c, c.T)                              # the norms first: c(i, j) and c(j, i) are the same bits


# ---- the restatement against the int8 path ---------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,D", [("ternary", 64), ("nbit4", 96), ("int8", 64), ("nbit4", 4096)])
def test_integer_valued_atoms_give_the_int8_paths_keys(recipe, D):
    """Dots below 2^24 are exact in the chain, and both inverse norms are fp32(1 / sqrt(exact fp64 sum of squares)) --
    the zero atoms too: 0 * anything finite is +0 on both paths."""
    a = NU.RECIPES[recipe](11, 150, D).copy()
    b = NU.RECIPES[recipe](12, 70, D).copy()
    a[[3, 77]] = 0
    b[5] = 0
    for k in (1, 10, 64):
        assert np.array_equal(U.reference_keys(a.astype(np.float32), None, k), NU.reference_keys(a, None, k))
        assert np.array_equal(U.reference_keys(a.astype(np.float32), None, k, True), NU.reference_keys(a, None, k, True))
        assert np.array_equal(U.reference_keys(a.astype(np.float32), b.astype(np.float32), k), NU.reference_keys(a, b, k))


def test_restatement_edge_cases():
    a = np.zeros((5, 8), dtype=np.float32)
    a[1, :3] = (1, -1, 1)
    a[3] = a[1]
    a[4, 0] = -128
    sim, idx = U.decode_keys(U.reference_keys(a, None, 7))
    assert idx[0].tolist() == [0, 1, 2, 3, 4, -1, -1] and sim[0, :5].tolist() == [0.0] * 5 and np.isinf(sim[0, 5])
    assert idx[3, :2].tolist() == [1, 3]                       # equal bits: the lower index comes first
    assert idx[4, 0] == 4 and sim[4, 0] == 1.0
    sim, idx = U.decode_keys(U.reference_keys(a, None, 5, exclude_self=True))
    assert (idx[:, 4] == -1).all() and not (idx == np.arange(5)[:, None]).any()


# ---- against what the reference's comparison and torch.topk recorded -------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_matches_the_reference(name):
    g = U.load_golden(name)
    case = U.GOLDEN_CASES[name]
    assert g["meta"]["lhs"] == case["lhs"] and g["meta"]["rhs"] == case["rhs"]
    a, b = U.golden_atoms(case)
    k = g["meta"]["k"]
    sim, idx = U.decode_keys(U.reference_keys(a, b, k))
    share = U.check_against_golden(g, sim, idx)
    print(f"{name}: {share:.1%} of the rows compared by index")
    assert share >= 0.9
