"""k-means over dictionary atoms without a GPU: qsae_kmeans_assign_f32 and qsae_kmeans_update_f32 are declared, bound
and exported by both libraries and answer every bad argument before any HIP call (the only reason these calls can be
made without a device); the numpy restatement of the arithmetic contract is within its derived bounds
of real arithmetic, its Lloyd loop recovers a planted partition, and its groups and center features equal what the
reference's own ``k_means_analysis`` recorded around a stubbed ``kmeans``."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import kmeans_util as U
import neighbors_f32_util as FU
from quantizedsae_amd import _lib, build
from quantizedsae_amd.inference import DictionaryInspector, kmeans_atoms
from quantizedsae_amd.inference.inspector import _groups_and_center_features

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("qsae_kmeans_assign_f32_workspace_bytes", "qsae_kmeans_assign_f32", "qsae_kmeans_update_f32_workspace_bytes",
         "qsae_kmeans_update_f32")


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "qsae.h").read_text()
    lib = _lib.load()
    assert _lib.DEBUG_LIB_PATH.exists(), "build with `python -m quantizedsae_amd.build`"
    for exported in (build.exported_symbols(_lib.LIB_PATH), build.exported_symbols(_lib.DEBUG_LIB_PATH)):
        for name in NAMES:
            assert re.search(rf"\b{name}\(", header)
            assert name in _lib.SIGNATURES and name in exported
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "kmeans.hip" in build.SOURCES
    assert lib.qsae_abi_version() == _lib.ABI_VERSION == 4     # an additive change
    assert f"kKmeansChunk = {U.KMEANS_CHUNK};" in (ROOT / "quantizedsae_amd" / "csrc" / "kmeans.hip").read_text()


@pytest.mark.parametrize("name", ["qsae_kmeans_assign_f32_workspace_bytes", "qsae_kmeans_update_f32_workspace_bytes"])
def test_workspace_is_monotone_and_zero_for_invalid_shapes(name):
    size = getattr(_lib.load(), name)
    grid = (1, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4500, 32768)
    for fixed in (1, 130, 1025, 32768):
        for D in (4, 64, 512):
            n = [size(v, fixed, D) for v in grid]
            c = [size(fixed, v, D) for v in grid]
            assert n == sorted(n) and c == sorted(c) and n[0] > 0 and c[0] > 0
        ds = [size(fixed, 300, D) for D in range(4, 1100, 4)]
        assert ds == sorted(ds) and ds[0] > 0
    for bad in ((0, 4, 64), (4, 0, 64), (-1, 4, 64), (4, -1, 64), (4, 4, 0), (4, 4, 6), (4, 4, 63), (4, 4, -4)):
        assert size(*bad) == 0, bad


def _assign(lib, *, atoms=0x1000, a_ld=64, N=8, centers=0x3000, c_ld=64, C=3, D=64, metric=0, keys=0x5000, ws=0x6000,
            ws_bytes=1 << 20):
    """Dummy non-null pointers: a call that got as far as a kernel launch would not return an argument error."""
    return lib.qsae_kmeans_assign_f32(atoms, a_ld, N, centers, c_ld, C, D, metric, keys, ws, ws_bytes, None)


def _update(lib, *, atoms=0x1000, a_ld=64, N=8, D=64, labels=0x2000, C=3, old=0x3000, old_ld=64, new=0x4000, new_ld=64,
            counts=0x5000, stats=0x5800, ws=0x6000, ws_bytes=1 << 20):
    return lib.qsae_kmeans_update_f32(atoms, a_ld, N, D, labels, C, old, old_ld, new, new_ld, counts, stats, ws, ws_bytes,
                                      None)


@pytest.mark.parametrize("bad", [
    dict(atoms=None), dict(centers=None), dict(keys=None), dict(N=-1), dict(C=0), dict(C=-1), dict(a_ld=60), dict(c_ld=60),
    dict(a_ld=66), dict(c_ld=66), dict(atoms=0x1004), dict(centers=0x3008), dict(keys=0x5004), dict(ws=0x6004),
    dict(metric=2), dict(metric=-1),
])
def test_assign_refuses_invalid_arguments_before_any_hip_call(bad):
    lib = _lib.load()
    assert _assign(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_kmeans_assign_f32" in lib.qsae_last_error()


@pytest.mark.parametrize("bad", [
    dict(atoms=None), dict(labels=None), dict(old=None), dict(new=None), dict(counts=None), dict(stats=None), dict(N=-1),
    dict(C=0), dict(a_ld=60), dict(old_ld=60), dict(new_ld=60), dict(a_ld=66), dict(old_ld=66), dict(new_ld=66),
    dict(atoms=0x1004), dict(old=0x3008), dict(new=0x4004), dict(labels=0x2002), dict(counts=0x5002), dict(stats=0x5804),
    dict(ws=0x6004),
])
def test_update_refuses_invalid_arguments_before_any_hip_call(bad):
    lib = _lib.load()
    assert _update(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_kmeans_update_f32" in lib.qsae_last_error()


@pytest.mark.parametrize("bad", [dict(D=0), dict(D=-4), dict(D=6), dict(D=63)])
def test_shapes_outside_the_limits_are_unsupported(bad):
    lib = _lib.load()
    for call in (_assign, _update):
        assert call(lib, **bad) == _lib.ERR_UNSUPPORTED
        assert call(lib, N=0, **bad) == _lib.ERR_UNSUPPORTED   # also when there is nothing to do


def test_small_workspace_and_no_atoms():
    lib = _lib.load()
    need = lib.qsae_kmeans_assign_f32_workspace_bytes(8, 3, 64)
    assert need > 0
    assert _assign(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert _assign(lib, ws=None) == _lib.ERR_WORKSPACE
    need = lib.qsae_kmeans_update_f32_workspace_bytes(8, 3, 64)
    assert need > 0
    assert _update(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert _update(lib, ws=None) == _lib.ERR_WORKSPACE
    # nothing to do: no pointer is looked at
    assert _assign(lib, N=0, atoms=None, centers=None, keys=None, ws=None, ws_bytes=0) == _lib.OK
    assert _update(lib, N=0, atoms=None, labels=None, old=None, new=None, counts=None, stats=None, ws=None,
                   ws_bytes=0) == _lib.OK


def test_python_argument_errors():
    f = torch.zeros((6, 64))
    with pytest.raises(ValueError, match="distance must be"):
        kmeans_atoms(f, 2, distance="manhattan")
    with pytest.raises(ValueError, match="init must be"):
        kmeans_atoms(f, 2, init="kmeans++")
    with pytest.raises(ValueError, match="exceeds"):
        kmeans_atoms(f, 7)
    with pytest.raises(ValueError, match="exceeds"):
        kmeans_atoms(f, 7, init_indices=list(range(7)))
    with pytest.raises(ValueError, match="init_indices must be"):
        kmeans_atoms(f, 2, init_indices=[0, 6])
    with pytest.raises(ValueError, match="init_indices must be"):
        kmeans_atoms(f, 2, init_indices=[0, 1, 2])
    with pytest.raises(ValueError, match="init_centers must be"):
        kmeans_atoms(f, 2, init_centers=torch.zeros((2, 32)))
    with pytest.raises(ValueError, match="not both"):
        kmeans_atoms(f, 2, init_centers=torch.zeros((2, 64)), init_indices=[0, 1])
    with pytest.raises(ValueError, match="num_clusters"):
        kmeans_atoms(f, 0)
    with pytest.raises(TypeError, match="fp32 or int8"):
        kmeans_atoms(torch.zeros((6, 64), dtype=torch.float64), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kmeans_atoms(f, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kmeans_atoms(torch.zeros((6, 64), dtype=torch.int8), 2, init_indices=[0, 1])
    with pytest.raises(ValueError, match="type must be"):
        DictionaryInspector(f).k_means_analysis(2, "manhattan")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DictionaryInspector(f).k_means_analysis(2)


# ---- the restatement against real arithmetic -------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", sorted(U.RECIPES))
@pytest.mark.parametrize("D", [64, 512, 4096])
def test_restated_scores_are_within_the_derived_bounds_of_fp64(recipe, D):
    """cosine: |c - c64| <= (D + 5) 2^-24 sum_d |a_d c_d| / (|a| |c|); euclidean: the bound of
    kmeans_util.euclid_f64.  Element by element.  Measured (largest err / bound over the nine cases):
    cosine 0.067, euclidean 0.076, both on the planted atoms at D = 64; the ternary means are dyadic, so the euclidean
    score of ternary atoms is exact)."""
    a = U.RECIPES[recipe](7 + D, 96, D)
    c = U.update(a, np.arange(96) % 12, np.zeros((12, D), np.float32))[0]    # means of 8 atoms each: what centers are
    c64, bound = FU.cosines_f64(a, c)
    err = np.abs(U.scores(a, c, "cosine").astype(np.float64) - c64)
    print(f"cosine {recipe} D={D}: max err {err.max():.3g}, largest err / bound = {(err[bound > 0] / bound[bound > 0]).max():.3g}")
    assert (err <= bound).all()
    s64, bound = U.euclid_f64(a, c)
    err = np.abs(U.scores(a, c, "euclidean").astype(np.float64) - s64)
    print(f"euclidean {recipe} D={D}: max err {err.max():.3g}, largest err / bound = {(err[bound > 0] / bound[bound > 0]).max():.3g}")
    assert (err <= bound).all()
    # the argmax of the euclidean score is the argmin of the squared distance
    d2 = ((a.astype(np.float64)[:, None, :] - c.astype(np.float64)[None, :, :]) ** 2).sum(2) if D <= 512 else None
    if d2 is not None:
        lab = U.labels_of(U.assign_keys(a, c, "euclidean"))
        chosen = d2[np.arange(96), lab]
        assert (chosen - d2.min(1) <= 2 * (bound[np.arange(96), lab] + bound[np.arange(96), d2.argmin(1)])).all()


def test_restatement_edge_cases():
    a = np.zeros((5, 8), dtype=np.float32)
    a[1, :3] = (1, -1, 1)
    a[3] = a[1]
    a[4, 0] = -3
    c = np.stack([a[1], a[1], np.zeros(8, np.float32), a[4]])
    for metric in ("cosine", "euclidean"):
        lab = U.labels_of(U.assign_keys(a, c, metric))
        assert lab[1] == 0 and lab[3] == 0 and lab[4] == 3      # identical centers: the lowest index
    assert U.labels_of(U.assign_keys(a, c, "cosine"))[0] == 0  # a zero atom: cosine +0 with every center -> center 0
    assert U.labels_of(U.assign_keys(a, c, "euclidean"))[0] == 2   # ... and nearest to the zero center
    nan = a.copy()
    nan[2, 0] = np.nan
    assert U.assign_keys(nan, c, "euclidean")[2] == 0 and U.labels_of(U.assign_keys(nan, c, "euclidean"))[2] == -1
    new, counts, stats = U.update(a, np.array([0, 0, 7, -1, 3]), c)
    assert counts.tolist() == [2, 0, 0, 1] and stats[1] == 2
    assert np.array_equal(new[1], c[1]) and np.array_equal(new[2], c[2]) and np.array_equal(new[3], a[4])
    assert np.array_equal(new[0], (a[0] + a[1]) / 2)
    assert stats[0] == pytest.approx(np.sqrt(((new[0] - c[0]).astype(np.float64) ** 2).sum()), rel=1e-15)


def test_lloyd_recovers_planted_clusters():
    a, truth = U.planted(3, 600, 64)
    for metric in ("cosine", "euclidean"):
        r = U.lloyd(a, a[:6], metric, 1e-4, 50)
        assert r["converged"] and r["n_empty"] == 0
        assert np.array_equal(r["labels"], truth)              # init atom c belongs to prototype c: even the names agree
        assert U.same_partition(r["labels"], truth)
        assert r["counts"].tolist() == [100] * 6


# ---- against what the reference's own code recorded ------------------------------------------------------------------
def test_restatement_matches_the_reference_post_processing():
    g = U.load_golden()
    a = U.golden_atoms()
    assert g["meta"]["N"] == U.GOLDEN_N and g["meta"]["C"] == U.GOLDEN_C and g["meta"]["empty"] == U.GOLDEN_EMPTY
    assert np.array_equal(g["atoms"], a.astype(np.int8))
    labels, centers = U.golden_lloyd(a)                        # what the generator supplied is reproducible
    assert np.array_equal(labels, g["labels"]) and np.array_equal(centers, g["centers"])
    assert U.groups(g["labels"], U.GOLDEN_C) == U.golden_groups(g)
    assert U.center_features(a, g["labels"], g["centers"], "cosine") == g["center_features"].tolist()
    assert g["center_features"][U.GOLDEN_EMPTY] == -1 and U.golden_groups(g)[U.GOLDEN_EMPTY] == []
    # the package's own segment reductions (plain torch: they run on any device) give the same, for both expressions
    A, L, Cc = torch.from_numpy(a), torch.from_numpy(g["labels"]), torch.from_numpy(g["centers"])
    groups, feats = _groups_and_center_features(A, L, Cc, "cosine")
    assert groups == U.golden_groups(g) and feats == g["center_features"].tolist()
    groups, feats = _groups_and_center_features(A, L, Cc, "euclidean")
    assert groups == U.golden_groups(g) and feats == U.center_features(a, g["labels"], g["centers"], "euclidean")
    skipped = g["labels"].copy()
    skipped[[0, 17]] = -1                                      # an atom without a cluster is in no group
    groups, feats = _groups_and_center_features(A, torch.from_numpy(skipped), Cc, "cosine")
    assert groups == U.groups(skipped, U.GOLDEN_C) and feats == U.center_features(a, skipped, g["centers"], "cosine")
