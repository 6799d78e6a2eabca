"""k-means over dictionary atoms on the GPU: qsae_kmeans_assign_f32 and qsae_kmeans_update_f32 equal the numpy restatement
of the arithmetic contract bit for bit -- on every edge of the tiling (128 atoms, 128 centers per tile),
with one and several center splits, with both loaders (D % 32 == 0 and the K tail), on zero atoms, a zero center and
identical centers, with strides wider than D and guards around every output; the whole loop of ``kmeans_atoms`` equals
the restatement's Lloyd run iteration by iteration; ``DictionaryInspector.k_means_analysis`` reproduces what the
reference's own post-processing recorded; and at the registry shape every atom's chosen center is within the derived
error bounds of the fp64 best."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dictionary_neighbors_util as NU
import kmeans_util as U
import quantizedsae_amd as Q
from quantizedsae_amd import _lib, ops
from quantizedsae_amd import torch_ops as T
from quantizedsae_amd.inference import DictionaryInspector, kmeans_atoms
from quantizedsae_amd.inference.inspector import _groups_and_center_features

pytestmark = pytest.mark.gpu
DEV = "cuda"
METRICS = ("cosine", "euclidean")
GUARD = 4096

# (N, C, D): every N in {1, 127, 128, 129, 257}, C in {1, 2, 16, 127, 128, 129, 300}, D in {4, 36, 64, 512} at least
# twice; C > 128 splits the centers over two or three workgroups per atom panel (atomicMax join); D in {4, 36} takes the
# K-tail loader, D in {64, 512} the asm-staged one
SHAPES = [(1, 1, 4), (1, 300, 36), (1, 129, 64), (127, 2, 64), (127, 128, 512), (128, 16, 512), (128, 300, 64),
          (128, 127, 4), (129, 127, 36), (129, 1, 64), (129, 2, 512), (257, 128, 64), (257, 129, 4), (257, 16, 36),
          (257, 300, 512), (127, 129, 36)]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the cached cases are read-only


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(N, Cn, D):
    """Gaussian atoms and centers with the hazards planted where the shape has room: a zero atom, a zero center, and the
    last center a copy of center 2 (equal bits: the lower index must win)."""
    a = U.gaussian(100 + N + D, N, D).copy()
    c = U.gaussian(200 + Cn + D, Cn, D).copy()
    if N >= 3:
        a[N // 2] = 0
    if Cn >= 4:
        c[1] = 0
        c[Cn - 1] = c[2]
    a.setflags(write=False)
    c.setflags(write=False)
    return a, c


@functools.lru_cache(maxsize=None)
def _expected(N, Cn, D, metric):
    a, c = _case(N, Cn, D)
    return U.assign_keys(a, c, metric)


def _wide(x, pad):
    """x in the leading columns of a wider tensor, NaN behind them."""
    w = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV)
    w[:, :x.shape[1]] = dev(x)
    return w


def _raw_assign(wa, wc, N, Cn, D, metric):
    """The C entry point on strided rows, with guards around keys and workspace -> keys [N] (numpy)."""
    lib = _lib.load()
    need = int(lib.qsae_kmeans_assign_f32_workspace_bytes(N, Cn, D))
    ws = torch.full((GUARD + need + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    kbuf = torch.full((512 + N + 512,), -7, dtype=torch.int64, device=DEV)
    assert (ws.data_ptr() + GUARD) % 16 == 0
    _lib.check(lib.qsae_kmeans_assign_f32(wa.data_ptr(), wa.stride(0), N, wc.data_ptr(), wc.stride(0), Cn, D,
                                          U.METRICS[metric], kbuf.data_ptr() + 8 * 512, ws.data_ptr() + GUARD, need, _stream()))
    torch.cuda.synchronize()
    assert (kbuf[:512] == -7).all() and (kbuf[512 + N:] == -7).all()
    assert (ws[:GUARD] == 0x5A).all() and (ws[GUARD + need:] == 0x5A).all()
    return kbuf[512:512 + N].cpu().numpy()


# ---- assign ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N,Cn,D", SHAPES)
def test_assign_equals_the_restatement(N, Cn, D, metric):
    a, c = _case(N, Cn, D)
    expect = _expected(N, Cn, D, metric)
    wa, wc = _wide(a, 12), _wide(c, 3 * D)                     # strides wider than D, NaN past D
    assert np.array_equal(_raw_assign(wa, wc, N, Cn, D, metric), expect)
    va, vc = wa[:, :D], wc[:, :D]
    assert ops._atoms_f32(va, "atoms").data_ptr() == wa.data_ptr()      # a column slice is read in place
    k1, k2 = ops.kmeans_assign(va, vc, metric), ops.kmeans_assign(va, vc, metric)
    assert np.array_equal(k1.cpu().numpy(), expect) and torch.equal(k1, k2)      # the same bits every call
    assert np.array_equal(ops.kmeans_assign(dev(a), dev(c), metric).cpu().numpy(), expect)
    labels = U.labels_of(expect)
    assert labels.min() >= 0 and labels.max() < Cn
    if Cn >= 4:
        assert not (labels == Cn - 1).any()                    # a copy of center 2: the lower index wins
    if metric == "cosine":
        assert torch.equal(k1, ops.nearest_atoms_f32(va, vc, 1)[:, 0])   # the second witness
        if N >= 3:
            assert labels[N // 2] == 0                         # a zero atom: cosine +0 with every center
    elif N >= 3 and Cn >= 4:
        assert labels[N // 2] == 1                             # a zero atom is nearest to the zero center


def test_assign_with_nan_atoms_stays_in_range():
    a, c = (x.copy() for x in _case(257, 129, 36))
    a[[0, 128, 256], 5] = np.nan
    for metric in METRICS:
        keys = _raw_assign(_wide(a, 4), _wide(c, 4), 257, 129, 36, metric)      # guards checked inside
        ok = np.ones(257, bool)
        ok[[0, 128, 256]] = False
        assert np.array_equal(keys[ok], _expected(257, 129, 36, metric)[ok])
        assert (keys[~ok] == 0).all()                          # every score NaN: no candidate


def test_assign_argument_errors_on_the_device():
    a = torch.zeros((4, 64), device=DEV)
    with pytest.raises(ValueError, match="metric"):
        ops.kmeans_assign(a, a, "manhattan")
    with pytest.raises(ValueError, match="same D"):
        ops.kmeans_assign(a, torch.zeros((2, 32), device=DEV))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.kmeans_assign(a[:, :38].contiguous(), a[:, :38].contiguous())
    with pytest.raises(ValueError, match="at least one"):
        ops.kmeans_assign(a, torch.zeros((0, 64), device=DEV))
    with pytest.raises(ValueError, match="different devices"):
        ops.kmeans_assign(a, torch.zeros((2, 64)))
    with pytest.raises(ValueError, match="labels"):
        ops.kmeans_update(a, torch.zeros((3,), dtype=torch.int64, device=DEV), a)
    assert ops.kmeans_assign(torch.zeros((0, 64), device=DEV), a).shape == (0,)
    new, counts, stats = ops.kmeans_update(torch.zeros((0, 64), device=DEV), torch.zeros((0,), dtype=torch.int32, device=DEV), a)
    assert torch.equal(new, a) and counts.tolist() == [0] * 4 and stats.tolist() == [0.0, 4.0]
    for kw in (dict(distance="manhattan"), dict(init_centers=torch.zeros((2, 32), device=DEV)),
               dict(init_centers=torch.zeros((2, 64)))):
        with pytest.raises(ValueError):
            kmeans_atoms(a, 2, **kw)
    with pytest.raises(ValueError, match="exceeds"):
        kmeans_atoms(a, 5)


# ---- update ----------------------------------------------------------------------------------------------------------
def _raw_update(a, labels, old, pad):
    """The C entry point with every row stride wider than D and guards around every output
    -> (centers [C, D], counts, stats) as numpy."""
    (N, D), Cn = a.shape, old.shape[0]
    lib = _lib.load()
    need = int(lib.qsae_kmeans_update_f32_workspace_bytes(N, Cn, D))
    ws = torch.full((GUARD + need + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    wa, wo = _wide(a, pad), _wide(old, pad + 4)
    new = torch.full((64 + Cn * (D + pad) + 64,), -7.0, device=DEV)
    counts = torch.full((64 + Cn + 64,), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((8 + 2 + 8,), -7.0, dtype=torch.float64, device=DEV)
    lab = dev(labels.astype(np.int32))
    _lib.check(lib.qsae_kmeans_update_f32(wa.data_ptr(), wa.stride(0), N, D, lab.data_ptr(), Cn, wo.data_ptr(), wo.stride(0),
                                          new.data_ptr() + 4 * 64, D + pad, counts.data_ptr() + 4 * 64,
                                          stats.data_ptr() + 8 * 8, ws.data_ptr() + GUARD, need, _stream()))
    torch.cuda.synchronize()
    assert (ws[:GUARD] == 0x5A).all() and (ws[GUARD + need:] == 0x5A).all()
    assert (new[:64] == -7).all() and (new[64 + Cn * (D + pad):] == -7).all()
    assert (counts[:64] == -7).all() and (counts[64 + Cn:] == -7).all()
    assert (stats[:8] == -7).all() and (stats[10:] == -7).all()
    rows = new[64:64 + Cn * (D + pad)].view(Cn, D + pad)
    assert (rows[:, D:] == -7).all()                           # floats of a row at or past D are not written
    return rows[:, :D].cpu().numpy(), counts[64:64 + Cn].cpu().numpy(), stats[8:10].cpu().numpy()


def _labels(seed, N, hi, lo=0):
    return (np.floor(U.S.uniform01(seed, N, stream=47) * (hi - lo)) + lo).astype(np.int32)


UPDATES = {
    # all 1000 atoms in one cluster: 16 chunks of one cluster, the other two clusters empty
    "one_cluster_n1000": lambda: (U.gaussian(1, 1000, 36), np.ones(1000, np.int32), U.gaussian(2, 3, 36), 4),
    # every cluster a single member: a permutation of 4096
    "permutation_4096": lambda: (U.gaussian(3, 4096, 4), np.argsort(U.S.uniform01(4, 4096, stream=47)).astype(np.int32),
                                 U.gaussian(5, 4096, 4), 4),
    # labels in [-2, 9) with C = 7: -2, -1, 7 and 8 are skipped; cluster 3 is emptied
    "skipped_labels_and_an_empty_cluster_d512": lambda: (
        U.gaussian(6, 700, 512), np.where(_labels(7, 700, 9, -2) == 3, 4, _labels(7, 700, 9, -2)), U.gaussian(8, 7, 512), 8),
    "n1_d4": lambda: (U.gaussian(9, 1, 4), np.array([1], np.int32), U.gaussian(10, 2, 4), 4),
    "uneven_clusters_d36": lambda: (U.gaussian(11, 1500, 36), (_labels(12, 1500, 40) ** 2 // 70).astype(np.int32),
                                    U.gaussian(13, 23, 36), 12),
    "two_slabs_d512": lambda: (U.gaussian(14, 300, 512), _labels(15, 300, 5), U.gaussian(16, 5, 512), 0),
}


@pytest.mark.parametrize("case", sorted(UPDATES))
def test_update_equals_the_restatement(case):
    a, labels, old, pad = UPDATES[case]()
    new, counts, stats = _raw_update(a, labels, old, pad)
    rnew, rcounts, rstats = U.update(a, labels, old)
    assert np.array_equal(counts, rcounts)
    assert np.array_equal(new.view(np.int32), rnew.view(np.int32))
    assert stats[1] == rstats[1]
    assert abs(stats[0] - rstats[0]) <= 1e-12 * rstats[0]
    empty = rcounts == 0
    assert np.array_equal(new[empty], old[empty])              # an empty cluster keeps its center
    if case.startswith("one_cluster"):
        assert counts.tolist() == [0, 1000, 0] and stats[1] == 2
    if case.startswith("skipped"):
        assert counts[3] == 0 and counts.sum() < 700
    # through ops (contiguous outputs, int64 labels), twice: the same bits
    r1 = ops.kmeans_update(dev(a), dev(labels.astype(np.int64)), dev(old))
    r2 = ops.kmeans_update(dev(a), dev(labels.astype(np.int32)), dev(old))
    assert np.array_equal(r1[0].cpu().numpy().view(np.int32), rnew.view(np.int32))
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    assert r1[1].dtype == torch.int32 and r1[2].dtype == torch.float64


# ---- the whole loop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_atoms_recovers_planted_clusters(metric):
    a, truth = U.planted(3, 600, 64)
    res = kmeans_atoms(dev(a), 6, distance=metric, init_indices=list(range(6)))
    assert res["converged"] and res["n_empty"] == 0 and res["center_shift"] ** 2 < 1e-4
    assert np.array_equal(res["labels"].cpu().numpy(), truth)
    assert res["labels"].dtype == torch.int64 and res["centers"].shape == (6, 64) and res["score"].dtype == torch.float32
    assert res["counts"].tolist() == [100] * 6
    ref = U.lloyd(a, a[:6], metric)
    assert res["n_iter"] == ref["n_iter"]
    assert np.array_equal(res["centers"].cpu().numpy().view(np.int32), ref["centers"].view(np.int32))
    c64 = ref["centers"].astype(np.float64)[truth]
    if metric == "euclidean":
        inertia = ((a.astype(np.float64) - c64) ** 2).sum()
    else:
        inertia = (1.0 - U.decode_keys(ref["keys"])[0].astype(np.float64)).sum()
    assert res["inertia"] == pytest.approx(inertia, rel=1e-9)


@pytest.mark.parametrize("metric", METRICS)
def test_every_iteration_equals_the_restatements_lloyd_run(metric):
    N, D, Cn, cap = 700, 36, 9, 12
    a = U.gaussian(21, N, D)
    init = list(range(0, 9 * 70, 70))
    ref = U.lloyd(a, a[init], metric, 1e-4, cap)
    A = dev(a)
    for m in range(1, ref["n_iter"] + 1):
        res = kmeans_atoms(A, Cn, distance=metric, init_indices=init, max_iter=m)
        assert res["n_iter"] == m
        # the labels after m updates are the labels iteration m + 1 starts from
        expect = ref["history"][m] if m < ref["n_iter"] else ref["labels"]
        assert np.array_equal(res["labels"].cpu().numpy(), expect), m
        assert np.array_equal(res["centers"].cpu().numpy().view(np.int32), ref["centers_history"][m - 1].view(np.int32)), m
    assert res["converged"] == ref["converged"] and res["center_shift"] == pytest.approx(ref["center_shift"], rel=1e-12)
    assert np.array_equal(res["score"].cpu().numpy(), U.decode_keys(ref["keys"])[0])
    # init_centers instead of indices, D not a multiple of 4 (zero-padded inside), check_every > 1
    res2 = kmeans_atoms(A[:, :34], Cn, distance=metric, init_centers=A[init, :34], max_iter=4, check_every=3, tol=0.0)
    ref2 = U.lloyd(a[:, :34], a[init, :34], metric, 0.0, 4)
    assert res2["centers"].shape == (Cn, 34) and np.array_equal(res2["labels"].cpu().numpy(), ref2["labels"])


def test_the_same_seed_gives_the_same_result():
    A = dev(U.gaussian(22, 700, 36))
    r1 = kmeans_atoms(A, 9, seed=5, max_iter=6)
    r2 = kmeans_atoms(A, 9, seed=5, max_iter=6)
    r3 = kmeans_atoms(A, 9, seed=6, max_iter=6)
    assert torch.equal(r1["labels"], r2["labels"]) and torch.equal(r1["centers"], r2["centers"])
    assert r1["inertia"] == r2["inertia"] and not torch.equal(r1["centers"], r3["centers"])
    gen = torch.Generator().manual_seed(5)
    ref = U.lloyd(A.cpu().numpy(), A.cpu().numpy()[torch.randperm(700, generator=gen)[:9].numpy()], "cosine", 1e-4, 6)
    assert np.array_equal(r1["labels"].cpu().numpy(), ref["labels"])


@pytest.mark.parametrize("variant", ["ternary", "binary"])
@pytest.mark.parametrize("type", METRICS)
def test_inspector_k_means_analysis(variant, type):
    model = NU.golden_model(Q, {"variant": variant, "seed": 71}, 64, 256).to(DEV)
    ins = DictionaryInspector(model)
    ids, centers, groups, center_features = ins.k_means_analysis(8, type, seed=3, max_iter=20)
    assert isinstance(ids, torch.Tensor) and ids.dtype == torch.int64 and ids.shape == (256,)
    assert isinstance(centers, torch.Tensor) and centers.dtype == torch.float32 and centers.shape == (8, 64)
    assert isinstance(groups, list) and len(groups) == 8 and isinstance(center_features, list) and len(center_features) == 8
    assert sorted(i for g in groups for i in g) == list(range(256)) and all(g == sorted(g) for g in groups)
    a = ins.atoms.float().cpu().numpy()
    labels = ids.cpu().numpy()
    assert groups == U.groups(labels, 8)
    assert center_features == U.center_features(a, labels, centers.cpu().numpy(), type)
    assert all((f in g) if g else f == -1 for f, g in zip(center_features, groups))


def test_golden_fixture_is_reproduced_from_its_labels_and_centers():
    g = U.load_golden()
    groups, center_features = _groups_and_center_features(dev(g["atoms"].astype(np.float32)), dev(g["labels"]),
                                                          dev(g["centers"]), "cosine")
    assert groups == U.golden_groups(g)
    assert center_features == g["center_features"].tolist()
    # and one update from the recorded labels gives the recorded centers (the empty cluster keeps its zero center)
    a = g["atoms"].astype(np.float32)
    new = ops.kmeans_update(dev(a), dev(g["labels"]), dev(g["centers"]))[0].cpu().numpy()
    assert np.array_equal(new, U.update(a, g["labels"], g["centers"])[0])


def test_torch_ops_pass_opcheck_and_equal_ops():
    a, c = _case(257, 129, 36)
    A, Cd = dev(a), dev(c)
    for metric in METRICS:
        keys = torch.ops.qsae.kmeans_assign(A, Cd, metric)
        assert torch.equal(keys, ops.kmeans_assign(A, Cd, metric)) and torch.equal(keys, T.kmeans_assign(A, Cd, metric))
        torch.library.opcheck(torch.ops.qsae.kmeans_assign.default, (A, Cd, metric))
    labels = dev(U.labels_of(_expected(257, 129, 36, "cosine")))
    out = torch.ops.qsae.kmeans_update(A, labels, Cd)
    assert all(torch.equal(x, y) for x, y in zip(out, ops.kmeans_update(A, labels, Cd)))
    assert all(torch.equal(x, y) for x, y in zip(out, T.kmeans_update(A, labels, Cd)))
    torch.library.opcheck(torch.ops.qsae.kmeans_update.default, (A, labels, Cd))


# ---- the registry shape ----------------------------------------------------------------------------------------------
def test_registry_shape_against_fp64_on_the_device():
    """No atom is excused: the fp64 score of the chosen center is no further below the fp64 best than the sum of the two
    pairs' error bounds (cosine: DESIGN.md 4.19's bound; euclidean: 4.20's)."""
    N, D, Cn = 32768, 512, 4096
    gen = torch.Generator(device=DEV).manual_seed(78)
    A = torch.randn((N, D), device=DEV, generator=gen)
    Cd = A[torch.randperm(N, device=DEV, generator=gen)[:Cn]] + 0.5 * torch.randn((Cn, D), device=DEV, generator=gen)
    u = 2.0 ** -24
    A64, C64 = A.double(), Cd.double()
    na, nc = torch.linalg.norm(A64, dim=1), torch.linalg.norm(C64, dim=1)
    H = 0.5 * (C64 * C64).sum(1)
    labels = {}
    for metric in METRICS:
        keys = ops.kmeans_assign(A, Cd, metric)
        lab = (0xFFFFFFFF - (keys & 0xFFFFFFFF))
        assert (keys != 0).all() and int(lab.max()) < Cn
        labels[metric] = lab
        worst = 0.0
        for r0 in range(0, N, 4096):
            rows = slice(r0, r0 + 4096)
            dot, absdot = A64[rows] @ C64.t(), A64[rows].abs() @ C64.abs().t()
            if metric == "cosine":
                den = na[rows, None] * nc[None, :]
                s64, bound = dot / den, (D + 5) * u * absdot / den
            else:
                e_chain = D * u / (1.0 - D * u) * absdot
                e_h = (u + D * 2.0 ** -52) * H[None, :]
                s64, bound = dot - H[None, :], e_chain + e_h + u * (dot.abs() + e_chain + H[None, :] + e_h)
            best, arg = s64.max(1)
            chosen = lab[rows, None]
            short = best - torch.gather(s64, 1, chosen)[:, 0]
            allowed = torch.gather(bound, 1, chosen)[:, 0] + torch.gather(bound, 1, arg[:, None])[:, 0]
            assert (short <= allowed).all(), metric
            worst = max(worst, float((short / allowed).max()))
        print(f"registry shape, {metric}: largest shortfall / allowed = {worst:.3g}")
    lab = labels["cosine"]
    new, counts, stats = ops.kmeans_update(A, lab, Cd)
    assert torch.equal(counts.long(), torch.bincount(lab, minlength=Cn))
    sum64 = torch.zeros((Cn, D), dtype=torch.float64, device=DEV).index_add_(0, lab, A64)
    abs64 = torch.zeros((Cn, D), dtype=torch.float64, device=DEV).index_add_(0, lab, A64.abs())
    n = counts.double().clamp(min=1)[:, None]
    mean64 = torch.where(counts[:, None] > 0, sum64 / n, C64)
    # fp32 rounding of the mean (relative 2^-23), plus the two fp64 sums' own error (at most n 2^-53 sum |x| each)
    tol = 2.0 ** -23 * mean64.abs() + 2.0 ** -52 * abs64
    assert ((new.double() - mean64).abs() <= tol).all()
    assert int(stats[1]) == int((counts == 0).sum())
    shift = torch.linalg.norm(new.double() - C64, dim=1).sum()
    assert abs(float(stats[0]) - float(shift)) <= 1e-9 * float(shift)
