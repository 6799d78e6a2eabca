"""qsae_nearest_atoms_i8 on the GPU: the keys equal the numpy restatement of the arithmetic contract
bit for bit -- on every edge of the tiling (128 rows, 256 columns) and of the column split (up to 8 workgroups per row
panel; above 2048 columns a workgroup takes more than one tile), on dictionaries built to make every product pass the
filter, and through DictionaryInspector against what the reference's own inspector class recorded."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dictionary_neighbors_util as U
from quantizedsae_amd import _lib, ops
from quantizedsae_amd import torch_ops as T
from quantizedsae_amd.inference import DictionaryInspector, integer_atoms, nearest_atoms

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, None, 32), (5, 3, 32), (33, 65, 64), (129, None, 96), (257, 130, 512), (300, 520, 64), (520, None, 4096),
          (2100, None, 64)]
# edges of the 128-row panel, the 256-column tile and the split (8 x 256 columns: one tile each; one more: two each)
EDGES = [(n, None, 32) for n in (127, 128, 255, 256, 257, 2047, 2048, 2049)] + \
        [(127, 255, 32), (128, 256, 32), (129, 257, 32), (3, 2049, 32), (2049, 3, 32), (1025, 2304, 32)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=4)
def _atoms(recipe, N, D, seed):
    return U.RECIPES[recipe](seed, N, D)


def _pair(recipe, Na, Nb, D):
    a = _atoms(recipe, Na, D, 100 + D)
    b = None if Nb is None else _atoms(recipe, Nb, D, 200 + D)
    return a, b


def _keys(a, b=None, k=10, exclude_self=False, want_duplicates=False):
    keys, dup = ops.nearest_atoms_i8(dev(a), None if b is None else dev(b), k, exclude_self, want_duplicates)
    return keys.cpu().numpy(), (None if dup is None else dup.cpu().numpy())


@pytest.mark.parametrize("recipe", sorted(U.RECIPES))
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("shape", SHAPES + EDGES, ids=lambda s: "x".join("self" if v is None else str(v) for v in s))
def test_keys_equal_the_restatement(shape, k, recipe):
    Na, Nb, D = shape
    a, b = _pair(recipe, Na, Nb, D)
    keys, dup = _keys(a, b, k, want_duplicates=b is None)
    assert np.array_equal(keys, U.reference_keys(a, b, k))
    if b is None:
        assert np.array_equal(dup, U.reference_duplicate_of(a))
        keys, _ = _keys(a, None, k, exclude_self=True)
        assert np.array_equal(keys, U.reference_keys(a, None, k, exclude_self=True))
    else:
        keys, _ = _keys(b, a, k)                             # the swapped problem
        assert np.array_equal(keys, U.reference_keys(b, a, k))


# ---- dictionaries built against the filter and the buffers -----------------------------------------------------------
def test_nested_atoms_every_product_passes_the_filter():
    N, D = 300, 320
    a = (np.arange(D)[None, :] <= np.arange(N)[:, None]).astype(np.int8)      # atom j: ones in dimensions 0..j
    for k in (1, 10, 64):
        keys, dup = _keys(a, None, k, want_duplicates=True)
        assert np.array_equal(keys, U.reference_keys(a, None, k))
        assert np.array_equal(dup, np.arange(N))
    _, idx = U.decode_keys(_keys(a, None, 10)[0])
    assert idx[-1].tolist() == list(range(299, 289, -1))


def test_identical_atoms():
    N = 300
    a = np.repeat(U.ternary(3, 1, 64), N, axis=0)
    for k in (1, 10, 64):
        keys, dup = _keys(a, None, k, want_duplicates=True)
        sim, idx = U.decode_keys(keys)
        assert np.array_equal(idx, np.tile(np.arange(k), (N, 1)))
        assert np.array_equal(keys, U.reference_keys(a, None, k))
        assert not dup.any()
    res = nearest_atoms(dev(a), None, 10)
    assert res["n_duplicate_groups"] == 1 and not res["duplicate_of"].any()


def test_zero_atoms_scattered():
    N, D = 700, 64
    a = U.ternary(5, N, D).copy()
    zeros = [3, 128, 129, 400, 699]
    a[zeros] = 0
    keys, dup = _keys(a, None, 10, want_duplicates=True)
    assert np.array_equal(keys, U.reference_keys(a, None, 10))
    sim, idx = U.decode_keys(keys)
    for z in zeros:
        # cosine 0 with everything: the positive cosines do not exist, so the lowest indices at exactly 0 lead
        assert idx[z].tolist() == list(range(10)) and not sim[z].any()
        assert dup[z] == 3
    expect = U.reference_duplicate_of(a)
    assert np.array_equal(dup, expect) and U.n_duplicate_groups(dup) == 1


def test_planted_pairs_and_triples_across_tiles_and_splits():
    N, D = 2300, 64                                          # 9 column tiles: two per workgroup, 5 splits
    a = U.nbit(9, N, D).copy()
    plant = {127: [128, 2299], 5: [255, 256], 511: [512], 1000: [2047, 2048], 0: [2298]}
    for src, dsts in plant.items():
        a[dsts] = a[src]
    keys, dup = _keys(a, None, 10, want_duplicates=True)
    assert np.array_equal(keys, U.reference_keys(a, None, 10))
    expect = np.arange(N, dtype=np.int32)
    for src, dsts in plant.items():
        expect[dsts] = src
    assert np.array_equal(dup, expect) and np.array_equal(dup, U.reference_duplicate_of(a))
    _, idx = U.decode_keys(keys)
    for src, dsts in plant.items():
        group = [src] + dsts
        for n, d in enumerate(dsts):
            assert idx[d, :n + 2].tolist() == group[:n + 2]  # the lower duplicates come before the atom itself
    assert nearest_atoms(dev(a), None, 1)["n_duplicate_groups"] == len(plant)


def test_k_larger_than_the_candidates():
    a = U.ternary(11, 7, 32)
    keys, _ = _keys(a, None, 64)
    assert np.array_equal(keys, U.reference_keys(a, None, 64)) and not keys[:, 7:].any() and keys[:, :7].all()
    keys, _ = _keys(a, U.ternary(12, 3, 32), 10)
    assert not keys[:, 3:].any() and keys[:, :3].all()
    keys, _ = _keys(a[:1], None, 5, exclude_self=True)       # one atom, itself excluded: nothing
    assert not keys.any()
    res = nearest_atoms(dev(a[:1]), None, 5, include_self=False)
    assert res["index"].tolist() == [[-1] * 5] and torch.isinf(res["similarity"]).all()
    keys, _ = ops.nearest_atoms_i8(dev(a), torch.empty((0, 32), dtype=torch.int8, device=DEV), 4)
    assert keys.shape == (7, 4) and not keys.any()
    keys, dup = ops.nearest_atoms_i8(torch.empty((0, 32), dtype=torch.int8, device=DEV), None, 4, want_duplicates=True)
    assert keys.shape == (0, 4) and dup.shape == (0,)


# ---- robustness ------------------------------------------------------------------------------------------------------
def test_strides_and_garbage_between_d_and_ld():
    Na, Nb, D, k = 300, 520, 64, 10
    a, b = _pair("int8", Na, Nb, D)
    wa = torch.full((Na, D + 48), 77, dtype=torch.int8, device=DEV)            # ld = 112
    wb = torch.full((Nb, 4 * D), -128, dtype=torch.int8, device=DEV)           # ld = 256
    wa[:, :D] = dev(a)
    wb[:, :D] = dev(b)
    va, vb = wa[:, :D], wb[:, :D]
    assert ops._atoms_i8(va, "a").data_ptr() == wa.data_ptr()                   # read in place
    keys, _ = ops.nearest_atoms_i8(va, vb, k)
    assert np.array_equal(keys.cpu().numpy(), U.reference_keys(a, b, k))
    keys, dup = ops.nearest_atoms_i8(vb, None, k, want_duplicates=True)
    assert np.array_equal(keys.cpu().numpy(), U.reference_keys(b, None, k))
    # a stride the kernel cannot read (not a multiple of 16) is copied, not refused
    odd = torch.full((Na, D + 5), 9, dtype=torch.int8, device=DEV)
    odd[:, :D] = dev(a)
    keys, _ = ops.nearest_atoms_i8(odd[:, :D], vb, k)
    assert np.array_equal(keys.cpu().numpy(), U.reference_keys(a, b, k))


@pytest.mark.parametrize("N", [300, 2100])
def test_outputs_stay_inside_their_buffers(N):
    D, k, pad = 64, 10, 1024
    a = _atoms("ternary", N, D, 31)
    A = dev(a)
    kbuf = torch.full((pad + N * k + pad,), -7, dtype=torch.int64, device=DEV)
    dbuf = torch.full((pad + N + pad,), -7, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    need = int(lib.qsae_nearest_atoms_i8_workspace_bytes(N, N, D, k))
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    _lib.check(lib.qsae_nearest_atoms_i8(A.data_ptr(), D, N, None, 0, 0, D, k, 0, kbuf.data_ptr() + 8 * pad,
                                         dbuf.data_ptr() + 4 * pad, ws.data_ptr(), need,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert (kbuf[:pad] == -7).all() and (kbuf[pad + N * k:] == -7).all()
    assert (dbuf[:pad] == -7).all() and (dbuf[pad + N:] == -7).all()
    assert (ws[need:] == 0x5A).all()
    assert np.array_equal(kbuf[pad:pad + N * k].view(N, k).cpu().numpy(), U.reference_keys(a, None, k))
    assert np.array_equal(dbuf[pad:pad + N].cpu().numpy(), U.reference_duplicate_of(a))


def test_two_calls_give_identical_bytes_and_duplicates_are_optional():
    a = dev(_atoms("nbit4", 2100, 64, 33))
    k1, d1 = ops.nearest_atoms_i8(a, None, 64, want_duplicates=True)
    k2, d2 = ops.nearest_atoms_i8(a, None, 64, want_duplicates=True)
    k3, d3 = ops.nearest_atoms_i8(a, None, 64)               # duplicate_of = NULL
    assert torch.equal(k1, k2) and torch.equal(d1, d2) and torch.equal(k1, k3) and d3 is None


def test_python_argument_errors_on_the_device():
    a = torch.zeros((4, 64), dtype=torch.int8, device=DEV)
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            ops.nearest_atoms_i8(a, None, bad_k)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.nearest_atoms_i8(a[:, :48].contiguous(), None, 4)
    with pytest.raises(ValueError, match="self mode"):
        ops.nearest_atoms_i8(a, a.clone(), 4, exclude_self=True)
    with pytest.raises(ValueError, match="self mode"):
        ops.nearest_atoms_i8(a, a.clone(), 4, want_duplicates=True)
    with pytest.raises(TypeError):
        ops.nearest_atoms_i8(a.float(), None, 4)
    with pytest.raises(ValueError, match="same D"):
        ops.nearest_atoms_i8(a, torch.zeros((4, 32), dtype=torch.int8, device=DEV), 4)


def test_torch_op_passes_opcheck_and_equals_ops():
    a, b = _pair("ternary", 300, 520, 64)
    A, B = dev(a), dev(b)
    for args in ((A, B, 10, False, False), (A, None, 10, True, True), (A, None, 3, False, False)):
        keys, dup = torch.ops.qsae.nearest_atoms_i8(*args)
        ek, ed = ops.nearest_atoms_i8(*args)
        assert torch.equal(keys, ek)
        assert torch.equal(dup, ed) if ed is not None else dup.numel() == 0
        torch.library.opcheck(torch.ops.qsae.nearest_atoms_i8.default, args)
    keys, dup = T.nearest_atoms_i8(A, None, 10, want_duplicates=False)
    assert dup is None and torch.equal(keys, ops.nearest_atoms_i8(A, None, 10)[0])


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.GOLDEN_CASES))
def test_inspector_against_the_reference_inspector(name):
    import quantizedsae_amd.sae as sae
    g = U.load_golden(name)
    model = U.golden_model(sae, g["meta"]["recipe"]).to(DEV)
    assert np.array_equal(integer_atoms(model).cpu().numpy(), g["atoms"])
    ins = DictionaryInspector(model)
    k = g["meta"]["k"]
    if int(g["zero_entries"]):
        with pytest.raises(ValueError, match="all-zero"):
            ins.calculate_k_nearest_features_cluster(k, "euclidean")
    else:
        de, ie = ins.calculate_k_nearest_features_cluster(k, "euclidean")
    dist, idx = ins.calculate_k_nearest_features_cluster(k)
    assert dist.shape == idx.shape == (g["atoms"].shape[0], k) and dist.dtype == torch.float32 and idx.dtype == torch.int64
    share = U.check_against_golden(g, dist.cpu().numpy(), idx.cpu().numpy())
    assert share >= 0.9
    if not int(g["zero_entries"]):
        assert torch.equal(ie, idx)
        assert torch.allclose(de, torch.sqrt(2 * dist), atol=1e-3)         # ||u - v||^2 = 2 - 2c = 2 * distance
    assert ins.count_duplicates() == int(g["count_duplicates"])
    assert ins.zero_entries() == int(g["zero_entries"])
    assert ins.sparsity_rate() == pytest.approx(float(g["sparsity_rate"]), abs=1e-12)
    assert ins.analyze_ternary_distribution() == dict(zip(g["values"].tolist(), g["value_counts"].tolist()))
    tol = float(g["ref_fp64_maxdev"]) + 3e-7
    for (f1, f2), dc in zip(g["meta"]["pairs"], g["pair_cosine"]):
        assert abs(float(ins.distance(f1, f2)) - dc) <= tol
    for s, count in zip(g["meta"]["same"], g["same_count"]):
        assert ins.check_same_entries(s)[0] == int(count)


def test_registry_shape_against_fp64_on_the_device():
    N, D, k = 32768, 512, 10
    a = U.ternary(77, N, D).copy()
    plant = {100: [20000], 4095: [4096, 32767], 16383: [16384]}
    for src, dsts in plant.items():
        a[dsts] = a[src]
    A = dev(a)
    res = nearest_atoms(A, None, k)
    rows = torch.arange(0, N, 64, device=DEV)
    A64 = A.double()
    nrm = torch.linalg.norm(A64, dim=1)
    assert (nrm > 0).all()
    c64 = (A64[rows] @ A64.t()) / nrm[rows, None] / nrm[None, :]
    sim, idx = res["similarity"][rows], res["index"][rows]
    got = torch.gather(c64, 1, idx)
    err = (sim.double() - got).abs().max().item()
    kth = torch.topk(c64, k, dim=1).values[:, -1:]
    short = (kth - got).max().item()
    print(f"registry shape: max |c - c64| = {err:.3g}, worst shortfall against the fp64 k-th largest = {short:.3g}")
    assert err <= 1e-6
    assert short <= 2e-6
    dup = res["duplicate_of"].cpu().numpy()
    expect = np.arange(N, dtype=np.int32)
    for src, dsts in plant.items():
        expect[dsts] = src
    assert np.array_equal(dup, expect)
    assert res["n_duplicate_groups"] == len(plant)
