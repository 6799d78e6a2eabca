"""qsae_nearest_atoms_f32 on the GPU: the keys equal the numpy restatement of the arithmetic contract
bit for bit -- on every edge of the tiling (128 queries, 128 candidates per tile), of the candidate split (up to 8
workgroups per query panel; above 1024 candidates a workgroup sweeps more than one tile), with both loaders (D % 32 == 0
and the K tail) and on both sides of k = 6 / 7, where a second workgroup stops fitting a CU's LDS; on dictionaries
built to make every product pass the filter; against the int8 path and cosine_compare where they answer the same
question; and through nearest_atoms / DictionaryInspector against what the reference recorded."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dictionary_neighbors_util as NU
import neighbors_f32_util as U
import quantizedsae_amd as Q
from quantizedsae_amd import _lib, ops
from quantizedsae_amd import torch_ops as T
from quantizedsae_amd.inference import DictionaryInspector, nearest_atoms

pytestmark = pytest.mark.gpu
DEV = "cuda"

QUERIES = (1, 127, 128, 129)
CANDIDATES = (1, 255, 256, 257, 1025)         # 1025: nine tiles, five splits of two tiles
DS = (4, 36, 64, 512)                         # 4, 36: the K-tail loader; 64, 512: the asm-staged loader
KS = (1, 6, 7, 10, 64)                        # 6 | 7: two workgroups per CU | one


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _atoms(N, D, seed):
    """Gaussian atoms; a few rows are scaled far up and down (the cosine must not care)."""
    a = U.gaussian(seed + D, N, D).copy()
    a[::7] *= np.float32(1e3)
    a[3::11] *= np.float32(1e-3)
    return a


@functools.lru_cache(maxsize=4)
def _cosines(Na, Nb, D):
    """The restatement's cosines, computed once per shape (Nb None: self) and shared by every k and mode."""
    a = _atoms(Na, D, 100)
    b = None if Nb is None else _atoms(Nb, D, 200)
    c = U.cosines(a, b)
    c.setflags(write=False)
    return a, b, c


def _keys(a, b=None, k=10, exclude_self=False):
    return ops.nearest_atoms_f32(dev(a), None if b is None else dev(b), k, exclude_self).cpu().numpy()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("Nb", CANDIDATES)
@pytest.mark.parametrize("Na", QUERIES)
def test_cross_keys_equal_the_restatement(Na, Nb, D):
    a, b, c = _cosines(Na, Nb, D)
    A, B = dev(a), dev(b)
    for k in KS:
        assert np.array_equal(ops.nearest_atoms_f32(A, B, k).cpu().numpy(), U.keys_of(c, k)), k
    # the swapped problem: the same products in the same order and a commutative scaling give c transposed
    for k in (1, 10, 64):
        assert np.array_equal(ops.nearest_atoms_f32(B, A, k).cpu().numpy(), U.keys_of(np.ascontiguousarray(c.T), k)), k


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", sorted(set(QUERIES + CANDIDATES)))
def test_self_keys_equal_the_restatement(N, D):
    a, _, c = _cosines(N, None, D)
    A = dev(a)
    for k in KS:
        assert np.array_equal(ops.nearest_atoms_f32(A, None, k).cpu().numpy(), U.keys_of(c, k)), k
        assert np.array_equal(ops.nearest_atoms_f32(A, None, k, True).cpu().numpy(), U.keys_of(c, k, True)), k


# ---- dictionaries built against the filter and the buffers -----------------------------------------------------------
@pytest.mark.parametrize("D", [4, 64])
def test_ordered_candidates_every_product_passes_the_filter(D):
    """Candidate j is at cosine (j + 1) / (Nb + 1) of every query: each later candidate beats all earlier ones, so every
    product passes the filter and every round fills the append buffer."""
    Na, Nb = 130, 1200                                       # ten tiles: five splits of two
    x = (np.arange(Nb, dtype=np.float64) + 1) / (Nb + 1)
    b = np.zeros((Nb, D), dtype=np.float32)
    b[:, 0], b[:, 1] = x, np.sqrt(1 - x * x)
    a = np.zeros((Na, D), dtype=np.float32)
    a[:, 0] = 1 + np.arange(Na)
    c = U.cosines(a, b)
    assert (np.diff(c, axis=1) > 0).all()
    for k in (1, 10, 64):
        keys = _keys(a, b, k)
        assert np.array_equal(keys, U.keys_of(c, k))
        assert np.array_equal(U.decode_keys(keys)[1], np.tile(np.arange(Nb - 1, Nb - 1 - k, -1), (Na, 1)))


def test_nested_atoms_in_self_mode():
    N, D = 300, 320
    a = (np.arange(D)[None, :] <= np.arange(N)[:, None]).astype(np.float32)   # atom j: ones in dimensions 0..j
    c = U.cosines(a)
    for k in (1, 10, 64):
        assert np.array_equal(_keys(a, None, k), U.keys_of(c, k))
        assert np.array_equal(_keys(a, None, k, True), U.keys_of(c, k, True))


def test_identical_atoms_tie_on_value_and_order_by_index():
    N = 140
    a = np.repeat(U.gaussian(3, 1, 64), N, axis=0)
    for k in (10, 64):
        keys = _keys(a, None, k)
        sim, idx = U.decode_keys(keys)
        assert np.array_equal(idx, np.tile(np.arange(k), (N, 1))) and (sim == sim[0, 0]).all()
        assert np.array_equal(keys, U.reference_keys(a, None, k))


def test_zero_atoms_scattered():
    N, D = 700, 64
    a = U.gaussian(5, N, D).copy()
    zeros = [3, 128, 129, 400, 699]
    a[zeros] = 0
    keys = _keys(a, None, 10)
    assert np.array_equal(keys, U.reference_keys(a, None, 10))
    sim, idx = U.decode_keys(keys)
    for z in zeros:
        # cosine +0 with everything, itself included: the lowest indices at exactly 0 lead
        assert idx[z].tolist() == list(range(10)) and not sim[z].any()
    only_zero = np.zeros((5, 8), dtype=np.float32)
    sim, idx = U.decode_keys(_keys(only_zero, None, 5))
    assert np.array_equal(idx, np.tile(np.arange(5), (5, 1))) and not sim.any() and not np.signbit(sim).any()


def test_k_larger_than_the_candidates_and_empty_sides():
    a = U.gaussian(11, 7, 32)
    keys = _keys(a, None, 64)
    assert np.array_equal(keys, U.reference_keys(a, None, 64)) and not keys[:, 7:].any() and keys[:, :7].all()
    keys = _keys(a, U.gaussian(12, 3, 32), 10)
    assert not keys[:, 3:].any() and keys[:, :3].all()
    keys = _keys(a[:1], None, 5, exclude_self=True)          # one atom, itself excluded: nothing
    assert not keys.any()
    res = nearest_atoms(dev(a[:1]), None, 5, include_self=False)
    assert res["index"].tolist() == [[-1] * 5] and torch.isinf(res["similarity"]).all()
    keys = ops.nearest_atoms_f32(dev(a), torch.empty((0, 32), device=DEV), 4)
    assert keys.shape == (7, 4) and not keys.any()
    keys = ops.nearest_atoms_f32(torch.empty((0, 32), device=DEV), None, 4)
    assert keys.shape == (0, 4)
    keys = ops.nearest_atoms_f32(torch.empty((0, 32), device=DEV), dev(a), 4)
    assert keys.shape == (0, 4)


# ---- memory ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [36, 64])
def test_strides_and_nan_between_d_and_ld(D):
    Na, Nb, k = 300, 520, 10
    a, b = _atoms(Na, D, 100), _atoms(Nb, D, 200)
    wa = torch.full((Na, D + 12), float("nan"), device=DEV)
    wb = torch.full((Nb, 4 * D), float("nan"), device=DEV)
    wa[:, :D] = dev(a)
    wb[:, :D] = dev(b)
    va, vb = wa[:, :D], wb[:, :D]
    assert ops._atoms_f32(va, "a").data_ptr() == wa.data_ptr()                 # read in place
    expect = U.reference_keys(a, b, k)
    assert np.array_equal(ops.nearest_atoms_f32(va, vb, k).cpu().numpy(), expect)
    assert np.array_equal(ops.nearest_atoms_f32(vb, None, k).cpu().numpy(), U.reference_keys(b, None, k))
    # a stride the kernel cannot read (not a multiple of 4) is copied, not refused
    odd = torch.full((Na, D + 5), float("nan"), device=DEV)
    odd[:, :D] = dev(a)
    assert np.array_equal(ops.nearest_atoms_f32(odd[:, :D], vb, k).cpu().numpy(), expect)


@pytest.mark.parametrize("N", [300, 1100])
def test_outputs_stay_inside_their_buffers(N):
    D, k, pad = 64, 10, 1024
    a = _atoms(N, D, 31)
    A = dev(a)
    kbuf = torch.full((pad + N * k + pad,), -7, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    need = int(lib.qsae_nearest_atoms_f32_workspace_bytes(N, N, D, k))
    ws = torch.full((4096 + need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    assert (ws.data_ptr() + 4096) % 16 == 0
    _lib.check(lib.qsae_nearest_atoms_f32(A.data_ptr(), D, N, None, 0, 0, D, k, 0, kbuf.data_ptr() + 8 * pad,
                                          ws.data_ptr() + 4096, need,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert (kbuf[:pad] == -7).all() and (kbuf[pad + N * k:] == -7).all()
    assert (ws[:4096] == 0x5A).all() and (ws[4096 + need:] == 0x5A).all()
    assert np.array_equal(kbuf[pad:pad + N * k].view(N, k).cpu().numpy(), U.reference_keys(a, None, k))


def test_two_calls_give_identical_bytes():
    a = dev(_atoms(1100, 64, 33))
    k1, k2 = ops.nearest_atoms_f32(a, None, 64), ops.nearest_atoms_f32(a, None, 64)
    assert torch.equal(k1, k2)


def test_python_argument_errors_on_the_device():
    a = torch.zeros((4, 64), device=DEV)
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            ops.nearest_atoms_f32(a, None, bad_k)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.nearest_atoms_f32(a[:, :38].contiguous(), None, 4)
    with pytest.raises(ValueError, match="self mode"):
        ops.nearest_atoms_f32(a, a.clone(), 4, exclude_self=True)
    with pytest.raises(TypeError):
        ops.nearest_atoms_f32(a.to(torch.int8), None, 4)
    with pytest.raises(ValueError, match="same D"):
        ops.nearest_atoms_f32(a, torch.zeros((4, 32), device=DEV), 4)


def test_torch_op_passes_opcheck_and_equals_ops():
    A, B = dev(_atoms(300, 64, 100)), dev(_atoms(520, 64, 200))
    for args in ((A, B, 10, False), (A, None, 10, True), (A, None, 3, False)):
        keys = torch.ops.qsae.nearest_atoms_f32(*args)
        assert torch.equal(keys, ops.nearest_atoms_f32(*args))
        torch.library.opcheck(torch.ops.qsae.nearest_atoms_f32.default, args)
    assert torch.equal(T.nearest_atoms_f32(A, None, 10), ops.nearest_atoms_f32(A, None, 10))


# ---- against code that exists today ----------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", ["ternary", "nbit4"])
def test_integer_valued_atoms_equal_the_int8_path(recipe):
    a = NU.RECIPES[recipe](21, 1100, 64).copy()
    b = NU.RECIPES[recipe](22, 300, 64).copy()
    a[[5, 500]] = 0
    A, B = dev(a), dev(b)
    for k in (1, 10, 64):
        assert torch.equal(ops.nearest_atoms_f32(A.float(), None, k), ops.nearest_atoms_i8(A, None, k)[0])
        assert torch.equal(ops.nearest_atoms_f32(A.float(), None, k, True), ops.nearest_atoms_i8(A, None, k, True)[0])
        assert torch.equal(ops.nearest_atoms_f32(B.float(), A.float(), k), ops.nearest_atoms_i8(B, A, k)[0])
    res = nearest_atoms(A, None, 10, atoms="fp32")
    ref = nearest_atoms(A, None, 10)
    assert torch.equal(res["index"], ref["index"]) and torch.equal(res["similarity"], ref["similarity"])
    assert "duplicate_of" not in res and "n_duplicate_groups" not in res and "duplicate_of" in ref


@pytest.mark.parametrize("D", [36, 512])
def test_k1_equals_cosine_compare(D):
    A, B = dev(_atoms(300, D, 100)), dev(_atoms(520, D, 200))
    row_best = ops.cosine_compare(A, B)[0]
    assert torch.equal(ops.nearest_atoms_f32(A, B, 1)[:, 0], row_best)
    row_best = ops.cosine_compare(B, None)[0]                # self mode: each atom's best other atom
    assert torch.equal(ops.nearest_atoms_f32(B, None, 1, True)[:, 0], row_best)


# ---- models ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.GOLDEN_CASES))
def test_models_against_the_reference(name):
    g = U.load_golden(name)
    case = U.GOLDEN_CASES[name]
    lhs, rhs = U.golden_models(Q, case)
    lhs = lhs.to(DEV)
    rhs = None if rhs is None else rhs.to(DEV)
    k = g["meta"]["k"]
    res = nearest_atoms(lhs, rhs, k)
    assert set(res) == {"similarity", "index", "distance"}
    assert res["similarity"].dtype == torch.float32 and res["index"].dtype == torch.int64
    share = U.check_against_golden(g, res["similarity"].cpu().numpy(), res["index"].cpu().numpy())
    assert share >= 0.9
    assert torch.equal(res["distance"], torch.clamp(1.0 - res["similarity"], min=0.0))
    a, b = U.golden_atoms(case)
    assert np.array_equal(res["index"].cpu().numpy(), U.decode_keys(U.reference_keys(a, b, k))[1])
    if rhs is None:
        ins = DictionaryInspector(lhs)
        assert ins.atoms.dtype == torch.float32 and np.array_equal(ins.atoms.cpu().numpy(), a)
        dist, idx = ins.calculate_k_nearest_features_cluster(k)
        assert torch.equal(dist, res["distance"]) and torch.equal(idx, res["index"])
        de, ie = ins.calculate_k_nearest_features_cluster(k, "euclidean")
        assert torch.equal(ie, idx) and torch.allclose(de, torch.sqrt(2 * dist), atol=1e-3)
        assert ins.count_duplicates() == 0 and ins.zero_entries() == 0
        c64, _ = U.cosines_f64(a)
        assert abs(float(ins.distance(1, 2)) - (1 - c64[1, 2])) <= 1e-5
        with pytest.raises(TypeError, match="fp32"):
            ins.analyze_ternary_distribution()


# ---- the registry shape ----------------------------------------------------------------------------------------------
def test_registry_shape_against_fp64_on_the_device():
    N, D, k = 32768, 512, 10
    A = torch.randn((N, D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(77))
    res = nearest_atoms(A, None, k)
    rows = torch.arange(0, N, 64, device=DEV)
    A64 = A.double()
    nrm = torch.linalg.norm(A64, dim=1)
    den = nrm[rows, None] * nrm[None, :]
    c64 = (A64[rows] @ A64.t()) / den
    bound = (D + 5) * 2.0 ** -24 * (A64[rows].abs() @ A64.abs().t()) / den
    sim, idx = res["similarity"][rows], res["index"][rows]
    assert (idx[:, 0] == rows).all()                         # an atom is its own nearest atom
    got, gb = torch.gather(c64, 1, idx), torch.gather(bound, 1, idx)
    err = (sim.double() - got).abs()
    kth = torch.topk(c64, k, dim=1).values[:, -1:]
    short = kth - got
    print(f"registry shape: max |c - c64| = {err.max().item():.3g} (largest err / bound {(err / gb).max().item():.3g}), "
          f"worst shortfall against the fp64 k-th largest = {short.max().item():.3g} "
          f"(largest shortfall / bound {(short / gb).max().item():.3g})")
    assert (err <= gb).all()
    assert (short <= 2 * gb).all()
