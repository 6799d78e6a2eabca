"""Token-overlap histogram between two SAEs on the int8 matrix pipe (qsae_token_overlap_hist): the kernel against the
numpy integer formulation at the edges of its tiling (256-feature workgroup tile, 128-feature wave tile, 32 x 32 MFMA
tile, 256-token chunk, 32-token fragment), with bits and strides it must ignore and sizes it must refuse; end to end
against the reference's recorded scores; as a dispatcher op; and once at the registry shape against torch's fp32
product.  Integer results throughout: every comparison is an equality."""
import functools

import numpy as np
import pytest
import torch

import token_overlap_util as U
from quantizedsae_amd.inference import jaccard_histogram, top_token_sets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1, 1), (5, 3, 31), (33, 65, 257), (129, 255, 300), (257, 130, 513), (300, 520, 1030), (520, 300, 4099)]
KS = [1, 3, 100, 128]


def _ops():
    from quantizedsae_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(Na, Nb, V, k):
    """(Ma, asize, Mb, bsize, want): sizes spread over 0..k, side A four times as dense as side B, row 0 of each side
    holding the tokens around the chunk edge and the last one; the reference result is computed once per case."""
    seed = 1000 * k + Na
    Ma, _ = U.random_sets(seed, Na, V, k, 0.6, stream=1)
    Mb, _ = U.random_sets(seed, Nb, V, k, 0.15, stream=3)
    edge = [t for t in (V - 1, 256, 255) if 0 <= t < V][:k]
    for M in (Ma, Mb):
        M[0] = 0
        M[0, edge] = 1
    asize, bsize = Ma.sum(1).astype(np.int32), Mb.sum(1).astype(np.int32)
    want = U.hist_numpy(Ma, asize, Mb, bsize, k)
    for a in (Ma, asize, Mb, bsize, want):
        a.setflags(write=False)
    return Ma, asize, Mb, bsize, want


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("Na,Nb,V", SHAPES)
def test_kernel_matches_numpy(Na, Nb, V, k):
    ops = _ops()
    Ma, asize, Mb, bsize, want = case(Na, Nb, V, k)
    assert want.sum() == int((asize > 0).sum()) * int((bsize > 0).sum())
    args = (dev(U.pack(Ma)), dev(asize), dev(U.pack(Mb)), dev(bsize), V, k)
    hist = ops.token_overlap_hist(*args)
    assert hist.dtype == torch.int64 and hist.shape == (k + 1, 2 * k + 1)
    assert np.array_equal(host(hist), want)
    assert ops.token_overlap_hist(*args, hist) is hist          # accumulation over calls
    assert np.array_equal(host(hist), 2 * want)
    # the sides swapped: the table of the transposed problem is the same table
    swapped = ops.token_overlap_hist(args[2], args[3], args[0], args[1], V, k)
    assert np.array_equal(host(swapped), want)


def test_bits_at_or_past_V_are_ignored():
    Na, Nb, V, k = 129, 255, 300, 100
    Ma, asize, Mb, bsize, want = case(Na, Nb, V, k)
    words = (V + 31) // 32
    garbage = np.uint32(0xFFFFFFFF) << np.uint32(V - 32 * (words - 1))
    pa, pb = U.pack(Ma).view(np.uint32).copy(), U.pack(Mb).view(np.uint32).copy()
    pa[:, -1] |= garbage
    pb[::2, -1] |= garbage
    got = _ops().token_overlap_hist(dev(pa.view(np.int32)), dev(asize), dev(pb.view(np.int32)), dev(bsize), V, k)
    assert np.array_equal(host(got), want)


def test_row_stride_larger_than_the_words_of_V():
    Na, Nb, V, k = 257, 130, 513, 3
    Ma, asize, Mb, bsize, want = case(Na, Nb, V, k)
    words = (V + 31) // 32
    wide_a = torch.full((Na, words + 5), -1, dtype=torch.int32, device=DEV)      # all-ones words beside the slice
    wide_b = torch.full((Nb, 2 * words + 3), -1, dtype=torch.int32, device=DEV)
    wide_a[:, 2:2 + words] = dev(U.pack(Ma))
    wide_b[:, :words] = dev(U.pack(Mb))
    got = _ops().token_overlap_hist(wide_a[:, 2:2 + words], dev(asize), wide_b[:, :words], dev(bsize), V, k)
    assert np.array_equal(host(got), want)
    # a slice wider than ceil(V / 32) words: what lies past V is not read
    got = _ops().token_overlap_hist(wide_a[:, 2:3 + words], dev(asize), wide_b[:, :words + 1], dev(bsize), V, k)
    assert np.array_equal(host(got), want)


def test_inconsistent_sizes_are_dropped_and_nothing_else_is_written():
    Na, Nb, V, k = 33, 65, 257, 3
    Ma, asize, Mb, bsize, clean = case(Na, Nb, V, k)
    Ma, Mb, asize, bsize = Ma.copy(), Mb.copy(), asize.copy(), bsize.copy()
    big = int(np.argmax(asize > 0))
    asize[big] = k + 1                                           # a size above k: the feature takes part in no pair
    small = int(np.flatnonzero(asize == k)[-1])
    assert small != big
    Mb[7], bsize[7] = Ma[small], k                               # its copy on the other side: intersection k ...
    asize[small] = 1                                             # ... against a stated size of 1
    bsize[9] = -4
    want = U.hist_numpy(Ma, asize, Mb, bsize, k)
    dropped_big = U.hist_numpy(Ma, np.where(np.arange(Na) == big, 0, asize), Mb, bsize, k)
    assert np.array_equal(want, dropped_big)
    live = int((asize > 0).sum()) * int((bsize > 0).sum())
    assert 0 < live - want.sum()                                 # the shortfall is how a caller sees it
    bins, pad = (k + 1) * (2 * k + 1), 64
    buf = torch.full((pad + bins + pad,), -7, dtype=torch.int64, device=DEV)
    hist = buf[pad:pad + bins].view(k + 1, 2 * k + 1)
    hist.zero_()
    _ops().token_overlap_hist(dev(U.pack(Ma)), dev(asize), dev(U.pack(Mb)), dev(bsize), V, k, hist)
    assert np.array_equal(host(hist), want)
    assert (host(buf[:pad]) == -7).all() and (host(buf[pad + bins:]) == -7).all()


def test_front_end_refuses_what_the_kernel_cannot_take():
    ops = _ops()
    s = torch.zeros((4, 3), dtype=torch.int32, device=DEV)
    n = torch.ones(4, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.token_overlap_hist(s.cpu(), n.cpu(), s, n, 70, 5)
    with pytest.raises(TypeError):
        ops.token_overlap_hist(s.long(), n, s, n, 70, 5)
    with pytest.raises(ValueError):
        ops.token_overlap_hist(s, n, s, n, 100, 5)              # 4 words needed, 3 given
    with pytest.raises(ValueError):
        ops.token_overlap_hist(s, n[:3], s, n, 70, 5)
    with pytest.raises(ValueError):
        ops.token_overlap_hist(s, n, s, n, 70, 129)
    with pytest.raises(ValueError):
        ops.token_overlap_hist(s, n, s, n, 70, 5, torch.zeros((6, 10), dtype=torch.int64, device=DEV))
    empty = ops.token_overlap_hist(s[:0], n[:0], s, n, 70, 5)
    assert empty.shape == (6, 11) and not host(empty).any()


# ---- end to end against the reference's recorded scores ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.RECIPES))
def test_jaccard_histogram_equals_the_reference(name):
    meta, gold = U.load(name)
    k = meta["k"]
    la, aa, lb, ab = U.token_lists(meta)
    want = U.hist_from_triples(gold["triples"], k)
    stats_a = {"tokens_per_feature": la, "activation_counts": torch.from_numpy(aa)}
    stats_b = {"tokens_per_feature": lb, "activation_counts": torch.from_numpy(ab)}
    for compact in (True, False):
        h = jaccard_histogram(stats_a, stats_b, k, device=DEV, compact=compact)
        assert not h.counts.is_cuda and np.array_equal(h.counts.numpy(), want)
        assert h.n_pairs == int(gold["n_pairs"])
    # CSR input already on the device
    csr_a = {"tokens_per_feature": tuple(dev(x) for x in U.csr(la)), "activation_counts": dev(aa)}
    csr_b = {"tokens_per_feature": tuple(dev(x) for x in U.csr(lb)), "activation_counts": dev(ab)}
    h = jaccard_histogram(csr_a, csr_b, k)
    assert np.array_equal(h.counts.numpy(), want)
    assert h.top_mean(100) == (float(gold["top_mean"][1]), int(gold["top_used"][1]))
    sets = top_token_sets(csr_a["tokens_per_feature"], csr_a["activation_counts"], k)
    assert sets.tokens.is_cuda and np.array_equal(np.sort(host(sets.sizes)), np.sort((gold["sets_a"] >= 0).sum(1)))


# ---- dispatcher op -------------------------------------------------------------------------------------------------
def test_torch_op_mutates_in_place_and_passes_opcheck():
    import quantizedsae_amd.torch_ops as T
    Na, Nb, V, k = 129, 255, 300, 3
    Ma, asize, Mb, bsize, want = case(Na, Nb, V, k)
    args = (dev(U.pack(Ma)), dev(asize), dev(U.pack(Mb)), dev(bsize), V, k)
    assert "Tensor(a6!) hist" in str(torch.ops.qsae.token_overlap_hist.default._schema)
    hist = torch.zeros((k + 1, 2 * k + 1), dtype=torch.int64, device=DEV)
    assert torch.ops.qsae.token_overlap_hist(*args, hist) is None
    assert np.array_equal(host(hist), want)
    assert T.token_overlap_hist(*args, hist) is hist            # the wrapper accumulates into the caller's table
    assert np.array_equal(host(hist), 2 * want)
    assert torch.equal(T.token_overlap_hist(*args), _ops().token_overlap_hist(*args))
    torch.library.opcheck(torch.ops.qsae.token_overlap_hist.default, (*args, torch.zeros_like(hist)))


# ---- the registry shape --------------------------------------------------------------------------------------------
def _device_sets(N, V, k, gen):
    """Zipf-like random sets built on the device: (packed int32 [N, V / 32], sizes int32 [N], bool [N, V])"""
    assert V % 32 == 0
    tok = (V * torch.rand((N, k), device=DEV, generator=gen) ** 3).long().clamp_(max=V - 1)
    M = torch.zeros((N, V), dtype=torch.bool, device=DEV)
    M.scatter_(1, tok, True)
    M[torch.rand(N, device=DEV, generator=gen) < 0.03] = False        # features without a set
    shifts = torch.arange(32, device=DEV, dtype=torch.int64)
    packed = torch.empty((N, V // 32), dtype=torch.int32, device=DEV)
    for r in range(0, N, 4096):
        packed[r:r + 4096] = (M[r:r + 4096].view(-1, V // 32, 32).long() << shifts).sum(-1).to(torch.int32)
    return packed, M.sum(1).to(torch.int32), M


def test_registry_shape_against_the_fp32_product():
    ops = _ops()
    N, V, k, rows = 32768, 50304, 100, 512
    gen = torch.Generator(device=DEV).manual_seed(11)
    pa, asize, Ma = _device_sets(N, V, k, gen)
    pb, bsize, Mb = _device_sets(N, V, k, gen)
    hist = ops.token_overlap_hist(pa, asize, pb, bsize, V, k)
    assert int(hist.sum()) == int((asize > 0).sum()) * int((bsize > 0).sum())
    # 512 rows of A against all of B: sums of at most k ones are exact in fp32
    inter = (Ma[:rows].float() @ Mb.float().T).long()
    sa, sb = asize[:rows].long()[:, None], bsize.long()[None, :]
    ok = (sa > 0) & (sb > 0)
    want = torch.bincount((inter * (2 * k + 1) + sa + sb - inter)[ok], minlength=(k + 1) * (2 * k + 1))
    got = ops.token_overlap_hist(pa[:rows], asize[:rows], pb, bsize, V, k)
    assert torch.equal(got.view(-1), want)
    assert int(got[1:].sum()) > 0 and int(got[0].sum()) > 0
