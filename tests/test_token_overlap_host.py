"""The token-overlap comparison without a GPU: qsae_token_overlap_hist is declared, bound and exported and answers every
bad argument before any HIP call (the only reason these calls can be made without a device); top_token_sets on host
tensors gives the reference's sets; JaccardHistogram turns the reference's (inter, union) counts back into the
numbers the reference printed."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import token_overlap_util as U
from quantizedsae_amd import _lib, build
from quantizedsae_amd.inference import (JaccardHistogram, average_unique_tokens_per_active_feature, top_token_sets)

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("qsae_token_overlap_hist_workspace_bytes", "qsae_token_overlap_hist")
CASES = sorted(U.RECIPES)


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "qsae.h").read_text()
    exported = build.exported_symbols(_lib.LIB_PATH)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header)
        assert name in _lib.SIGNATURES and name in exported
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "token_overlap.hip" in build.SOURCES
    assert lib.qsae_abi_version() == _lib.ABI_VERSION == 4     # an additive change


def test_workspace_is_monotone_and_zero_for_invalid_shapes():
    size = _lib.load().qsae_token_overlap_hist_workspace_bytes
    grid = (1, 5, 255, 256, 257, 1030, 32768)
    for fixed in grid:
        for vary in range(3):
            sizes = []
            for v in grid:
                args = [fixed, fixed, fixed]
                args[vary] = v
                sizes.append(size(*args))
            assert sizes == sorted(sizes) and sizes[0] > 0
    assert size(300, 200, 1030) == (300 + 200) * 5 * 32       # both sides re-tiled by 256-token chunk, nothing else
    assert size(300, 200, 256) < size(300, 200, 257)
    assert size(-1, 4, 32) == 0 and size(4, -1, 32) == 0 and size(4, 4, 0) == 0 and size(4, 4, -7) == 0


def _call(lib, *, asets=0x1000, a_ld=3, asize=0x2000, Na=8, bsets=0x3000, b_ld=3, bsize=0x4000, Nb=8, V=70, k=10,
          hist=0x5000, ws=0x6000, ws_bytes=1 << 20):
    """Dummy non-null pointers: a call that got as far as a kernel launch would not return an argument error."""
    return lib.qsae_token_overlap_hist(asets, a_ld, asize, Na, bsets, b_ld, bsize, Nb, V, k, hist, ws, ws_bytes, None)


@pytest.mark.parametrize("bad", [
    dict(asets=None), dict(asize=None), dict(bsets=None), dict(bsize=None), dict(hist=None), dict(V=0), dict(V=-3),
    dict(a_ld=2), dict(b_ld=2), dict(Na=-1), dict(Nb=-1), dict(ws=0x6004),
])
def test_invalid_arguments_are_refused_before_any_hip_call(bad):
    lib = _lib.load()
    assert _call(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_token_overlap_hist" in lib.qsae_last_error()


@pytest.mark.parametrize("k", [0, 129, -1])
def test_k_outside_the_table_limit_is_unsupported(k):
    lib = _lib.load()
    assert _call(lib, k=k) == _lib.ERR_UNSUPPORTED
    assert _call(lib, k=k, Na=0) == _lib.ERR_UNSUPPORTED       # also when there is nothing to do


def test_small_workspace_and_empty_sides():
    lib = _lib.load()
    need = lib.qsae_token_overlap_hist_workspace_bytes(8, 8, 70)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert _call(lib, ws=None) == _lib.ERR_WORKSPACE
    for empty in (dict(Na=0), dict(Nb=0), dict(Na=0, Nb=0)):
        assert _call(lib, **empty) == _lib.OK
        assert _call(lib, asets=None, asize=None, bsets=None, bsize=None, hist=None, ws=None, ws_bytes=0, **empty) == _lib.OK


# ---- top_token_sets on host tensors --------------------------------------------------------------------------------
def _sorted_rows(tokens: torch.Tensor) -> np.ndarray:
    """padded sets with each row's tokens ascending and the -1 fill last, as the fixtures store them"""
    t = tokens.numpy().astype(np.int64)
    big = np.where(t < 0, np.iinfo(np.int64).max, t)
    big.sort(axis=1)
    return np.where(big == np.iinfo(np.int64).max, -1, big)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("form", ["lists", "csr"])
def test_top_token_sets_equal_the_reference_sets(name, form):
    meta, gold = U.load(name)
    la, aa, lb, ab = U.token_lists(meta)
    for lists, act, want in ((la, aa, gold["sets_a"]), (lb, ab, gold["sets_b"])):
        tpf = lists if form == "lists" else tuple(torch.from_numpy(x) for x in U.csr(lists))
        sets = top_token_sets(tpf, torch.from_numpy(act), meta["k"])
        assert sets.tokens.shape == want.shape and sets.tokens.dtype == torch.int64
        assert np.array_equal(_sorted_rows(sets.tokens), want)
        assert np.array_equal(sets.sizes.numpy(), (want >= 0).sum(1))
        # most frequent first, -1 only beyond the size
        assert np.array_equal((sets.tokens.numpy() >= 0).sum(1), sets.sizes.numpy())
        assert all((row[:n] >= 0).all() for row, n in zip(sets.tokens.numpy(), sets.sizes.numpy()))
        assert sets.distinct.tolist() == [len(set(t)) for t in lists]
        live = [len(set(t)) for t, a in zip(lists, act) if a > 0]
        assert average_unique_tokens_per_active_feature(sets, torch.from_numpy(act)) == float(sum(live) / len(live))


def test_top_token_sets_order_and_degenerate_inputs():
    lists = [[5, 9, 9, 5, 2, 7, 7], [], [4], [3, 3]]
    sets = top_token_sets(lists, torch.tensor([7, 0, 1, 0]), 3)
    # counts 5:2 9:2 2:1 7:2 -- the three twos in order of first occurrence; feature 3 has a list but never fired
    assert sets.tokens.tolist() == [[5, 9, 7], [-1, -1, -1], [4, -1, -1], [-1, -1, -1]]
    assert sets.sizes.tolist() == [3, 0, 1, 0] and sets.distinct.tolist() == [4, 0, 1, 1]
    none = top_token_sets([[], []], torch.tensor([0, 0]), 4)
    assert none.tokens.tolist() == [[-1] * 4] * 2 and none.sizes.tolist() == [0, 0]
    assert average_unique_tokens_per_active_feature(none, torch.tensor([0, 0])) == 0.0
    with pytest.raises(ValueError):
        top_token_sets([[1]], torch.tensor([1, 1]), 4)
    with pytest.raises(ValueError):
        top_token_sets([[-1]], torch.tensor([1]), 4)
    with pytest.raises(ValueError):
        top_token_sets([[1]], torch.tensor([1]), 0)


# ---- JaccardHistogram against the numbers of the reference ---------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_histogram_gives_the_numbers_of_the_reference(name):
    meta, gold = U.load(name)
    h = JaccardHistogram(torch.from_numpy(U.hist_from_triples(gold["triples"], meta["k"])))
    assert h.n_pairs == int(gold["n_pairs"])
    assert h.top(10000) == gold["top_scores"].tolist()
    for n, used, mean in zip(gold["top_n"].tolist(), gold["top_used"].tolist(), gold["top_mean"].tolist()):
        assert h.top(n) == gold["top_scores"][:n].tolist()
        assert h.top_mean(n) == (mean, used)
    want = float(gold["mean"])
    assert abs(h.mean() - want) <= math.ulp(want)
    s = h.summary()
    assert s["n_pairs"] == h.n_pairs and s["mean"] == h.mean()
    assert s["top"] == {n: h.top_mean(n) for n in (10, 100, 1000, 10000)}


def test_histogram_without_pairs():
    h = JaccardHistogram(torch.zeros((4, 7), dtype=torch.int64))
    assert h.n_pairs == 0 and h.mean() is None and h.top(5) == [] and h.top_mean(5) == (None, 0)


def test_numpy_formulation_matches_the_reference_triples():
    """the formulation the GPU tests compare the kernel with, on the reference's own sets"""
    for name in CASES:
        meta, gold = U.load(name)
        k, V = meta["k"], meta["V"]
        sa, sb = gold["sets_a"], gold["sets_b"]
        got = U.hist_numpy(U.membership(sa, V), (sa >= 0).sum(1), U.membership(sb, V), (sb >= 0).sum(1), k)
        assert np.array_equal(got, U.hist_from_triples(gold["triples"], k))
        M = U.membership(sa, V)
        bits = U.pack(M).view(np.uint32)
        assert all(((bits[i, t >> 5] >> np.uint32(t & 31)) & 1) == M[i, t] for i in (2, 3, 4) for t in (0, V // 2, V - 1))
