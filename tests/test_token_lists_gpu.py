"""Tokens per feature as ordered CSR lists on the device (qsae_token_lists_*, inference/token_lists.py) against the numpy
restatement of the reference's definition (dynamic_analysis.py:283-306): tokens_per_feature[f] =
flat_tok[np.nonzero(mask[:, f])[0]] over the concatenated batches.  Integer work: every comparison is exact."""
import numpy as np
import pytest
import torch

import token_lists_util as U
from golden_util import Fixture
from quantizedsae_amd import (BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, ResidualQuantizedSAE)
from quantizedsae_amd.inference import TokenLists, jaccard_histogram, token_lists_to_python, top_token_sets
from quantizedsae_amd.inference import analysis as A
from quantizedsae_amd.inference import framework as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _ops():
    from quantizedsae_amd import ops
    return ops


def _batch(count, tok):
    """count = (offsets, workspace) of one batch -> (offsets, tokens) on the host"""
    ops = _ops()
    offsets, ws = count
    assert offsets.dtype == torch.int64 and ws.dtype == torch.uint8
    tokens = ops.token_lists_fill(ws, offsets, dev(tok), int(offsets[-1]))
    assert tokens.dtype == torch.int32
    return host(offsets), host(tokens)


def _check(got, mask, tok):
    want_off, want_tok = U.restate(mask, tok)
    assert np.array_equal(got[0], want_off)
    assert np.array_equal(got[1], want_tok)


# ---- test 1: compact form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,k,H", [(1, 1, 32), (37, 5, 33), (300, 65, 1024), (2100, 3, 64)])
def test_compact_form_equals_the_restatement(B, k, H):
    """(2100, 3, 64): 66 bitmap words per unit, so the prefix scan carries across a 64-word round."""
    ops = _ops()
    rng = np.random.default_rng(B * 11 + k)
    never, always = H - 1, 0                                # a unit active in no row and a unit active in every row
    idx = np.empty((B, k), np.int32)
    for r in range(B):
        others = rng.permutation(np.arange(1, H - 1))[:k - 1] if k > 1 else np.zeros(0, np.int64)
        row = np.concatenate([[always], others])
        idx[r] = rng.permutation(row)                       # distinct units per row, `always` at a random slot
    val = rng.standard_normal((B, k)).astype(np.float32)
    val[idx == always] = 1.5
    if B * k >= 8:                                          # planted inactive values (never on the always-active unit)
        flat = np.flatnonzero(idx.reshape(-1) != always)
        for pos, v in zip(flat[:3], (0.0, -0.0, np.nan)):
            val.reshape(-1)[pos] = v
    tok = U.row_tokens(B)
    mask = np.zeros((B, H), bool)
    with np.errstate(invalid="ignore"):
        np.put_along_axis(mask, idx.astype(np.int64), val > 0, axis=1)
    assert mask[:, always].all() and not mask[:, never].any()
    _check(_batch(ops.token_lists_count(dev(idx), dev(val), H), tok), mask, tok)
    all_on = np.zeros((B, H), bool)
    np.put_along_axis(all_on, idx.astype(np.int64), True, axis=1)
    _check(_batch(ops.token_lists_count(dev(idx), None, H), tok), all_on, tok)


# ---- test 2: bits form, identity index ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,words", [(5, 1), (333, 7), (2100, 2), (1030, 64)])
def test_bits_form_with_the_identity_map(B, words):
    ops = _ops()
    rng = np.random.default_rng(B + words)
    H = 32 * words
    bits = rng.random((B, H)) < rng.random(H)               # unequal densities per unit
    bits[:, 0] = True
    bits[:, H - 1] = False
    tok = U.row_tokens(B)
    _check(_batch(ops.token_lists_count_bits(dev(U.pack(bits)), H), tok), bits, tok)
    # more units than packed positions: the units past nbits have empty lists
    wide = np.concatenate([bits, np.zeros((B, 5), bool)], axis=1)
    _check(_batch(ops.token_lists_count_bits(dev(U.pack(bits)), H + 5), tok), wide, tok)
    # a column slice of a wider packed tensor is read in place
    z = dev(np.concatenate([U.pack(~bits), U.pack(bits)], axis=1))[:, words:]
    _check(_batch(ops.token_lists_count_bits(z, H), tok), bits, tok)


# ---- test 3: bits form with an index map --------------------------------------------------------------------------
def test_bits_form_with_a_permutation_and_pad_slots_whose_bits_are_set():
    ops = _ops()
    rng = np.random.default_rng(3)
    B, nbits, H = 201, 64, 50
    index = np.full(nbits, -1, np.int32)
    slots = rng.permutation(nbits)
    index[slots[:H]] = rng.permutation(H)
    bits = rng.random((B, nbits)) < 0.4
    bits[:, index < 0] = True                               # pad slots: set, and ignored
    mask = np.zeros((B, H), bool)
    mask[:, index[index >= 0]] = bits[:, index >= 0]
    tok = U.row_tokens(B)
    for idx_t in (dev(index), dev(index).long()):
        _check(_batch(ops.token_lists_count_bits(dev(U.pack(bits)), H, idx_t), tok), mask, tok)


def test_bits_form_with_the_residual_layout():
    ops = _ops()
    rng = np.random.default_rng(4)
    B, nbits = 130, 96                                      # three stages of 32 side by side, each with its unit offset
    index = np.arange(nbits, dtype=np.int32)
    bits = rng.random((B, nbits)) < 0.3
    tok = U.row_tokens(B)
    _check(_batch(ops.token_lists_count_bits(dev(U.pack(bits)), nbits, dev(index)), tok), bits, tok)


def test_bits_form_with_every_position_a_pad():
    ops = _ops()
    B, nbits, H = 70, 128, 40
    bits = np.ones((B, nbits), bool)
    offsets, tokens = _batch(ops.token_lists_count_bits(dev(U.pack(bits)), H, dev(np.full(nbits, -1, np.int32))), U.row_tokens(B))
    assert offsets.shape == (H + 1,) and not offsets.any() and tokens.shape == (0,)


def test_empty_batch_and_refused_arguments():
    ops = _ops()
    off, tok = _batch(ops.token_lists_count_bits(torch.zeros((0, 2), dtype=torch.int32, device=DEV), 64), U.row_tokens(0))
    assert not off.any() and tok.shape == (0,)
    off, tok = _batch(ops.token_lists_count(torch.zeros((0, 4), dtype=torch.int32, device=DEV), None, 33), U.row_tokens(0))
    assert off.shape == (34,) and not off.any() and tok.shape == (0,)
    z = torch.zeros((4, 2), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.token_lists_count_bits(z, 32)                   # identity map with more positions than units
    with pytest.raises(ValueError):
        ops.token_lists_count_bits(z, 64, torch.zeros(63, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.token_lists_count_bits(z.cpu(), 64)
    with pytest.raises(TypeError):
        ops.token_lists_count(z.long(), None, 64)


# ---- test 4: regroup ------------------------------------------------------------------------------------------------
def _token_ids(n_rows, tpc):
    contexts = (n_rows + tpc - 1) // tpc
    return ((np.arange(contexts * tpc, dtype=np.int64) * 7919) % 50257).reshape(contexts, tpc)


@pytest.mark.parametrize("rows", [(7, 0, 64, 33), (45,), ()], ids=["four_batches", "one_batch", "no_batch"])
def test_regroup_equals_the_single_mask_restatement(rows):
    rng = np.random.default_rng(9)
    H, tpc = 33, 5                                          # contexts straddle the batch boundaries
    n = sum(rows)
    flat_tok = _token_ids(n, tpc).reshape(-1)[:n]
    mask = rng.random((n, H)) < 0.3
    mask[:, 4] = False
    mask[:, 7] = True
    bits = np.concatenate([mask, np.zeros((n, 64 - H), bool)], axis=1)
    lists, g = TokenLists(H, DEV), 0
    for i, b in enumerate(rows):
        tok = torch.from_numpy(flat_tok[g:g + b])           # int64 on the host, as analyze_dataset passes it
        if i % 2 == 0:
            index = np.where(np.arange(64) < H, np.arange(64), -1).astype(np.int32)
            lists.add_bits(dev(U.pack(bits[g:g + b])), dev(index), tok)
        else:                                               # the same rows in the compact form: every unit listed, val = +-1
            idx = np.tile(np.arange(H, dtype=np.int32), (b, 1))
            lists.add_compact(dev(idx), dev(np.where(mask[g:g + b], 1.0, -1.0).astype(np.float32)), tok)
        g += b
    offsets, tokens = lists.finish()
    assert offsets.dtype == torch.int64 and tokens.dtype == torch.int32
    assert offsets.device == tokens.device == torch.device(DEV)
    _check((host(offsets), host(tokens)), mask, flat_tok)
    assert token_lists_to_python(offsets, tokens) == [flat_tok[np.nonzero(mask[:, f])[0]].tolist() for f in range(H)]


def test_regroup_op_alone():
    ops = _ops()
    bo = torch.tensor([[0, 2, 2, 3], [0, 0, 1, 4], [0, 0, 0, 0]], dtype=torch.int64, device=DEV)
    seg = torch.tensor([10, 11, 12, 20, 21, 22, 23], dtype=torch.int32, device=DEV)
    offsets, tokens = ops.token_lists_regroup(bo, seg)
    assert host(offsets).tolist() == [0, 2, 3, 7] and host(tokens).tolist() == [10, 11, 20, 12, 21, 22, 23]


# ---- test 5: model level ------------------------------------------------------------------------------------------
def _wrap(name, model):
    return F.SAEWrapper(F.SAE_REGISTRY[name], model, DEV)


def _load(model, sd):
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return model.to(DEV).eval()


def _model(name):
    fx = Fixture(name)
    m, sd = fx.meta, fx.state_dict()
    if m["variant"] == "binary":
        model = _load(BinarySAE(m["D"], m["H"], gamma=m["gamma"], n_bits=m["n_bits"]), sd)
        model.k = m["k"] / m["H"]
        return _wrap("b_sae", model), fx.x()
    if m["variant"] == "baseline":
        return _wrap("baseline_sae", _load(BaselineSparseAutoencoder(m["D"], m["H"]), sd)), fx.x()
    if m["variant"] == "matryoshka":
        model = _load(QuantizedMatryoshkaSAE(m["D"], m["H"], 32, abs_range=m["abs_range"], n_bits=m["n_bits"]), sd)
        return _wrap("q_sae", model), fx.x()
    model = _load(ResidualQuantizedSAE(m["D"], m["H"], 32, abs_range=m["abs_range"], n_bits=m["n_bits"]), sd)
    return _wrap("rq_sae", model), fx.x()


def _edge_needs_padding():
    m = Fixture("matryoshka_edge").meta
    return QuantizedMatryoshkaSAE(m["D"], m["H"], 32, abs_range=m["abs_range"], n_bits=m["n_bits"]).decoder.needs_padding


MODEL_NAMES = ["binary_small", "baseline_small", "matryoshka_small", "residual_small"] + (
    ["matryoshka_edge"] if _edge_needs_padding() else [])
_stats_cache = {}


def _model_stats(name):
    """(mask, flat tokens, stats with_tokens="csr", stats with_tokens=True) of one fixture model, computed once"""
    if name not in _stats_cache:
        sae, x = _model(name)
        n = len(x)
        cut = max(1, n // 3)
        tpc = 3
        token_ids = torch.from_numpy(_token_ids(n, tpc))
        loader = [torch.from_numpy(x[:cut]), (torch.from_numpy(x[cut:]),)]       # two uneven batches, one a (tensor,) tuple
        mask = np.concatenate([A._activation_mask(sae, dev(x[:cut])).numpy(), A._activation_mask(sae, dev(x[cut:])).numpy()])
        kw = dict(token_ids=token_ids, tokens_per_context=tpc)
        st = {mode: A.analyze_dataset(sae, loader, with_tokens=mode, **kw) for mode in ("csr", True)}
        sep = A.compute_activation_stats(sae, loader, with_tokens="csr", **kw)
        _stats_cache[name] = (mask, token_ids.reshape(-1).numpy()[:n], st["csr"], st[True], sep)
    return _stats_cache[name]


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_csr_lists_equal_the_python_lists_and_the_restatement(name):
    mask, flat_tok, csr, lists, sep = _model_stats(name)
    H = mask.shape[1]
    assert mask.any()
    for st in (csr, sep):
        tpf = st["tokens_per_feature"]
        assert type(tpf) is tuple and len(tpf) == 2
        offsets, tokens = tpf
        assert offsets.dtype == torch.int64 and tokens.dtype == torch.int32
        assert offsets.device == tokens.device == torch.device(DEV)
        as_lists = token_lists_to_python(offsets, tokens)
        assert as_lists == lists["tokens_per_feature"]
        assert as_lists == [flat_tok[np.nonzero(mask[:, f])[0]].tolist() for f in range(H)]
        assert torch.equal((offsets[1:] - offsets[:-1]).cpu(), st["activation_counts"])
        assert torch.equal(st["activation_counts"], lists["activation_counts"])
        assert torch.equal(st["coactivation"], lists["coactivation"])
    assert csr["mse_final"] == pytest.approx(lists["mse_final"], rel=1e-12)


def test_csr_mode_forms_no_mask_and_calls_no_nonzero(monkeypatch):
    sae, x = _model("matryoshka_small")

    def boom(*a, **k):
        raise AssertionError("the bool mask was formed")
    monkeypatch.setattr(A, "_activation_mask", boom)
    monkeypatch.setattr(A, "_bits_to_mask", boom)
    monkeypatch.setattr(torch.Tensor, "nonzero", boom)
    st = A.compute_activation_stats(sae, [torch.from_numpy(x)], token_ids=torch.zeros((len(x), 1), dtype=torch.long),
                                    tokens_per_context=1, with_tokens="csr")
    offsets, _tokens = st["tokens_per_feature"]
    assert torch.equal((offsets[1:] - offsets[:-1]).cpu(), st["activation_counts"])


@pytest.mark.parametrize("a,b", [("binary_small", "matryoshka_small"), ("residual_small", "baseline_small")])
def test_jaccard_histogram_takes_the_csr_stats_as_they_are(a, b):
    csr_a, lists_a = _model_stats(a)[2:4]
    csr_b, lists_b = _model_stats(b)[2:4]
    got = jaccard_histogram(csr_a, csr_b, k_tokens=3)
    want = jaccard_histogram(lists_a, lists_b, k_tokens=3, device=DEV)
    assert torch.equal(got.counts.cpu(), want.counts.cpu()) and int(got.counts.sum()) > 0
    sets = top_token_sets(csr_a["tokens_per_feature"], csr_a["activation_counts"], 3)
    want_sets = top_token_sets(lists_a["tokens_per_feature"], lists_a["activation_counts"], 3)
    assert torch.equal(sets.tokens.cpu(), want_sets.tokens) and torch.equal(sets.sizes.cpu(), want_sets.sizes)


# ---- test 6: no [B, H] allocation -------------------------------------------------------------------------------
def test_bits_form_stays_below_a_byte_per_row_and_unit():
    """The bool mask of this batch alone is B * H bytes; results plus the row bitmap are about a quarter of that."""
    ops = _ops()
    B, H = 4096, 32768
    gen = torch.Generator(device=DEV).manual_seed(6)
    pre = torch.where(torch.rand((B, H), device=DEV, generator=gen) < 1.0 / 64, 1.0, -1.0)
    want_counts = (pre > 0).sum(0)
    z = ops.train_pre_bits(pre)                             # the existing packer: bit = pre above the sigmoid cutoff
    tok = dev(U.row_tokens(B))
    del pre
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    offsets, ws = ops.token_lists_count_bits(z, H)
    n = int(offsets[-1])
    tokens = ops.token_lists_fill(ws, offsets, tok, n)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"peak growth {grown} bytes, cap {B * H}, entries {n}")
    assert grown < B * H
    assert torch.equal(offsets[1:] - offsets[:-1], want_counts) and int(offsets[0]) == 0
    assert n == int(want_counts.sum()) == tokens.numel()
    # spot check of the lists themselves: the first and the last unit against the bits
    zh = host(z).view(np.uint32)
    for u in (0, H - 1):
        rows = np.nonzero((zh[:, u >> 5] >> (u & 31)) & 1)[0]
        assert np.array_equal(host(tokens[int(offsets[u]):int(offsets[u + 1])]), U.row_tokens(B)[rows])


# ---- dispatcher ops ----------------------------------------------------------------------------------------------
def test_torch_ops_match_and_pass_opcheck():
    import quantizedsae_amd.torch_ops as T
    rng = np.random.default_rng(12)
    B, words, H = 100, 3, 96
    bits = rng.random((B, 32 * words)) < 0.2
    z, tok = dev(U.pack(bits)), dev(U.row_tokens(B))
    index = dev(rng.permutation(H).astype(np.int32))
    offsets, ws = T.token_lists_count_bits(z, H, index)
    want_off, _ = _ops().token_lists_count_bits(z, H, index)
    assert torch.equal(offsets, want_off)
    n = int(offsets[-1])
    tokens = T.token_lists_fill(ws, offsets, tok, n)
    mask = np.zeros((B, H), bool)
    mask[:, host(index)] = bits
    _check((host(offsets), host(tokens)), mask, U.row_tokens(B))
    idx = dev(np.stack([rng.permutation(H)[:4] for _ in range(B)]).astype(np.int32))
    val = dev(rng.standard_normal((B, 4)).astype(np.float32))
    off2, ws2 = T.token_lists_count(idx, val, H)
    assert torch.equal(off2, _ops().token_lists_count(idx, val, H)[0])
    both = T.token_lists_regroup(torch.stack([offsets, offsets]), torch.cat([tokens, tokens]))
    assert torch.equal(both[0], 2 * offsets)
    torch.library.opcheck(torch.ops.qsae.token_lists_count_bits.default, (z, index, H))
    torch.library.opcheck(torch.ops.qsae.token_lists_count.default, (idx, val, H))
    torch.library.opcheck(torch.ops.qsae.token_lists_fill.default, (ws, offsets, tok, n))
    torch.library.opcheck(torch.ops.qsae.token_lists_regroup.default, (torch.stack([offsets, offsets]), torch.cat([tokens, tokens])))
