"""Strongest activations per feature on the device (qsae_top_examples_*, inference/top_examples.py) against the numpy
restatement of tests/top_examples_util.py: collect every candidate (value > floor), sort by (feature, key descending),
keep n per feature.  Keys are integers, so every comparison is equal bits and nothing here has a tolerance."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import top_examples_util as U
from quantizedsae_amd import (BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, TernarySparseAutoencoder, _lib,
                              synthetic as S)
from quantizedsae_amd.inference import DictionaryInspector, TopExamples, examples_to_python
from quantizedsae_amd.inference import analysis as A
from quantizedsae_amd.inference import framework as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ukeys(t):
    return t.detach().cpu().numpy().view(np.uint64)


def _ops():
    from quantizedsae_amd import ops
    return ops


def fresh(H, n):
    return torch.zeros((H, n), dtype=torch.int64, device=DEV)


def run_compact(idx, val, H, n, cuts, floor=0.0, base=0, keys=None):
    ops = _ops()
    keys = fresh(H, n) if keys is None else keys
    for a, b in zip(cuts[:-1], cuts[1:]):
        ops.top_examples_compact(dev(idx[a:b]), None if val is None else dev(val[a:b]), floor, base + a, keys)
    return keys


def run_dense(lat, H, n, cuts, floor=0.0, base=0, keys=None):
    ops = _ops()
    keys = fresh(H, n) if keys is None else keys
    full = dev(lat)                                             # [B, ld]; the op reads the column slice in place
    for a, b in zip(cuts[:-1], cuts[1:]):
        ops.top_examples_dense(full[a:b, :H], floor, base + a, keys)
    return keys


_cases = {}


def compact_case(case):
    """(idx, val, restated keys) of one planted case, computed once and left unchanged"""
    if case not in _cases:
        B, k, H, n = case
        idx, val = U.compact_case(11 + B, B, k, H)
        _cases[case] = (idx, val, U.restate(H, n, *U.candidates_compact(idx, val, H)))
    return _cases[case]


# ---- compact form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.COMPACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_compact_form_equals_the_restatement(case):
    """(130, 2, 4, 64): lists longer than one 64-entry round at n = 64; (2100, 3, 64, 64): 66 bitmap words per unit, so
    the scan carries across a round.  Unit 0 fires in every row with ascending values (every candidate passes the
    running threshold), unit 1 descends, unit 2 ties at 0.5 (the lower position wins), unit H - 1 never fires."""
    B, k, H, n = case
    idx, val, want = compact_case(case)
    got = ukeys(run_compact(idx, val, H, n, [0, B]))
    assert np.array_equal(got, want)
    assert (want[H - 1] == 0).all() and want[0, 0] == U.full_key(val[B - 1:, 0], [B - 1])[0]
    if B >= n:
        assert np.array_equal(U.key_position(want[0]), np.arange(B - 1, B - 1 - n, -1))     # ascending: the last n rows
    if k >= 2 and H >= 4 and B >= 8:
        two = want[2][want[2] != 0]
        ties = U.key_value(two) == 0.5
        assert ties.sum() >= 2 and (np.diff(U.key_position(two[ties])) > 0).all()           # equal values: positions ascend


def test_fewer_candidates_than_n_leave_a_zero_tail():
    idx, val, want = compact_case((130, 2, 4, 64))
    got = ukeys(run_compact(idx, val, 4, 64, [0, 130]))
    filled = (got != 0).sum(1)
    assert filled[0] == 64 and 0 < filled[1] < 64 and filled[3] == 0
    for h in range(4):
        assert (got[h, :filled[h]] != 0).all() and (got[h, filled[h]:] == 0).all()
    v, p, c = _ops().top_examples_decode(dev(got.view(np.int64)))
    wv, wp, wc = U.decode(want)
    assert np.array_equal(v.cpu().numpy().view(np.int32), wv.view(np.int32))
    assert np.array_equal(p.cpu().numpy(), wp) and np.array_equal(c.cpu().numpy(), wc)
    assert p.dtype == torch.int64 and c.dtype == torch.int32 and (p.cpu().numpy()[3] == -1).all()


def test_without_values_every_in_range_entry_counts_at_one():
    B, k, H, n = 300, 65, 1024, 16
    idx, _, _ = compact_case((B, k, H, n))
    got = ukeys(run_compact(idx, None, H, n, [0, 100, B]))
    want = U.restate(H, n, *U.candidates_compact(idx, None, H))
    assert np.array_equal(got, want)
    assert np.array_equal(U.key_position(want[0]), np.arange(n))   # all values equal: the first n rows


@pytest.mark.parametrize("case", [(300, 65, 1024, 16), (2100, 3, 64, 64)], ids=lambda c: "x".join(map(str, c)))
def test_streaming_in_uneven_batches_gives_identical_keys(case):
    B, k, H, n = case
    idx, val, want = compact_case(case)
    cuts = U.splits(B, 7)
    assert len(cuts) == 8 and cuts[1] - cuts[0] == 1             # 7 batches, one of a single row
    assert np.array_equal(ukeys(run_compact(idx, val, H, n, cuts)), want)
    # the same rows in reverse batch order (positions kept): the result is a function of the set of pairs
    keys = fresh(H, n)
    for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
        run_compact(idx[a:b], val[a:b], H, n, [0, b - a], base=a, keys=keys)
    assert np.array_equal(ukeys(keys), want)


def test_a_second_dataset_continues_a_state_and_base_reaches_the_last_position():
    B, k, H, n = 300, 65, 1024, 16
    idx, val, want = compact_case((B, k, H, n))
    keys = run_compact(idx, val, H, n, [0, B])
    idx2, val2 = U.compact_case(77, 200, 9, H)
    run_compact(idx2, val2, H, n, [0, 64, 200], floor=0.25, base=5000, keys=keys)
    want2 = U.restate(H, n, *U.candidates_compact(idx2, val2, H, 5000, 0.25), old=want)
    assert np.array_equal(ukeys(keys), want2)
    assert (want2 != want).any() and (U.key_position(want2[want2 != 0]) < 300).any()      # both datasets are in the state
    base = 2 ** 32 - 200                                        # the last row sits at position 2^32 - 1
    want3 = U.restate(H, n, *U.candidates_compact(idx2, val2, H, base))
    assert np.array_equal(ukeys(run_compact(idx2, val2, H, n, [0, 64, 200], base=base)), want3)
    assert U.key_position(want3[0, :1])[0] == 2 ** 32 - 1


def _guarded(nbytes):
    g = 4096
    buf = torch.full((nbytes + 2 * g,), 0x5A, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + g, lambda: bool((buf[:g] == 0x5A).all() and (buf[g + nbytes:] == 0x5A).all())


def test_guard_words_and_repeated_calls_on_one_workspace():
    """Straight through the C ABI with 0x5A guards around keys, the workspace and the decoded outputs; the same
    workspace serves every call and is never cleared by the caller."""
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, k, H, n = 300, 65, 1024, 16
    idx, val, want = compact_case((B, k, H, n))
    d_idx, d_val = dev(idx), dev(val)
    need = lib.qsae_top_examples_compact_workspace_bytes(B, k, H)
    kbuf, kptr, kclean = _guarded(H * n * 8)
    wbuf, wptr, wclean = _guarded(need)
    for rep in range(2):                                        # the second pass finds the workspace as the first left it
        kbuf[4096:4096 + H * n * 8] = 0
        for a, b in [(0, 37), (37, 38), (38, B)]:
            rc = lib.qsae_top_examples_compact(d_idx[a:b].data_ptr(), d_val[a:b].data_ptr(), b - a, k, H, n, 0.0, a, kptr, wptr,
                                               need, stream)
            assert rc == 0, lib.qsae_last_error()
        torch.cuda.synchronize()
        assert kclean() and wclean()
        assert np.array_equal(kbuf[4096:4096 + H * n * 8].cpu().numpy().view(np.uint64).reshape(H, n), want)
    Bd, Hd, ld, nd = 200, 300, 304, 64
    lat = U.dense_case(21 + Bd, Bd, Hd, ld)
    d_lat = dev(lat)
    need = lib.qsae_top_examples_dense_workspace_bytes(Bd, Hd, nd)
    kbuf, kptr, kclean = _guarded(Hd * nd * 8)
    wbuf, wptr, wclean = _guarded(need)
    kbuf[4096:4096 + Hd * nd * 8] = 0
    for a, b in [(0, 130), (130, Bd)]:
        rc = lib.qsae_top_examples_dense(d_lat[a:b].data_ptr(), ld, b - a, Hd, nd, 0.0, a, kptr, wptr, need, stream)
        assert rc == 0, lib.qsae_last_error()
    outs = [_guarded(Hd * nd * 4), _guarded(Hd * nd * 8), _guarded(Hd * 4)]
    assert lib.qsae_top_examples_decode(kptr, Hd, nd, outs[0][1], outs[1][1], outs[2][1], stream) == 0
    torch.cuda.synchronize()
    assert kclean() and wclean() and all(o[2]() for o in outs)
    wantd = U.restate(Hd, nd, *U.candidates_dense(lat, Hd))
    assert np.array_equal(kbuf[4096:4096 + Hd * nd * 8].cpu().numpy().view(np.uint64).reshape(Hd, nd), wantd)
    assert np.array_equal(outs[2][0][4096:4096 + Hd * 4].cpu().numpy().view(np.int32), U.decode(wantd)[2])


# ---- dense form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.DENSE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dense_form_equals_the_restatement(case):
    """NaN sits at and past column H of every row (ld > H) and must not be read; column H - 1 never exceeds 0."""
    B, H, ld, n = case
    lat = U.dense_case(21 + B, B, H, ld)
    want = U.restate(H, n, *U.candidates_dense(lat, H))
    assert np.array_equal(ukeys(run_dense(lat, H, n, [0, B])), want)
    if B > 2:
        assert np.array_equal(ukeys(run_dense(lat, H, n, U.splits(B, 3))), want)
    if H >= 2:
        assert (want[H - 1] == 0).all()


def test_dense_floor_and_a_continued_state():
    B, H, ld, n = 193, 128, 128, 10
    lat = U.dense_case(5, B, H, ld)
    keys = run_dense(lat, H, n, [0, B], floor=0.5, base=1000)
    want = U.restate(H, n, *U.candidates_dense(lat, H, 1000, 0.5))
    assert np.array_equal(ukeys(keys), want)
    assert (U.key_value(want[want != 0]) > 0.5).all()
    lat2 = U.dense_case(6, B, H, ld)
    run_dense(lat2, H, n, [0, 1, B], floor=-0.25, base=2 ** 32 - B, keys=keys)
    want2 = U.restate(H, n, *U.candidates_dense(lat2, H, 2 ** 32 - B, -0.25), old=want)
    assert np.array_equal(ukeys(keys), want2)
    assert (U.key_value(want2[want2 != 0]) == 0).any()          # at a negative floor a zero is a candidate


def test_dense_of_the_densified_rows_equals_compact():
    B, k, H, n = 300, 65, 1024, 16
    idx, val, want = compact_case((B, k, H, n))
    lat = np.zeros((B, H), np.float32)
    ok = (idx >= 0) & (idx < H)
    rows = np.broadcast_to(np.arange(B)[:, None], idx.shape)
    lat[rows[ok], idx[ok]] = val[ok]                            # units are distinct within a row
    assert np.array_equal(ukeys(run_dense(lat, H, n, [0, 100, B])), want)


# ---- workload width ------------------------------------------------------------------------------------------------------
def test_workload_width_in_two_batches():
    B, k, H, n = 16384, 65, 32768, 16
    idx, val = U.compact_case(3, B, k, H)
    want = U.restate(H, n, *U.candidates_compact(idx, val, H))
    assert np.array_equal(ukeys(run_compact(idx, val, H, n, [0, 9000, B])), want)
    assert (want[:, 0] != 0).sum() > H // 2


# ---- dispatcher ops ------------------------------------------------------------------------------------------------------
def test_torch_ops_mutate_in_place_and_pass_opcheck():
    import quantizedsae_amd.torch_ops as T
    B, k, H, n = 37, 5, 33, 3
    idx, val, want = compact_case((B, k, H, n))
    keys = fresh(H, n)
    assert torch.ops.qsae.top_examples_compact(dev(idx), dev(val), 0.0, 0, keys) is None
    assert np.array_equal(ukeys(keys), want)
    assert "Tensor(a4!) keys" in str(torch.ops.qsae.top_examples_compact.default._schema)
    assert "Tensor(a3!) keys" in str(torch.ops.qsae.top_examples_dense.default._schema)
    lat = U.dense_case(4, 65, H, H + 3)
    kd = T.top_examples_dense(dev(lat)[:, :H], 0.0, 0, fresh(H, n))
    assert np.array_equal(ukeys(kd), U.restate(H, n, *U.candidates_dense(lat, H)))
    out = torch.ops.qsae.top_examples_decode(keys)
    assert all(torch.equal(a, b) for a, b in zip(out, _ops().top_examples_decode(keys)))
    torch.library.opcheck(torch.ops.qsae.top_examples_compact.default, (dev(idx), dev(val), 0.0, 0, fresh(H, n)))
    torch.library.opcheck(torch.ops.qsae.top_examples_compact.default, (dev(idx), None, 0.0, 5, fresh(H, n)))
    torch.library.opcheck(torch.ops.qsae.top_examples_dense.default, (dev(lat[:, :H]), 0.0, 0, fresh(H, n)))
    torch.library.opcheck(torch.ops.qsae.top_examples_decode.default, (keys,))
    with pytest.raises(ValueError, match="keys"):
        _ops().top_examples_compact(dev(idx), dev(val), 0.0, 0, torch.zeros((H, 65), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="latent"):
        _ops().top_examples_dense(dev(lat), 0.0, 0, fresh(H, n))


# ---- model level ---------------------------------------------------------------------------------------------------------
def _wrap(name, model):
    return F.SAEWrapper(F.SAE_REGISTRY[name], model, DEV)


def _load(model, sd):
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return model.to(DEV).eval()


@pytest.mark.parametrize("variant", ["binary", "baseline"])
def test_analyze_dataset_collects_the_models_own_strongest_activations(variant):
    D, H, n, tpc = 64, 1024, 8, 5
    if variant == "binary":
        model = _load(BinarySAE(D, H, gamma=4.0, n_bits=4), S.binary_sae_params(31, D, H, 4, enc_bias_std=0.1))
        model.k = 16 / H                                        # the default 0.002 would keep two units per row
        sae = _wrap("b_sae", model)
    else:
        sae = _wrap("baseline_sae", _load(BaselineSparseAutoencoder(D, H), S.baseline_sae_params(32, D, H, bias_std=0.1)))
    x = S.activations(33, 230, D)
    cuts = [0, 1, 131, 230]                                     # three uneven batches
    loader = [torch.from_numpy(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    token_ids = torch.arange(1000, 1000 + 46 * tpc).reshape(46, tpc)
    kw = dict(token_ids=token_ids, tokens_per_context=tpc, coactivation=None)
    st = A.analyze_dataset(sae, loader, with_tokens="csr", top_examples=n, **kw)
    feats, keys = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        idx, val, _ = sae.model.forward_compact(dev(x[a:b]))
        f, kk = U.candidates_compact(idx.cpu().numpy(), val.cpu().numpy(), H, a)
        feats.append(f)
        keys.append(kk)
    want = U.restate(H, n, np.concatenate(feats), np.concatenate(keys))
    wv, wp, wc = U.decode(want)
    te = st["top_examples"]
    assert np.array_equal(te["values"].cpu().numpy().view(np.int32), wv.view(np.int32))
    assert np.array_equal(te["positions"].cpu().numpy(), wp) and np.array_equal(te["counts"].cpu().numpy(), wc)
    assert wc.max() == n
    assert torch.equal(torch.minimum(st["activation_counts"], torch.tensor(n)), te["counts"].cpu().long())
    sep = A.compute_activation_stats(sae, loader, with_tokens="csr", top_examples=n, **kw)["top_examples"]
    assert all(torch.equal(sep[key], te[key]) for key in ("values", "positions", "counts"))
    plain = A.analyze_dataset(sae, loader, with_tokens="csr", **kw)
    assert set(plain) == set(st) - {"top_examples"} and torch.equal(plain["activation_counts"], st["activation_counts"])
    py = examples_to_python(te, token_ids, tpc)
    f = int(np.argmax(wc))
    assert len(py) == H and [e[0] for e in py[f]] == wv[f, :wc[f]].tolist()
    assert all(e[3] == 1000 + e[1] * tpc + e[2] and e[1] * tpc + e[2] == int(p) for e, p in zip(py[f], wp[f]))


def test_threshold_models_have_no_magnitude_to_rank_by():
    q = _wrap("q_sae", _load(QuantizedMatryoshkaSAE(64, 1024, top_k=8, abs_range=4, n_bits=4), S.matryoshka_sae_params(5, 64, 1024)))
    kw = dict(token_ids=torch.zeros((64, 1), dtype=torch.long), tokens_per_context=1)
    for fn in (A.analyze_dataset, A.compute_activation_stats):
        with pytest.raises(TypeError, match="one bit per unit"):
            fn(q, [torch.from_numpy(S.activations(1, 64, 64))], top_examples=8, **kw)


def _ternary():
    D, H = 64, 1024
    sd = S.ternary_sae_params(41, D, H)
    sd["encoder.0.bias"] = sd["encoder.0.bias"] - np.float32(0.2)          # every bias below zero: a zero input row is all <= 0
    assert (sd["encoder.0.bias"] < 0).all()
    model = _load(TernarySparseAutoencoder(D, H), sd)
    lines, tokens = 7, 19
    x = S.activations(42, lines * tokens, D)
    x[5] = 0.0                                                  # pre-activation = bias < 0 everywhere
    x[20] = x[3]
    return model, torch.from_numpy(x).reshape(lines, tokens, D), lines, tokens


def test_inspector_top_examples_of_the_ternary_model_equal_topk_of_its_latent():
    model, data, lines, tokens = _ternary()
    n = 6
    ins = DictionaryInspector(model)
    res = ins.top_examples(data, n)
    lat = model.encoder(data.reshape(lines * tokens, -1).to(DEV))
    assert not (lat[5] > 0).any() and (lat > 0).any()
    tv, _ = torch.topk(lat.t().contiguous(), n, dim=1)          # values only: torch.topk leaves the order of ties open
    got_v = res["values"]
    assert torch.equal(got_v, torch.where(tv > 0, tv, torch.zeros_like(tv)))
    want = U.restate(lat.shape[1], n, *U.candidates_dense(lat.cpu().numpy(), lat.shape[1]))   # ties: the lower position
    wv, wp, wc = U.decode(want)
    assert np.array_equal(res["positions"].cpu().numpy(), wp) and np.array_equal(res["counts"].cpu().numpy(), wc)
    # rows 3 and 20 are the same input: wherever both are kept with equal values, 3 comes first
    p = res["positions"].cpu().numpy()
    both = [(list(r).index(3), list(r).index(20)) for r in p if 3 in r and 20 in r]
    assert both and all(a + 1 == b for a, b in both)
    # a list of contexts, as the reference walks its dataset, gives the same state
    res2 = ins.top_examples([c for c in data], n)
    assert all(torch.equal(res[key], res2[key]) for key in res)
    with pytest.raises(TypeError, match="not from atoms"):
        DictionaryInspector(ins.atoms).top_examples(data, n)


def test_linguistic_analyze_is_the_argmax_of_the_dense_latent():
    model, data, lines, tokens = _ternary()
    ins = DictionaryInspector(model)
    fa = ins.linguistic_analyze(data)
    lat = model.encoder(data.reshape(lines * tokens, -1).to(DEV))
    want = torch.max(lat, dim=1).indices.reshape(lines, tokens)
    assert fa.shape == (lines, tokens) and fa.dtype == torch.int64 and torch.equal(fa, want)
    assert fa.reshape(-1)[5] == 0 and not (lat[5] > 0).any()    # an all-nonpositive row: index 0, as argmax of zeros
    assert torch.equal(ins.linguistic_analyze([c for c in data]), fa)
    ov = ins.print_feature_activations_overview(fa)
    flat = fa.reshape(-1).cpu().numpy()
    assert np.array_equal(ov.counts.cpu().numpy(), np.bincount(flat, minlength=lat.shape[1]))
    assert np.array_equal(ov.positions.cpu().numpy(), np.argsort(flat, kind="stable"))
    d = ov.to_python()
    assert sum(e["cnt"] for e in d.values()) == lines * tokens and d[0]["pos"][0] <= (0, 5)


def test_overview_on_the_device_equals_the_reference():
    z = np.load(ROOT / "tests" / "golden" / "inspector_overview.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    ins = DictionaryInspector(torch.zeros((meta["H"], 32), dtype=torch.int8, device=DEV))
    fa = z["feature_activations"]
    for table in (fa.tolist(), torch.from_numpy(fa), dev(fa)):
        ov = ins.print_feature_activations_overview(table)
        assert np.array_equal(ov.counts.cpu().numpy(), z["counts"]) and np.array_equal(ov.offsets.cpu().numpy(), z["offsets"])
        assert np.array_equal(ov.positions.cpu().numpy(), z["positions"])
    for i, (f, _targets) in enumerate(meta["pairs"]):
        m = dev(z["match_masks"][i])
        assert ins.check_sensitivity(dev(fa), m, f) == z["sensitivity"][i]
        assert ins.check_specificity(ov, m, f) == z["specificity"][i]
