"""Dictionaries wider than one selection kernel on the MI355X (include/qsae_wide.h, ``latent_path = "slabs"``): the three
device entry points through the C ABI between the guards of a GuardedArena, each twice on one poisoned workspace; the slab
path against the models' own ``"auto"`` path at shapes both take, bit for bit (lists, dense latent, reconstruction), at two
slab widths; models past the old limits against the dense exact encoder plus a sort, the CPU oracle and the sparse decoders;
training at hidden_dim = 65540 against the fp64 restatements, and Trainer steps that repeat bit for bit and leave the fp16
copy of the new weights; and one call each of the objectives that select through the same paths."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import wide_util as U
from guard_util import GuardedArena, poison_, snapshot, unchanged
from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, _lib, ops, synthetic as S
from quantizedsae_amd.inference.sparsity_curve import SparsityCurve
from quantizedsae_amd.training import BatchTopK, Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
#: the entry points of qsae_wide.h that this file drives between guards (the ledger of tests/test_wide_host.py)
GUARDED = ("qsaew_merge_topk", "qsaew_encode_topk", "qsaew_encode_topk_prefilter")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _twice(arena, call, inout, outs, read_only, check):
    """The call twice on the same buffers (inout restored and outputs poisoned again in between; the workspace, poisoned before
    the first call, keeps what that call left): return code 0, guards intact, read-only operands unchanged, then ``check``"""
    lib = _lib.load()
    saved = [t.clone() for t in inout]
    snap = snapshot(read_only)
    for run in ("first call", "second call on the same workspace"):
        if run != "first call":
            for t, s in zip(inout, saved):
                t.copy_(s)
            for t in outs:
                poison_(t)
        rc = call(lib)
        torch.cuda.synchronize()
        assert rc == 0, (run, rc, lib.qsae_last_error())
        assert arena.intact(), f"{run}: wrote outside its buffers"
        assert unchanged(snap), f"{run}: altered a read-only operand"
        check(run)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
NAN_ROW, NEG_ROW, TIE_ROW = 3, 5, 7


def encoder_inputs(seed, B, D, H, tie_units=None):
    """x [B, D], W [H, D], b [H] with the three awkward rows: NAN_ROW is all NaN (a flagged row wherever the prefilter runs),
    NEG_ROW has every pre-activation negative (column 0 of W is positive, the row is -100 e_0), and ``tie_units`` = (h1, h2)
    share one weight row and bias, which TIE_ROW points at -- a tie that must go to the lower unit."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((B, D), device=DEV, generator=g)
    bound = (6.0 / (D + H)) ** 0.5
    W = (torch.rand((H, D), device=DEV, generator=g) * 2 - 1) * bound
    b = torch.randn((H,), device=DEV, generator=g) * 0.05
    W[:, 0] = W[:, 0].abs() + bound
    if B > max(NAN_ROW, NEG_ROW, TIE_ROW):
        x[NAN_ROW] = float("nan")
        x[NEG_ROW] = 0.0
        x[NEG_ROW, 0] = -100.0
        if tie_units is not None:
            h1, h2 = tie_units
            W[h2] = W[h1]
            b[h2] = b[h1]
            x[TIE_ROW] = 50.0 * W[h1] / W[h1].norm()
    return x, W, b


# ---- 1. the C ABI between guards --------------------------------------------------------------------------------------------
def test_merge_between_guards_equals_the_restatement():
    S_, B, k = 3, 37, 65
    widths = [k + 2, 4 * k, k]
    starts = [0, widths[0], widths[0] + widths[1], sum(widths)]
    pidx_h, pval_h = U.part_lists(11, S_, B, k, U.KINDS, widths)
    ld = starts[-1] + 5
    dense_h = U.dense_before(pidx_h, pval_h, starts, ld)
    ridx, rval, rdense = U.merge_ref(pidx_h, pval_h, starts, dense_h)
    arena = GuardedArena(DEV)
    pidx, pval, dense = arena.from_numpy(pidx_h), arena.from_numpy(pval_h), arena.from_numpy(dense_h)
    idx, val = arena.tensor((B, k), torch.int32), arena.tensor((B, k), torch.float32)
    cstarts = (C.c_int * (S_ + 1))(*starts)

    def check(run):
        assert U.same_bits(host(idx), ridx) and U.same_bits(host(val), rval), run
        assert U.same_bits(host(dense), rdense), run          # losers +0, winners and every other element untouched

    _twice(arena, lambda lib: lib.qsaew_merge_topk(_ptr(pidx), _ptr(pval), S_, B, k, cstarts, _ptr(idx), _ptr(val), _ptr(dense), ld,
                                                   _stream()), [dense], [idx, val], [pidx, pval], check)
    # the front ends give the same bits, with and without a dense latent
    d2 = dev(dense_h)
    i2, v2 = ops.merge_topk_parts(dev(pidx_h), dev(pval_h), starts, d2)
    i3, v3 = torch.ops.qsae.merge_topk_parts(dev(pidx_h), dev(pval_h), starts, None)
    assert same(i2, idx) and same(v2, val) and same(d2, dense) and same(i3, idx) and same(v3, val)


def _encode_between_guards(prefilter, B, D, H, k, slab, want):
    lib = _lib.load()
    x_, W_, b_ = encoder_inputs(21, B, D, H, tie_units=(17, H - 9))
    arena = GuardedArena(DEV)
    x, W, b = arena.from_tensor(x_), arena.from_tensor(W_), arena.from_tensor(b_)
    read_only = [x, W, b]
    Wq = meta = None
    if prefilter:
        q, m = ops.prefilter_pack_w(W_, b_)
        Wq, meta = arena.from_tensor(q), arena.from_tensor(m)
        read_only += [Wq, meta]
    sizer = lib.qsaew_encode_topk_prefilter_workspace_bytes if prefilter else lib.qsaew_encode_topk_workspace_bytes
    need = int(sizer(B, D, H, k, slab))
    assert need > 0
    ws = arena.tensor((need,), torch.uint8)
    ld = H + 4
    idx, val, dense = arena.tensor((B, k), torch.int32), arena.tensor((B, k), torch.float32), arena.tensor((B, ld), torch.float32)
    widx, wval, wdense = want(x_, W_, b_)
    flagged = C.c_int(-1)

    def call(lib):
        if prefilter:
            return lib.qsaew_encode_topk_prefilter(_ptr(x), _ptr(W), _ptr(b), _ptr(Wq), _ptr(meta), B, D, H, k, slab, _ptr(idx), _ptr(val),
                                                   _ptr(dense), ld, _ptr(ws), need, 0, C.byref(flagged), _stream())
        return lib.qsaew_encode_topk(_ptr(x), _ptr(W), _ptr(b), B, D, H, k, slab, _ptr(idx), _ptr(val), _ptr(dense), ld, _ptr(ws), need,
                                     _stream())

    def check(run):
        assert same(idx, widx), run
        assert same(val, wval), run
        assert same(dense[:, :H], wdense), run               # every element: zeros, survivors, erased losers
        assert bool((dense[:, H:].contiguous().view(torch.uint8) == 0x5A).all()), run      # the pad columns are nobody's
        if prefilter:
            assert flagged.value >= 1, run                   # the NaN row, at least once
        assert int(idx[TIE_ROW, 0]) == 17 and int(idx[TIE_ROW, 1]) == H - 9, run

    _twice(arena, call, [], [idx, val, dense], read_only, check)       # the workspace keeps the first call's leftovers
    return idx, val


def test_encode_topk_between_guards_equals_the_one_piece_call():
    B, D, H, k, slab = 100, 64, 5124, 41, 2048              # three slabs, every one through the chunked form
    assert len(U.plan(H, k, slab)) == 4
    _encode_between_guards(False, B, D, H, k, slab, lambda x, W, b: ops.encode_topk_latent(x, W, b, k))


def test_encode_topk_prefilter_between_guards_equals_the_one_piece_call():
    B, D, H, k, slab = 2048, 64, 16384, 41, 8192            # two slabs of 8192: both through the fp16 prefilter
    assert ops.prefilter_supported(B, D, 8192, k) and ops.prefilter_supported(B, D, H, k)
    def want(x, W, b):
        Wq, meta = ops.prefilter_pack_w(W, b)
        return ops.encode_topk_prefilter(x, W, b, Wq, meta, k)
    idx, val = _encode_between_guards(True, B, D, H, k, slab, want)
    # ... and the exact entry point on the same shape (fused form per slab) gives the same lists
    x, W, b = encoder_inputs(21, B, D, H, tie_units=(17, H - 9))
    i2, v2, _ = ops.encode_topk_wide(x, W, b, k, slab=slab)
    assert same(i2, idx) and same(v2, val)


# ---- 2. equivalence with the existing paths ------------------------------------------------------------------------------------
def _binary(D, H, k, W, b, seed=1):
    with torch.device(DEV):
        m = BinarySAE(D, H, gamma=4.0, n_bits=4).eval()
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    with torch.no_grad():
        m.encoder.linear.weight.copy_(W)
        m.encoder.linear.bias.copy_(b)
        m.decoder.weight.bernoulli_(0.5, generator=g).mul_(60.0).sub_(30.0)       # polarised: the hard packed decode
        m.decoder.bias.normal_(0.0, 0.1, generator=g)
    m.k = (k + 0.5) / H
    assert m.top_k == k and m.decoder.resolved_decode_mode() == "hard"
    return m


def _baseline(D, H, k, W, b, seed=2):
    with torch.device(DEV):
        m = BaselineSparseAutoencoder(D, H).eval()
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    with torch.no_grad():
        m.encoder.linear.weight.copy_(W)
        m.encoder.linear.bias.copy_(b)
        m.decoder.weight.normal_(0.0, 0.05, generator=g)
        m.decoder.bias.normal_(0.0, 0.1, generator=g)
    m.topk = k
    return m


MAKE = {"binary": _binary, "baseline": _baseline}
EQUIV = [(20480, 128, 41, 2304), (32768, 64, 65, 100), (16384, 64, 33, 2048)]


@pytest.mark.parametrize("kind", ["binary", "baseline"])
@pytest.mark.parametrize("H,D,k,B", EQUIV, ids=[f"H{h}-D{d}-k{k}-B{b}" for h, d, k, b in EQUIV])
def test_slabs_equal_the_auto_path_bit_for_bit(kind, H, D, k, B):
    """slab widths 8192 and 4096 (at H = 20480: three ragged slabs of 6912, 6912 and 6656 units, then five) against "auto"
    (the forward in one prefilter call at the big batches, the in-place path at B = 100); at H = 16384 the slabs of 8192 go
    through the prefilter themselves"""
    tie = (100, H - 100)
    x, W, b = encoder_inputs(31, B, D, H, tie_units=tie)
    m = MAKE[kind](D, H, k, W, b)
    want_full = m(x)
    want_compact = m.forward_compact(x)
    assert m.resolved_latent_path(B) != "slabs"
    m.latent_path = "slabs"
    seen = []
    for width in (8192, 4096):
        m.slab_width = width
        full, compact = m(x), m.forward_compact(x)
        assert len(full) == len(want_full)
        for got, want in zip(full, want_full):               # the dense latent (every element), the reconstruction(, polarize)
            assert same(got, want), (width, got.shape)
        for got, want in zip(compact, want_compact):         # idx, val, reconstruction
            assert same(got, want), (width, got.shape)
        seen.append(compact)
    for a, c in zip(*seen):                                  # two slab widths, the same bits
        assert same(a, c)
    idx = want_compact[0]
    assert idx[NAN_ROW].tolist() == list(range(k))           # every key ties: the lowest units, over all slabs
    assert bool((want_compact[1][NEG_ROW] < 0).all())
    assert idx[TIE_ROW, :2].tolist() == list(tie)            # the tie across the first and the last slab goes to the lower unit


# ---- 3. past the old limits ------------------------------------------------------------------------------------------------------
def _check_selection(x, W, b, k, idx, val):
    import test_limits_gpu as L
    ridx, rval = L.ref_topk(x, W, b, k)
    assert torch.equal(idx, ridx), f"{int((idx != ridx).any(1).sum())} rows differ"
    assert same(val, rval)
    L.check_oracle_rows(x, W, b, k, idx, val, n=8)


@pytest.mark.parametrize("B", [2048, 100])
def test_binary_sae_of_65540_units(B):
    D, H, k = 64, 65540, 131
    x, W, b = encoder_inputs(41, B, D, H)
    x[NAN_ROW] = x[NAN_ROW + 1]                              # (the references below order finite rows)
    m = _binary(D, H, k, W, b)
    assert m.top_k == int(H * 0.002)
    with pytest.raises(ValueError, match="65536|32768"):
        m(x)
    m.latent_path = "slabs"
    latent, recon, _ = m(x)
    idx, val, recon_c = m.forward_compact(x)
    _check_selection(x, W, b, k, idx, val)
    dec = m.decoder
    want = ops.decode_binary_sparse(idx, val, dec.packed()["packed"], dec.out_features, dec.n_bits, dec.quantization_step,
                                    dec.bias.detach())
    assert same(recon, want) and same(recon_c, want)
    assert same(latent, ops.densify(idx, val, H))
    assert m.last_flagged_rows >= 0 and len(ops.wide_plan(H, k)) == 4


def test_baseline_sae_of_40960_units_at_a_small_batch():
    D, H, k, B = 64, 40960, 32, 100
    x, W, b = encoder_inputs(42, B, D, H)
    x[NAN_ROW] = x[NAN_ROW + 1]
    m = _baseline(D, H, k, W, b)
    with pytest.raises(ValueError, match="32768"):
        m(x)
    m.latent_path = "slabs"
    h, recon = m(x)
    idx, val, recon_c = m.forward_compact(x)
    _check_selection(x, W, b, k, idx, val)
    want = ops.decode_table_sparse(idx, val, m._table(), 1.0, m.decoder.bias.detach())
    assert same(recon, want) and same(recon_c, want) and same(h, ops.densify(idx, val, H))


def test_binary_sae_of_131072_units_with_k_lowered():
    D, H, k, B = 64, 131072, 100, 2048
    x, W, b = encoder_inputs(43, B, D, H)
    x[NAN_ROW] = x[NAN_ROW + 1]
    m = _binary(D, H, k, W, b)
    with pytest.raises(ValueError, match="65536"):
        m.forward_compact(x)
    m.latent_path = "slabs"
    m.k = 0.002
    with pytest.raises(ValueError, match="limit of 256"):
        m.forward_compact(x)
    m.k = (k + 0.5) / H
    idx, val, recon = m.forward_compact(x)
    _check_selection(x, W, b, k, idx, val)
    dec = m.decoder
    assert same(recon, ops.decode_binary_sparse(idx, val, dec.packed()["packed"], dec.out_features, dec.n_bits,
                                                dec.quantization_step, dec.bias.detach()))
    with pytest.raises(ValueError, match="not built for latent_path = 'slabs'"):
        m.forward_submit(x)


# ---- 4. training -----------------------------------------------------------------------------------------------------------------
CONFIG = {"input_dim": 64, "n_bits": 4, "hidden_dim": 65540, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 32,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 2048}
SAE_TYPE = {"binary": "b_sae", "baseline": "baseline_sae"}


def _train_model(kind, H, path, D=64):
    if kind == "binary":
        m = BinarySAE(D, H, gamma=4.0, n_bits=4)
        sd = S.binary_sae_params(51, D, H, 4, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1)
    else:
        m = BaselineSparseAutoencoder(D, H)
        sd = S.baseline_sae_params(52, D, H, bias_std=0.05)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    m.latent_path = path
    return m.to(DEV)


@pytest.mark.parametrize("kind", ["binary", "baseline"])
def test_forward_train_gradients_at_65540_units_against_fp64(kind):
    """the project's training tolerance: 1e-5 of the largest gradient entry, per tensor"""
    import test_train_baseline_gpu as TB
    import test_train_gpu as TG
    T = TG if kind == "binary" else TB
    model = _train_model(kind, 65540, "slabs")
    x = dev(S.activations(53, 2048, 64))
    with pytest.raises(ValueError):
        _train_model(kind, 65540, "auto").forward_train(x)
    got = T.train_step_grads(model, x)
    want = T.restated(model, x)
    errs = {key: T.U.max_rel_err(got[key].detach().cpu(), want[key]) for key in T.U.GRAD_KEYS}
    print(kind, " ".join(f"{k}: {e:.3g}" for k, e in errs.items()))
    for key, err in errs.items():
        assert err <= 1e-5, f"{key}: max |err| / max |g| = {err:.3g}"


def _trainer_steps(kind, model, tmp_path, batches, after_step=None):
    trainer = Trainer(CONFIG, SAE_TYPE[kind], False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path))
    opt = trainer._make_optimizer()
    if after_step is not None:                                # right behind the optimizer's step: the baseline's step sequence
        plain_step = opt.step                                 # goes on to normalise the decoder, which drops every derived copy

        def step(*a, **kw):
            out = plain_step(*a, **kw)
            after_step()
            return out
        opt.step = step
    for x in batches:
        trainer._step(opt, x, False)
    return {name: p.detach().clone() for name, p in model.named_parameters()}, opt


@pytest.mark.parametrize("kind", ["binary", "baseline"])
def test_trainer_steps_at_65540_units_repeat_and_keep_the_fp16_copy(kind, tmp_path):
    batches = [dev(S.activations(60 + i, 2048, 64)) for i in range(3)]
    first = _train_model(kind, 65540, "slabs")
    second = copy.deepcopy(first)
    lin = first.encoder.linear
    checked = []

    def after_step():
        assert first._pref_cache.is_current((lin.weight, lin.bias))
        held = first._pref_cache.peek()
        Wq, meta = ops.prefilter_pack_w(lin.weight.detach(), lin.bias.detach())
        assert torch.equal(held["Wq"], Wq) and same(held["meta"], meta)
        checked.append(1)

    a, opt_a = _trainer_steps(kind, first, tmp_path, batches, after_step)
    b, opt_b = _trainer_steps(kind, second, tmp_path, batches)
    assert len(checked) == 3
    for name in a:
        assert same(a[name], b[name]), name
    for p, q in zip(first.parameters(), second.parameters()):
        for key in ("exp_avg", "exp_avg_sq"):
            assert same(opt_a.state[p][key], opt_b.state[q][key])
    assert not same(a["encoder.0.weight"], _train_model(kind, 65540, "slabs").encoder.linear.weight)


@pytest.mark.parametrize("kind", ["binary", "baseline"])
def test_trainer_steps_under_slabs_equal_auto_at_20480_units(kind, tmp_path):
    batches = [dev(S.activations(70 + i, 2304, 64)) for i in range(3)]
    auto = _train_model(kind, 20480, "auto")
    slabs = copy.deepcopy(auto)
    slabs.latent_path, slabs.slab_width = "slabs", 8192
    assert auto.resolved_latent_path(2304) == "prefilter" and slabs.resolved_latent_path(2304) == "slabs"
    a, _ = _trainer_steps(kind, auto, tmp_path, batches)
    s, _ = _trainer_steps(kind, slabs, tmp_path, batches)
    for name in a:
        assert same(a[name], s[name]), name


# ---- 5. one call each of what selects through the same paths ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["binary", "baseline"])
def test_objectives_under_slabs_equal_auto(kind):
    D, H, k, B = 64, 4096, 16, 64
    x, W, b = encoder_inputs(81, B, D, H, tie_units=(5, H - 5))
    x[NAN_ROW] = x[NAN_ROW + 1]
    auto = MAKE[kind](D, H, k, W, b)
    slabs = copy.deepcopy(auto)
    slabs.latent_path, slabs.slab_width = "slabs", 1024
    assert len(ops.wide_plan(H, 64, 1024)) == 5

    def flat(outs):
        out = []
        for o in outs:
            out += list(o) if isinstance(o, (tuple, list)) else [o]
        return out

    bounds = [H // 4, H // 2, H]
    for name, run in (("forward_nested", lambda m: m.forward_nested(x, bounds)),
                      ("forward_multi_topk", lambda m: m.forward_multi_topk(x, [k, 4 * k])),
                      ("forward_batch_topk", lambda m: m.forward_batch_topk(x, BatchTopK(m, k=k, cap=4 * k)))):
        for got, want in zip(flat(run(slabs)), flat(run(auto))):
            assert same(got, want), name
    ks = [1, k // 2, k, 4 * k]
    results, recons = [], []
    for m in (slabs, auto):
        curve = SparsityCurve(m, ks)
        recon = torch.empty((len(ks), B, D), dtype=torch.float32, device=DEV)
        curve.add(x, recon_out=recon)
        results.append(curve.finish())
        recons.append(recon)
    assert same(recons[0], recons[1])
    assert np.array_equal(results[0]["sse"].view(np.uint64), results[1]["sse"].view(np.uint64))
