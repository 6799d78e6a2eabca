"""The optimizer step on the MI355X: both kernels against the numpy restatement bit for bit (tests/optim_util.py; "bit for bit"
as its docstring defines it), the fused call's (Wq, meta) against prefilter_pack_w of the updated values, the optimizer against
torch.optim.Adam on the same device with the fp64 restatement as the ruler, and the property the feature exists for: after a
step the top-k models' prefilter state is already that of the new weights, and every model's next forward equals that of a
fresh model loaded from the state dict.

Figures printed by test_optimizer_matches_the_restatement_and_torch_adam on an MI355X (10 steps, BinarySAE(64, 1024)):
see profiles/optim.txt."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optim_util as U
from quantizedsae_amd import (BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, TernarySparseAutoencoder, ops,
                              synthetic as S, torch_ops)
from quantizedsae_amd.optim import Adam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SC = U.scalars()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---- kernel level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", U.ADAM_SIZES + [2 ** 24 + 5])
def test_adam_step_equals_the_restatement(n):
    """2^24 + 5: 64-bit indexing, several grid-stride trips and a one-element tail."""
    case = U.adam_case(n)
    want = U.adam_f32(*case, SC)
    # all pointers aligned; p one element off its boundary; g one element off (the large case: aligned only)
    for shift_p, shift_g in ((0, 0), (1, 0), (0, 1)) if n < 2 ** 24 else ((0, 0),):
        p, g, m, v = (dev(np.concatenate([np.zeros(s, np.float32), a]))[s:] for a, s in zip(case, (shift_p, shift_g, 0, 0)))
        assert p.data_ptr() % 16 == 4 * shift_p and g.data_ptr() % 16 == 4 * shift_g
        ops.adam_step(p, g, m, v, *SC)
        for name, got, w in zip("pmv", (p, m, v), want):
            assert U.same_bits(host(got), w), (n, shift_p, shift_g, name)
        assert U.same_bits(host(g), case[1])


@pytest.mark.parametrize("case", U.PREF_CASES, ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}")
def test_adam_step_prefilter_equals_adam_then_pack_w(case):
    H, D, variant = case
    w, b = U.pref_case(H, D, variant)
    wwant, bwant, Wq_want, meta_want = U.pref_expected(w, b, SC)
    W, gW, mW, vW = (dev(a) for a in w)
    bq = tuple(dev(a) for a in b) if b is not None else (None,) * 4
    Wq, meta = ops.adam_step_prefilter(W, gW, mW, vW, *bq, *SC)
    for name, got, want in zip(("W", "mW", "vW"), (W, mW, vW), wwant):
        assert U.same_bits(host(got), want), name
    if b is not None:
        for name, got, want in zip(("bias", "mb", "vb"), (bq[0], bq[2], bq[3]), bwant):
            assert U.same_bits(host(got), want), name
    assert U.same_bits(host(Wq), Wq_want)
    for i in range(4):
        assert U.same_bits(host(meta)[i:i + 1], meta_want[i:i + 1]), (i, host(meta), meta_want)
    # and against the three-pass kernel on the updated values: the same bits, NaNs included
    Wq2, meta2 = ops.prefilter_pack_w(W, bq[0])
    assert torch.equal(bits(Wq), bits(Wq2)) and torch.equal(bits(meta), bits(meta2))
    if variant != "nan":
        assert torch.equal(Wq, Wq2) and torch.equal(meta, meta2)
    # into given buffers: the same result, no new tensors
    W, gW, mW, vW = (dev(a) for a in w)
    bq = tuple(dev(a) for a in b) if b is not None else (None,) * 4
    Wq3, meta3 = torch.full_like(Wq, 7.0), torch.full_like(meta, 7.0)
    out = ops.adam_step_prefilter(W, gW, mW, vW, *bq, *SC, Wq=Wq3, meta=meta3)
    assert out[0] is Wq3 and out[1] is meta3 and torch.equal(bits(Wq3), bits(Wq)) and torch.equal(bits(meta3), bits(meta))


def test_dispatcher_ops_move_the_version_counters():
    p, g, m, v = (dev(a) for a in U.adam_case(100))
    before = [t._version for t in (p, g, m, v)]
    torch.ops.qsae.adam_step(p, g, m, v, *SC)
    assert [t._version for t in (p, g, m, v)] == [before[0] + 1, before[1], before[2] + 1, before[3] + 1]
    w, b = U.pref_case(8, 64, "plain")
    W, gW, mW, vW = (dev(a) for a in w)
    bias, gb, mb, vb = (dev(a) for a in b)
    Wq, meta = torch.empty((8, 64), dtype=torch.float16, device=DEV), torch.empty(4, device=DEV)
    written, read = (W, mW, vW, bias, mb, vb, Wq, meta), (gW, gb)
    before = [t._version for t in written + read]
    torch.ops.qsae.adam_step_prefilter(W, gW, mW, vW, bias, gb, mb, vb, *SC, Wq, meta)
    assert [t._version for t in written + read] == [x + 1 for x in before[:8]] + before[8:]
    with pytest.raises(ValueError, match="together or not at all"):
        ops.adam_step_prefilter(W, gW, mW, vW, bias, None, mb, vb, *SC)
    with pytest.raises(ValueError, match="contiguous"):
        ops.adam_step(p[::2], g[::2], m[::2], v[::2], *SC)
    with pytest.raises(TypeError):
        ops.adam_step(p.double(), g, m, v, *SC)


# ---- the optimizer against torch's on the device --------------------------------------------------------------------------------
def _small_binary():
    m = BinarySAE(64, 1024, gamma=4.0, n_bits=4)
    sd = S.binary_sae_params(41, 64, 1024, 4, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _groups(sae, cls, **kw):
    enc = [sae.encoder.linear.weight, sae.encoder.linear.bias]
    rest = [p for p in sae.parameters() if all(p is not q for q in enc)]
    return cls([{"params": enc, "lr": 1e-3}, {"params": rest, "lr": 3e-3, "betas": (0.8, 0.99), "eps": 1e-6}], **kw)


def _group_of(name):
    return dict(lr=1e-3) if name.startswith("encoder") else dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6)


class _Ruler:
    """The restatement per tensor, in fp32 (what ours must equal) and in fp64 (the ruler), with each tensor's own step count."""

    def __init__(self, model, state=None):
        self.s32, self.s64, self.t = {}, {}, {}
        for name, p in model.named_parameters():
            z = np.zeros(p.shape, np.float32)
            m, v, t = (host(state[p]["exp_avg"]), host(state[p]["exp_avg_sq"]), int(state[p]["step"])) \
                if state is not None and p in state else (z, z, 0)
            self.s32[name] = (host(p).copy(), m.copy(), v.copy())
            self.s64[name] = tuple(a.astype(np.float64) for a in self.s32[name])
            self.t[name] = t

    def step(self, grads):
        for name, g in grads.items():
            self.t[name] += 1
            sc = U.scalars(t=self.t[name], **_group_of(name))
            a, b = self.s32[name], self.s64[name]
            self.s32[name] = U.adam_f32(a[0], g, a[1], a[2], sc)
            self.s64[name] = U.adam_f64(b[0], g, b[1], b[2], sc)

    def distance(self, model):
        return max(float(np.abs(host(p).astype(np.float64) - self.s64[name][0]).max()) for name, p in model.named_parameters())


def _fixed_grads(model, step, seed):
    """name -> gradient of this step; decoder.bias has none in odd steps"""
    rng = np.random.default_rng([seed, step])
    return {name: U.bulk_grad(rng, tuple(p.shape)) for name, p in model.named_parameters()
            if not (name == "decoder.bias" and step % 2 == 1)}


def _assign(model, grads):
    for name, p in model.named_parameters():
        p.grad = dev(grads[name]) if name in grads else None


def test_optimizer_matches_the_restatement_and_torch_adam():
    ours_m = _small_binary()
    theirs_m = copy.deepcopy(ours_m)
    ours, theirs = _groups(ours_m, Adam, model=ours_m), _groups(theirs_m, torch.optim.Adam, foreach=False)
    ruler = _Ruler(ours_m)
    lin = ours_m.encoder.linear
    for step in range(10):
        grads = _fixed_grads(ours_m, step, 5)
        _assign(ours_m, grads)
        _assign(theirs_m, grads)
        ours.step()
        theirs.step()
        ruler.step(grads)
        # the encoder pair went the fused way: the cache holds the state of the new weights
        assert ours_m._pref_cache.is_current((lin.weight, lin.bias))
    for name, p in ours_m.named_parameters():
        assert U.same_bits(host(p), ruler.s32[name][0]), name
        st = ours.state[p]
        assert U.same_bits(host(st["exp_avg"]), ruler.s32[name][1]) and U.same_bits(host(st["exp_avg_sq"]), ruler.s32[name][2])
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and int(st["step"]) == ruler.t[name]
        assert st["exp_avg"].device == p.device
    assert ruler.t["decoder.bias"] == 5 and ruler.t["encoder.0.weight"] == 10
    d_ours, d_theirs = ruler.distance(ours_m), ruler.distance(theirs_m)
    print(f"10 steps: max |ours - fp64| = {d_ours:.3e}, max |torch.optim.Adam(foreach=False) - fp64| = {d_theirs:.3e}, "
          f"ratio {d_ours / d_theirs:.3f}")
    assert d_theirs > 0 and d_ours <= 1.25 * d_theirs

    # a run switches optimizers at a checkpoint: torch's Adam continues from our state dict to the same parameters
    cont_m = copy.deepcopy(ours_m)
    cont = _groups(cont_m, torch.optim.Adam, foreach=False)
    cont.load_state_dict(copy.deepcopy(ours.state_dict()))      # (load_state_dict keeps same-device tensors as they are)
    ruler = _Ruler(ours_m, ours.state)
    for step in range(10, 13):
        grads = _fixed_grads(ours_m, step, 5)
        _assign(ours_m, grads)
        _assign(cont_m, grads)
        ours.step()
        cont.step()
        ruler.step(grads)
    d_ours, d_cont = ruler.distance(ours_m), ruler.distance(cont_m)
    apart = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(ours_m.parameters(), cont_m.parameters()))
    print(f"3 steps on from the checkpoint: max |ours - fp64| = {d_ours:.3e}, max |torch from our state dict - fp64| = "
          f"{d_cont:.3e}, max |ours - torch| = {apart:.3e}")
    assert d_cont > 0 and d_ours <= 1.25 * d_cont and apart <= d_ours + d_cont
    for name, p in ours_m.named_parameters():
        assert U.same_bits(host(p), ruler.s32[name][0]), name
    # and ours takes torch's state dict
    back = _groups(ours_m, Adam, model=ours_m)
    back.load_state_dict(copy.deepcopy(cont.state_dict()))
    assert int(back.state[lin.weight]["step"]) == 13 and torch.equal(back.state[lin.weight]["exp_avg"],
                                                                    cont.state[cont_m.encoder.linear.weight]["exp_avg"])


def test_non_contiguous_and_sparse_gradients():
    p = torch.nn.Parameter(torch.zeros(6, 4, device=DEV))
    opt = Adam([p], lr=1e-2)
    g = torch.arange(24, dtype=torch.float32, device=DEV).reshape(4, 6).t() + 1
    p.grad = g
    assert not p.grad.is_contiguous()
    opt.step()
    want = U.adam_f32(np.zeros((6, 4), np.float32), host(g), 0, 0, U.scalars(lr=1e-2, t=1))
    assert U.same_bits(host(p), want[0].reshape(6, 4))
    # an empty parameter with a gradient is stepped silently, as by torch.optim.Adam (its data_ptr() is 0)
    z = torch.nn.Parameter(torch.zeros(0, 4, device=DEV))
    z.grad = torch.zeros(0, 4, device=DEV)
    zopt = Adam([z])
    zopt.step()
    assert int(zopt.state[z]["step"]) == 1 and zopt.state[z]["exp_avg"].shape == (0, 4)
    e = torch.nn.Parameter(torch.zeros(6, 4, device=DEV))
    e.grad = torch.sparse_coo_tensor(torch.tensor([[1], [2]]), torch.tensor([1.0]), (6, 4)).to(DEV)
    with pytest.raises(RuntimeError, match="sparse"):
        Adam([e]).step()


# ---- derived state: what the feature is for ------------------------------------------------------------------------------------
B_PREF, D_PREF, H_PREF = 2048, 512, 8192          # the smallest shape both models send down the prefilter path


def _topk_model(kind, sd=None):
    if kind == "binary":
        m = BinarySAE(D_PREF, H_PREF, gamma=4.0, n_bits=4)
        sd = sd or S.binary_sae_params(51, D_PREF, H_PREF, 4, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1)
    else:
        m = BaselineSparseAutoencoder(D_PREF, H_PREF)
        sd = sd or S.baseline_sae_params(52, D_PREF, H_PREF, bias_std=0.05)
    m.load_state_dict({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in sd.items()})
    m.latent_path = "prefilter"
    m = m.to(DEV)
    assert m.resolved_latent_path(B_PREF) == "prefilter"          # so that this cannot pass on another path
    return m


def _train_outputs(kind, model, x):
    outs = model.forward_train(x)
    if kind == "binary":
        latent, recon, pol = outs
        return 0.5 * F.mse_loss(recon, x) + 1e-2 * pol, (latent, recon, pol)
    latent, recon = outs
    return F.mse_loss(recon, x), (latent, recon)


class _Counted:
    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *a, **kw):
        self.n += 1
        return self.fn(*a, **kw)


@pytest.fixture
def pack_w_calls(monkeypatch):
    counted = _Counted(torch_ops.prefilter_pack_w)
    monkeypatch.setattr(torch_ops, "prefilter_pack_w", counted)
    return counted


def _assert_forward_equals_fresh(kind, model, x, outs):
    fresh = _topk_model(kind, dict(model.state_dict()))
    with torch.no_grad():
        _, want = _train_outputs(kind, fresh, x)
    for got, w in zip(outs, want):
        assert torch.equal(got.detach(), w)
    assert model.last_flagged_rows == fresh.last_flagged_rows


@pytest.mark.parametrize("kind", ["binary", "baseline"])
def test_a_step_leaves_the_prefilter_state_of_the_new_weights(kind, pack_w_calls):
    model = _topk_model(kind)
    lin = model.encoder.linear
    x = dev(S.activations(53, B_PREF, D_PREF))
    opt = Adam(model.parameters(), lr=1e-3, model=model)
    buffers = None
    for step in range(5):
        before = pack_w_calls.n
        loss, outs = _train_outputs(kind, model, x)
        made = pack_w_calls.n - before
        # the forward after a fused step finds its fp16 copy; after the fallback step (3) it rebuilds it itself, once
        assert made == (1 if step in (0, 4) else 0), (step, made)
        if step > 0:
            _assert_forward_equals_fresh(kind, model, x, outs)
        if step == 4:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 3:
            lin.bias.grad = None                                   # a condition of the fused route fails in this step
        w_before = lin.weight.detach().clone()
        opt.step()
        assert not torch.equal(w_before, lin.weight)
        valid = model._pref_cache.is_current((lin.weight, lin.bias))
        assert valid == (step != 3)
        if valid:
            held = model._pref_cache.peek()
            Wq, meta = ops.prefilter_pack_w(lin.weight.detach(), lin.bias.detach())
            assert torch.equal(held["Wq"], Wq) and torch.equal(held["meta"], meta)
            # the buffers of the copy the first forward built take every later one: no allocation per step
            ptrs = (held["Wq"].data_ptr(), held["meta"].data_ptr())
            assert buffers in (None, ptrs)
            buffers = ptrs
    assert int(opt.state[lin.weight]["step"]) == 4 and int(opt.state[lin.bias]["step"]) == 3


@pytest.mark.parametrize("kind", ["binary", "baseline"])
def test_without_model_the_forward_rebuilds_the_copy_after_every_step(kind, pack_w_calls):
    model = _topk_model(kind)
    x = dev(S.activations(53, B_PREF, D_PREF))
    opt = Adam(model.parameters(), lr=1e-3)
    for step in range(4):
        before = pack_w_calls.n
        loss, outs = _train_outputs(kind, model, x)
        assert pack_w_calls.n - before == 1
        if step > 0:
            _assert_forward_equals_fresh(kind, model, x, outs)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()


def _ternary():
    m = TernarySparseAutoencoder(64, 256)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in S.ternary_sae_params(61, 64, 256).items()})
    m = m.to(DEV)
    m.decoder.init_mask(0.7)
    return m, dev(S.activations(61, 24, 64)), lambda x, outs: F.mse_loss(outs[1], x), \
        lambda sd: _loaded(TernarySparseAutoencoder(64, 256), sd)


def _matryoshka():
    m = QuantizedMatryoshkaSAE(64, 1024, 32, abs_range=1.5, n_bits=4)
    sd = S.matryoshka_sae_params(62, 64, 1024, bias_std=0.1)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return m.to(DEV), dev(S.activations(62, 256, 64)), \
        lambda x, outs: sum(0.5 * F.mse_loss(r, x) for r in outs[1]) + sum(outs[0]) * 1.5e-3, \
        lambda sd: _loaded(QuantizedMatryoshkaSAE(64, 1024, 32, abs_range=1.5, n_bits=4), sd)


def _loaded(m, sd):
    m.load_state_dict(sd)
    return m.to(DEV)


def _flat(outs):
    out = []
    for o in outs:
        out += list(o) if isinstance(o, (list, tuple)) else [o]
    return out


@pytest.mark.parametrize("make", [_ternary, _matryoshka], ids=["ternary", "matryoshka"])
def test_the_other_models_caches_follow_the_generic_route(make):
    """K-interleaved encoder copy, packed decoder: keyed on version counters, which the dispatcher op moves."""
    model, x, loss_fn, fresh_of = make()
    opt = Adam(model.parameters(), lr=1e-2, model=model)
    assert opt._model is None
    with torch.no_grad():
        first = [t.clone() for t in _flat(model(x))]
    for _ in range(3):
        loss = loss_fn(x, model.forward_train(x))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        with torch.no_grad():
            got, want = _flat(model(x)), _flat(fresh_of(model.state_dict())(x))
            got_t, want_t = _flat(model.forward_train(x)), _flat(fresh_of(model.state_dict()).forward_train(x))
        for a, b in zip(got + got_t, want + want_t):
            assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(first, got))
