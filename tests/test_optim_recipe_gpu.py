"""The recipe around the Adam step on the MI355X (include/qsae_optim.h): the four entry points through the C ABI between the
guards of a GuardedArena, each twice on one workspace, with the read-only operands unchanged bit for bit and the outputs equal
to the numpy restatements of tests/optim_recipe_util.py; then the layers above -- optim.Adam(max_grad_norm=, ema_decay=),
BaselineSparseAutoencoder.project_decoder_grad and Trainer(grad_clip=, decoder_grad_projection=, ema_decay=) -- against a
manual loop made of the same forward and backward, ``grad.mul_(coef)`` with the restatement's coefficient and the plain
``optim.Adam.step()``: bit for bit.  "Bit for bit" as tests/optim_util.py defines it."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import optim_recipe_util as R
import optim_util as U
from guard_util import GuardedArena, poison_, snapshot, unchanged
from quantizedsae_amd import (BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, _lib, ops, optim,
                              synthetic as S, torch_ops)
from quantizedsae_amd.training import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SC = U.scalars()
OMD = R.one_minus(R.DECAY)
#: the entry points of qsae_optim.h that this file drives between guards (the ledger of tests/test_optim_recipe_host.py)
GUARDED = ("qsaeo_project_columns", "qsaeo_grad_norm", "qsaeo_adam_step", "qsaeo_adam_step_prefilter")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _twice(arena, call, inout, outs, read_only, check):
    """The call twice on the same buffers (inout restored, outputs poisoned again): return code 0, guards intact, read-only
    operands unchanged, then ``check``"""
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


# ---- kernel level: the C ABI between guards ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bulk_norm():
    ts = R.norm_case("bulk")
    return ts, float(R.grad_norm(ts, 1.0)[1].view(np.float64)[1])


def _norm_between_guards(ts, max_norm):
    arena = GuardedArena(DEV)
    T = len(ts)
    placed = [arena.from_tensor(torch.from_numpy(t), offset_bytes=4 if i == R.NORM_SHIFTED else 0) for i, t in enumerate(ts)]
    assert placed[R.NORM_SHIFTED].data_ptr() % 16 == 4
    counts = (C.c_int64 * T)(*[t.size for t in ts])
    ptrs = (C.c_void_p * T)(*[p.data_ptr() if p.numel() else 0 for p in placed])
    need = int(_lib.load().qsaeo_grad_norm_workspace_bytes(counts, T))
    assert need > 0
    ws = arena.tensor((need,), torch.uint8)
    coef, report = arena.tensor((1,), torch.float32), arena.tensor((R.HEAD + T,), torch.int64)
    want_coef, want = R.grad_norm(ts, max_norm)

    def check(run):
        assert R.same_report(host(report), want), run
        assert U.same_bits(host(coef), np.array([want_coef], np.float32)), run
    _twice(arena, lambda lib: lib.qsaeo_grad_norm(ptrs, counts, T, max_norm, _ptr(coef), _ptr(report), _ptr(ws), need, _stream()),
           [], [coef, report], placed, check)
    return float(host(coef)[0]), host(report)


@pytest.mark.parametrize("side", ["below", "above"])
def test_grad_norm_between_guards_equals_the_restatement(bulk_norm, side):
    ts, norm = bulk_norm
    coef, words = _norm_between_guards(ts, norm * (0.5 if side == "below" else 2.0))
    assert (words[3] == 1 and abs(coef - 0.5) < 1e-6) if side == "below" else (words[3] == 0 and coef == 1.0)
    # the front end: the same words
    got_coef, got = ops.grad_norm([dev(t) for t in ts], norm * (0.5 if side == "below" else 2.0))
    assert np.array_equal(host(got), words) and float(got_coef) == coef


@pytest.mark.parametrize("kind", ["zeros", "inf", "nan"])
def test_grad_norm_corners_between_guards(kind):
    coef, words = _norm_between_guards(R.norm_case(kind), 1.0)
    f = words.view(np.float64)
    if kind == "zeros":
        assert f[1] == 0.0 and coef == 1.0 and words[3] == 0
    elif kind == "inf":
        assert np.isinf(f[1]) and coef == 0.0 and words[3] == 1
    else:
        assert np.isnan(f[1]) and np.isnan(coef) and words[3] == 1


@pytest.mark.parametrize("case", R.PROJECT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_project_columns_between_guards_equals_the_restatement(case):
    D, H, ld = case
    W_np, G_np = R.project_case(D, H, ld)
    want = R.project_columns(W_np, G_np, H)
    arena = GuardedArena(DEV)
    W, G = arena.from_numpy(W_np), arena.from_numpy(G_np)

    def check(run):
        assert U.same_bits(host(G), want), run
    _twice(arena, lambda lib: lib.qsaeo_project_columns(_ptr(W), _ptr(G), D, H, ld, _stream()), [G], [], [W], check)
    got = host(G)
    assert np.array_equal(got[:, H:].view(np.uint32), G_np[:, H:].view(np.uint32))
    if H >= 8:
        assert np.isnan(got[:, 5]).all() and not np.isnan(got[:, [4, 6]]).any()
    # the front end on the live columns (a view with the row stride ld)
    G2 = dev(G_np)
    ops.project_columns(dev(W_np)[:, :H], G2[:, :H])
    assert U.same_bits(host(G2), want)


@pytest.mark.parametrize("n", U.ADAM_SIZES)
def test_recipe_step_between_guards_equals_the_restatement(n):
    case = U.adam_case(n)
    e_np = R.ema_case(n)
    lib = _lib.load()
    # every coefficient with and without the average on 16-byte loads; p one element off (element-wise loads) for two of them
    combos = [(coef, with_ema, 0) for coef in R.COEFS for with_ema in (False, True)] + [(0.25, True, 1), (None, False, 1)]
    for coef, with_ema, shift_p in combos:
        want = R.recipe_f32(*case, SC, coef, e_np if with_ema else None, OMD)
        arena = GuardedArena(DEV)
        p = arena.from_numpy(case[0]) if shift_p == 0 else arena.from_tensor(torch.from_numpy(case[0]), offset_bytes=4)
        g, m, v = (arena.from_numpy(a) for a in case[1:])
        e = arena.from_numpy(e_np) if with_ema else None
        c = arena.from_numpy(np.array([coef], np.float32)) if coef is not None else None

        def check(run):
            for name, got, w in zip("pmve", (p, m, v, e), want):
                assert (got is None and w is None) or U.same_bits(host(got), w), (n, coef, with_ema, shift_p, name, run)
        _twice(arena, lambda lib: lib.qsaeo_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, *SC, _ptr(c), _ptr(e),
                                                        float(OMD), _stream()),
               [p, m, v] + ([e] if with_ema else []), [], [g] + ([c] if c is not None else []), check)
    # neither stream: qsae_adam_step's output byte for byte, in both load widths
    for shift_g in (0, 1):
        a = [dev(np.concatenate([np.zeros(s, np.float32), x]))[s:] for x, s in zip(case, (0, shift_g, 0, 0))]
        b = [t.clone() for t in a]
        if shift_g:
            b[1] = dev(np.concatenate([np.zeros(1, np.float32), case[1]]))[1:]
        assert lib.qsaeo_adam_step(*map(_ptr, a), n, *SC, None, None, 0.0, _stream()) == 0
        assert lib.qsae_adam_step(*map(_ptr, b), n, *SC, _stream()) == 0
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_recipe_step_large():
    """2^24 + 5 with the coefficient and the average: 64-bit indexing, several grid-stride trips and a one-element tail"""
    n = 2 ** 24 + 5
    case = U.adam_case(n)
    e_np = R.ema_case(n)
    want = R.recipe_f32(*case, SC, 0.25, e_np, OMD)
    p, g, m, v = (dev(a) for a in case)
    e, c = dev(e_np), dev(np.array([0.25], np.float32))
    ops.adam_step_clipped(p, g, m, v, *SC, coef=c, ema=e, one_minus_decay=float(OMD))
    for name, got, w in zip("pmve", (p, m, v, e), want):
        assert U.same_bits(host(got), w), name
    assert U.same_bits(host(g), case[1])


@pytest.mark.parametrize("case", U.PREF_CASES, ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}")
def test_recipe_pair_between_guards_equals_the_step_then_pack_w(case):
    H, D, variant = case
    w, b = U.pref_case(H, D, variant)
    eW_np = R.ema_case(H * D).reshape(H, D)
    eb_np = R.ema_case(H) if b is not None else None
    for coef, with_ema in ((None, False), (0.25, False), (None, True), (0.25, True), (float("nan"), True)):
        W2, mW2, vW2, eW2 = R.recipe_f32(*w, SC, coef, eW_np if with_ema else None, OMD)
        b2 = R.recipe_f32(*b, SC, coef, eb_np if with_ema else None, OMD) if b is not None else None
        Wq_want, meta_want = U.pack_w(W2, b2[0] if b2 is not None else None)
        arena = GuardedArena(DEV)
        W, gW, mW, vW = (arena.from_numpy(a) for a in w)
        bias, gb, mb, vb = (arena.from_numpy(a) for a in b) if b is not None else (None,) * 4
        eW = arena.from_numpy(eW_np) if with_ema else None
        eb = arena.from_numpy(eb_np) if with_ema and b is not None else None
        c = arena.from_numpy(np.array([coef], np.float32)) if coef is not None else None
        Wq, meta = arena.tensor((H, D), torch.float16), arena.tensor((4,), torch.float32)

        def check(run):
            for name, got, want in zip(("W", "mW", "vW", "eW"), (W, mW, vW, eW), (W2, mW2, vW2, eW2)):
                assert (got is None and want is None) or U.same_bits(host(got), want), (coef, with_ema, name, run)
            if b is not None:
                for name, got, want in zip(("bias", "mb", "vb", "eb"), (bias, mb, vb, eb), b2):
                    assert (got is None and want is None) or U.same_bits(host(got), want), (coef, with_ema, name, run)
            assert U.same_bits(host(Wq), Wq_want), (coef, with_ema, run)
            for i in range(4):
                assert U.same_bits(host(meta)[i:i + 1], meta_want[i:i + 1]), (coef, with_ema, i, run)
            # and against the three-pass kernel on the updated values
            Wq2, meta2 = ops.prefilter_pack_w(W, bias)
            assert torch.equal(Wq.view(torch.int16), Wq2.view(torch.int16)) and torch.equal(meta.view(torch.int32), meta2.view(torch.int32))
        _twice(arena, lambda lib: lib.qsaeo_adam_step_prefilter(*map(_ptr, (W, gW, mW, vW, bias, gb, mb, vb)), H, D, *SC, _ptr(c),
                                                                  _ptr(eW), _ptr(eb), float(OMD), _ptr(Wq), _ptr(meta), _stream()),
               [t for t in (W, mW, vW, bias, mb, vb, eW, eb) if t is not None], [Wq, meta],
               [t for t in (gW, gb, c) if t is not None], check)


def test_dispatcher_ops_move_the_version_counters_of_what_they_write():
    p, g, m, v = (dev(a) for a in U.adam_case(100))
    e, c = dev(R.ema_case(100)), torch.ones(1, device=DEV)
    before = [t._version for t in (p, m, v, e, g, c)]
    torch.ops.qsae.adam_step_clipped(p, g, m, v, *SC, c, e, 0.001)
    assert [t._version for t in (p, m, v, e, g, c)] == [x + 1 for x in before[:4]] + before[4:]
    report = torch.empty(5, dtype=torch.int64, device=DEV)
    before = (c._version, report._version, g._version)
    torch.ops.qsae.grad_norm([g], 1.0, c, report)
    assert (c._version, report._version, g._version) == (before[0] + 1, before[1] + 1, before[2])
    W, G = torch.randn(8, 16, device=DEV), torch.randn(8, 16, device=DEV)
    before = (W._version, G._version)
    torch.ops.qsae.project_columns(W, G)
    assert (W._version, G._version) == (before[0], before[1] + 1)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.project_columns(torch.randn(8, 6, device=DEV), torch.randn(8, 6, device=DEV))
    with pytest.raises(ValueError, match="same memory"):
        ops.project_columns(W, W)
    with pytest.raises(ValueError, match="emab"):
        ops.adam_step_prefilter_clipped(W, G, G.clone(), G.clone(), None, None, None, None, *SC, emaW=W.clone(),
                                        emab=torch.zeros(8, device=DEV))


# ---- the layers above: three Trainer steps against the manual loop --------------------------------------------------------------
CONFIG = {"input_dim": 64, "n_bits": 4, "hidden_dim": 1024, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 32,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 256}


def _load(m, sd):
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return m.to(DEV)


def _model(sae_type):
    if sae_type == "b_sae":
        return _load(BinarySAE(64, 1024, gamma=4.0, n_bits=4),
                     S.binary_sae_params(41, 64, 1024, 4, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1))
    if sae_type == "baseline_sae":
        m = _load(BaselineSparseAutoencoder(64, 1024), S.baseline_sae_params(42, 64, 1024, bias_std=0.05))
        m.normalize_decoder_weights()
        return m
    return _load(QuantizedMatryoshkaSAE(64, 1024, 32, abs_range=1.5, n_bits=4), S.matryoshka_sae_params(62, 64, 1024, bias_std=0.1))


def _flat(outs):
    out = []
    for o in outs if isinstance(outs, (list, tuple)) else [outs]:
        out += list(o) if isinstance(o, (list, tuple)) else [o]
    return out


def _batches(steps=3):
    return [dev(S.activations(70 + i, 256, 64)) for i in range(steps)]


def _trainer(sae_type, model, tmp_path, **kw):
    return Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path), **kw)


class _ManualClip:
    """What the parent's means make of a clipped step, between the Trainer's zero_grad and step: the restatement's projection
    (when asked for) on the decoder gradient, the restatement's coefficient from a copy of the gradients, ``grad.mul_(coef)``,
    then the plain ``optim.Adam.step()``.  ``clip`` None: half the first step's norm."""

    def __init__(self, model, project=False, clip=None):
        self.model, self.project, self.clip = model, project, clip
        self.opt = optim.Adam(model.parameters(), lr=CONFIG["lr"], model=model)
        self.reports = []

    def zero_grad(self, set_to_none=True):
        self.opt.zero_grad(set_to_none=set_to_none)

    def step(self):
        if self.project:
            w = self.model.decoder.weight
            w.grad.copy_(dev(R.project_columns(host(w), host(w.grad), w.shape[1])))
        grads = [host(p.grad) for p in self.model.parameters() if p.grad is not None]
        if self.clip is None:
            self.clip = 0.5 * float(R.grad_norm(grads, 1.0)[1].view(np.float64)[1])
        coef, words = R.grad_norm(grads, self.clip)
        self.reports.append((coef, words))
        c = torch.tensor(float(coef), dtype=torch.float32, device=DEV)
        for p in self.model.parameters():
            if p.grad is not None:
                p.grad.mul_(c)
        self.opt.step()


def _assert_same_training_state(model, opt, ref_model, ref_opt):
    for (name, p), q in zip(model.named_parameters(), ref_model.parameters()):
        assert U.same_bits(host(p), host(q)), name
        for key in ("exp_avg", "exp_avg_sq"):
            assert U.same_bits(host(opt.state[p][key]), host(ref_opt.state[q][key])), (name, key)
        assert float(opt.state[p]["step"]) == float(ref_opt.state[q]["step"])


@pytest.mark.parametrize("sae_type,project", [("b_sae", False), ("baseline_sae", False), ("q_sae", False), ("baseline_sae", True)])
def test_clipped_trainer_steps_equal_the_manual_loop(sae_type, project, tmp_path):
    batches = _batches()
    ref_model = _model(sae_type)
    model = copy.deepcopy(ref_model)
    ref_trainer = _trainer(sae_type, ref_model, tmp_path)
    manual = _ManualClip(ref_model, project=project)
    for x in batches:
        ref_trainer._step(manual, x, False)
    assert manual.reports[0][1][3] == 1 and 0.4 < float(manual.reports[0][0]) <= 0.5           # the first step is clipped
    trainer = _trainer(sae_type, model, tmp_path, grad_clip=manual.clip, decoder_grad_projection=project)
    opt = trainer._make_optimizer()
    for x, (coef, words) in zip(batches, manual.reports):
        trainer._step(opt, x, False)
        assert R.same_report(host(opt.last_clip), words)                                       # the report, bit for bit
        rep = opt.clip_report()
        f = words.view(np.float64)
        assert rep.norm == f[1] and rep.coef == float(coef) and rep.clipped == bool(words[3]) and rep.per_tensor == tuple(f[R.HEAD:])
        # .grad is left unscaled: the report's per-tensor sums are those of the gradients still in place
        again, _ = R.grad_norm([host(p.grad) for p in model.parameters() if p.grad is not None], manual.clip)
        assert float(again) == float(coef)
    _assert_same_training_state(model, opt, ref_model, manual.opt)


def test_logging_steps_report_the_clip(tmp_path):
    model = _model("b_sae")
    seen = []
    trainer = _trainer("b_sae", model, tmp_path, grad_clip=1e-3, log_fn=seen.append, log_every=2)
    chunk = torch.from_numpy(S.activations(75, 1024, 64)).to(torch.float16).reshape(1, 1024, 64)
    torch.manual_seed(0)
    trainer.one_epoch(chunk)
    assert len(seen) == 2
    for m in seen:
        assert m["grad_norm"] > 1e-3 and 0 < m["grad_clip_coef"] < 1 and m["grad_clipped"] == 1
        assert abs(m["grad_clip_coef"] * (m["grad_norm"] + 1e-6) - 1e-3) < 1e-9


# ---- the moving average ------------------------------------------------------------------------------------------------------
def test_ema_follows_the_restatement_and_exchanges_with_the_weights(tmp_path):
    batches = _batches()
    model = _model("b_sae")
    trainer = _trainer("b_sae", model, tmp_path, ema_decay=R.DECAY)
    opt = trainer._make_optimizer()
    first = {name: host(p).copy() for name, p in model.named_parameters()}
    after = []
    plain_step = opt.step

    def step():
        plain_step()
        after.append({name: host(p).copy() for name, p in model.named_parameters()})
    opt.step = step
    lin = model.encoder.linear
    for i, x in enumerate(batches):
        if i == 2:                                             # the last step: a fresh optimizer, as every epoch has; the
            opt = trainer._make_optimizer()                    # Trainer's dict carries the averages over
            plain_step = opt.step
            opt.step = step
        trainer._step(opt, x, False)
        assert model._pref_cache.is_current((lin.weight, lin.bias))          # the encoder pair went the fused way
    for name, p in model.named_parameters():
        e = first[name]
        for snap in after:
            e = R.ema_f32(e, snap[name], OMD)
        assert U.same_bits(host(trainer.ema_state[p]), e), name
        assert opt.state[p]["ema"] is trainer.ema_state[p]
        assert not np.array_equal(e, host(p))
    x = batches[0]
    with torch.no_grad():
        before = [t.clone() for t in _flat(model(x))]
        weights = {name: host(p).copy() for name, p in model.named_parameters()}
        fresh = BinarySAE(64, 1024, gamma=4.0, n_bits=4)
        fresh.load_state_dict(trainer.ema_state_dict())
        fresh = fresh.to(DEV)
        want = _flat(fresh(x))
        with opt.ema_weights():
            inside = [t.clone() for t in _flat(model(x))]
            for name, p in model.named_parameters():           # and the averages hold the weights meanwhile
                assert U.same_bits(host(trainer.ema_state[p]), weights[name]), name
        back = _flat(model(x))
    for a, b in zip(inside, want):
        assert torch.equal(a, b)
    for a, b in zip(back, before):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(inside, before))
    for name, p in model.named_parameters():
        assert U.same_bits(host(p), weights[name]), name


# ---- derived state on the prefilter path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["binary", "baseline"])
def test_clipped_averaged_steps_leave_the_prefilter_state_of_the_new_weights(kind, monkeypatch):
    """The loop of tests/test_optim_gpu.py at its shape, with the clip and the average on: the fused route still leaves the
    fp16 copy of the new weights.  (Trainer's baseline_sae step ends in normalize_decoder_weights(), whose invalidate_packed()
    drops the encoder copies as well; the optimizer is driven directly here, as there.)"""
    import test_optim_gpu as OG
    counted = OG._Counted(torch_ops.prefilter_pack_w)
    monkeypatch.setattr(torch_ops, "prefilter_pack_w", counted)
    model = OG._topk_model(kind)
    lin = model.encoder.linear
    x = dev(S.activations(53, OG.B_PREF, OG.D_PREF))
    opt = optim.Adam(model.parameters(), lr=1e-3, model=model, max_grad_norm=1e-4, ema_decay=R.DECAY)
    for step in range(4):
        before = counted.n
        loss, outs = OG._train_outputs(kind, model, x)
        assert counted.n - before == (1 if step == 0 else 0), step          # zero calls after the first forward
        if step > 0:
            OG._assert_forward_equals_fresh(kind, model, x, outs)           # (the fresh model packs its own copy)
        if step == 3:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        assert opt.clip_report().clipped and "ema" in opt.state[lin.weight] and "ema" in opt.state[lin.bias]
        assert model._pref_cache.is_current((lin.weight, lin.bias))
        held = model._pref_cache.peek()
        Wq, meta = ops.prefilter_pack_w(lin.weight.detach(), lin.bias.detach())
        assert torch.equal(held["Wq"], Wq) and torch.equal(held["meta"], meta)


# ---- defaults --------------------------------------------------------------------------------------------------------------
RECIPE_OPS = ("project_columns", "grad_norm", "adam_step_clipped", "adam_step_prefilter_clipped")


@pytest.fixture
def recipe_calls(monkeypatch):
    calls = {name: 0 for name in RECIPE_OPS}

    def counting(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper
    for name in RECIPE_OPS:
        monkeypatch.setattr(torch_ops, name, counting(name, getattr(torch_ops, name)))
    return calls


def test_without_the_options_no_recipe_op_is_reached(recipe_calls, tmp_path):
    x = _batches(1)[0]
    for sae_type in ("b_sae", "baseline_sae", "q_sae"):
        model = _model(sae_type)
        trainer = _trainer(sae_type, model, tmp_path)
        opt = trainer._make_optimizer()
        for _ in range(2):
            trainer._step(opt, x, False)
        assert opt.last_clip is None and all("ema" not in st for st in opt.state.values())
    p = torch.nn.Parameter(torch.zeros(64, device=DEV))
    p.grad = torch.ones(64, device=DEV)
    optim.Adam([p]).step()
    assert recipe_calls == {name: 0 for name in RECIPE_OPS}
    # ... and the wrappers do count: every option reaches its op
    model = _model("baseline_sae")
    trainer = _trainer("baseline_sae", model, tmp_path, grad_clip=1.0, decoder_grad_projection=True, ema_decay=0.9)
    trainer._step(trainer._make_optimizer(), x, False)
    assert recipe_calls["project_columns"] == 1 and recipe_calls["grad_norm"] == 1
    assert recipe_calls["adam_step_prefilter_clipped"] == 1 and recipe_calls["adam_step_clipped"] >= 1
