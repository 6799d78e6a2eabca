"""QuantizedMatryoshkaSAE / ResidualQuantizedSAE.forward_train, their HIP backward (csrc/train_gemm.hip, csrc/train.hip) and
apply_secant_grad() on the MI355X: the reference's own gradients, forward parity with forward() on every bits path, the full
size against the fp64 restatement, both decoder-gradient paths, determinism, edge shapes, missing incoming gradients and the
reference trainer's q_sae / rq_sae loops."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantizedsae_amd import QuantizedMatryoshkaSAE, ResidualQuantizedSAE, synthetic as S

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_matryoshka_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5          # max |err| / max |g| per tensor: the project's training tolerance (test_train_gpu.py, test_train_baseline_gpu.py)
LAM = 1.5e-3
GRAD_PATHS = ("dense", "lists")


def _load(m, sd):
    m.load_state_dict({name: torch.from_numpy(np.ascontiguousarray(v)) for name, v in sd.items()})
    return m.to(DEV)


def make_q(sd, D, H, n_bits=4, allow_bias=True, grad_path="auto", bits_path="auto"):
    m = QuantizedMatryoshkaSAE(D, H, 32, abs_range=U.ABS_RANGE, n_bits=n_bits, allow_bias=allow_bias)
    m.decoder_grad_path, m.bits_path = grad_path, bits_path
    return _load(m, sd)


def make_rq(sd, D, H, n_bits=4, grad_path="auto"):
    m = ResidualQuantizedSAE(D, H, 32, abs_range=U.ABS_RANGE, n_bits=n_bits)
    for s in m.saes:
        s.decoder_grad_path = grad_path
    return _load(m, sd)


def q_loss(x, groups, levels, lam=LAM):
    """the q_sae branch of the reference trainer"""
    return sum(0.5 * F.mse_loss(r, x) for r in levels) + sum(groups) * lam


def rq_loss(x, groups, levels, lam=LAM):
    """the rq_sae branch of the reference trainer"""
    residual, rec, sp = x, [], 0
    for i, r in enumerate(levels):
        rec.append(0.5 * F.mse_loss(r, residual))
        residual = (residual - r).detach() * 2
        sp = sp + groups[i] * lam * U.RQ_STAGE_WEIGHTS[i]
    return sum(rec) + sp


def grads_of(model):
    return {name: (p.grad.detach().clone() if p.grad is not None else None) for name, p in model.named_parameters()}


def gpu_z(model, x):
    """bool [B, H] in the parameters' order: the z bits forward() uses"""
    dec = model.decoder
    with torch.no_grad():
        zb = model.activation_bits(x, "dense")
    return U.unpack_bits(zb, model.hidden_dim, dec.padded_index(DEV) if dec.needs_padding else None)


def restated(model, x, levels, lam=LAM, units=None, want_dx=False, G=None, gg=None):
    """fp64 gradients (train_matryoshka_util, on the GPU in fp64) of the q_sae loss on the GPU's own z bits and levels."""
    lin, dec = model.encoder.linear, model.decoder
    if G is None and gg is None:
        G, gg = U.trainer_incoming(x.detach(), torch.stack([l.detach() for l in levels]), model.n_bits, lam)
    g = U.grads64(x.detach(), lin.weight, lin.bias, dec.weight, dec.weight_mirror, gpu_z(model, x.detach()), G, gg,
                  model.n_bits, model.allow_bias, units=units, want_dx=want_dx)
    if want_dx and G is not None:
        g["x"] = g["x"] - G.sum(0)          # the loss also reads x directly: d/dx of 0.5 mse(result[i], x)
    return g


def assert_close(got: dict, want: dict, keys, tol=TOL, what="", units=None):
    errs = {}
    for key in keys:
        g = got[key]
        if units is not None and key != "decoder.bias" and key != "x":
            g = g[units.to(g.device)]
        errs[key] = U.max_rel_err(g, want[key])
    print(what, " ".join(f"{k}: {e:.3g}" for k, e in errs.items()))
    for key, err in errs.items():
        assert err <= tol, f"{what} {key}: max |err| / max |g| = {err:.3g}"


def step(model, x, lam=LAM, loss_fn=q_loss):
    model.zero_grad(set_to_none=True)
    groups, levels = model.forward_train(x)
    loss = loss_fn(x, groups, levels, lam)
    loss.backward()
    return loss, groups, levels


def check_step(model, x, what, units=None, want_dx=False):
    """one trainer step against the fp64 table, before and after apply_secant_grad()"""
    x = x.clone().requires_grad_(want_dx)
    _, _, levels = step(model, x)
    got = grads_of(model)
    want = restated(model, x, levels, units=units, want_dx=want_dx)
    keys = [k for k in U.PARAM_KEYS if not (k == "decoder.bias" and not model.allow_bias)]
    if want_dx:
        got["x"] = x.grad
        keys.append("x")
    assert_close(got, want, keys, what=what, units=units)
    model.decoder.apply_secant_grad()
    sec = grads_of(model)
    assert_close(sec, {k: want["secant." + k] for k in ("decoder.weight", "decoder.weight_mirror")},
                 ("decoder.weight", "decoder.weight_mirror"), what=what + " secant", units=units)
    return got, want


# ---- the reference's gradients -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_path", GRAD_PATHS)
@pytest.mark.parametrize("name", sorted(n for n, c in U.CASES.items() if c["kind"] == "q"))
def test_gradients_match_reference_fixtures(name, grad_path):
    meta, z = U.load_fixture(name)
    sd, x_np = U.case_inputs(meta, meta["seed"])
    model = make_q(sd, meta["D"], meta["H"], meta["n_bits"], meta["allow_bias"], grad_path)
    x = torch.from_numpy(x_np).to(DEV)
    want_z = np.unpackbits(z["z.0"], axis=1, bitorder="little")[:, :meta["H"]].astype(bool)
    assert np.array_equal(gpu_z(model, x).cpu().numpy(), want_z), "z bits differ from the reference"
    loss, groups, levels = step(model, x, meta["lam"])
    assert model.last_decoder_grad_path == grad_path
    assert abs(loss.item() - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    got = grads_of(model)
    keys = list(U.PARAM_KEYS)
    if not meta["allow_bias"]:
        assert got["decoder.bias"] is None and z["grad.decoder.bias"].size == 0
        keys.remove("decoder.bias")
    assert_close(got, {k: z["grad." + k] for k in keys}, keys, what=f"{name} {grad_path}")
    model.decoder.apply_secant_grad()
    sec = grads_of(model)
    keys = ("decoder.weight", "decoder.weight_mirror")
    assert_close(sec, {k: z["secant." + k] for k in keys}, keys, what=f"{name} {grad_path} secant")
    for k in ("encoder.0.weight", "encoder.0.bias"):
        assert torch.equal(sec[k], got[k])


@pytest.mark.parametrize("grad_path", GRAD_PATHS)
def test_residual_gradients_match_reference_fixture(grad_path):
    name = "train_matryoshka_residual"
    meta, z = U.load_fixture(name)
    sd, x_np = U.case_inputs(meta, meta["seed"])
    model = make_rq(sd, meta["D"], meta["H"], meta["n_bits"], grad_path)
    x = torch.from_numpy(x_np).to(DEV)
    loss, groups, levels = step(model, x, meta["lam"], rq_loss)
    residual = x
    for i, sae in enumerate(model.saes):
        want_z = np.unpackbits(z[f"z.{i}"], axis=1, bitorder="little")[:, :sae.hidden_dim].astype(bool)
        assert np.array_equal(gpu_z(sae, residual).cpu().numpy(), want_z), f"stage {i}: z bits differ from the reference"
        residual = (residual - levels[i].detach()) * 2
    assert abs(loss.item() - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    got = grads_of(model)
    for i in range(1, meta["n_bits"]):
        assert got.pop(f"saes.{i}.decoder.bias") is None and z[f"grad.saes.{i}.decoder.bias"].size == 0
    keys = sorted(got)
    assert_close(got, {k: z["grad." + k] for k in keys}, keys, what=f"{name} {grad_path}")
    model.apply_secant_grad()
    sec = grads_of(model)
    keys = [k for k in keys if k.endswith("decoder.weight") or k.endswith("decoder.weight_mirror")]
    assert_close(sec, {k: z["secant." + k] for k in keys}, keys, what=f"{name} {grad_path} secant")


# ---- forward parity -------------------------------------------------------------------------------------------------------
def _resolved_paths(model, B):
    seen = []
    for p in ("auto", "dense", "prefilter", "band"):
        model.bits_path = p
        r = model.resolved_bits_path(B)
        if (p, r) not in seen:
            seen.append((p, r))
    return [p for p, _ in seen]


@pytest.mark.parametrize("sigmas", [-2.5, 0.0], ids=["sparse", "dense"])
@pytest.mark.parametrize("B,H", [(96, 2048), (8192, 32768)])
def test_forward_train_outputs_equal_forward(B, H, sigmas):
    D, n = 512, 4
    model = make_q(U.q_params(721, D, H, sigmas), D, H, n)
    x = torch.from_numpy(S.activations(721, B, D)).to(DEV)
    for path in _resolved_paths(model, B):
        model.bits_path = path
        for _ in range(2):                                   # the second round after "auto" has seen this batch's density
            groups, levels = model(x)
            tg, tl = model.forward_train(x)
            assert all(t.grad_fn is not None for t in tg + tl)
            for a, b in zip(groups + levels, tg + tl):
                assert a.shape == b.shape and torch.equal(a, b.detach()), f"bits_path {path}"


def test_residual_forward_train_outputs_equal_forward():
    for B, H in [(96, 2048), (8192, 32768)]:
        D, n = 512, 4
        model = make_rq(U.rq_params(722, D, H, n, -2.5), D, H, n)
        x = torch.from_numpy(S.activations(722, B, D)).to(DEV)
        groups, levels = model(x)
        tg, tl = model.forward_train(x)
        assert len(tg) == len(tl) == n and all(t.grad_fn is not None for t in tg + tl)
        for a, b in zip(groups + levels, tg + tl):
            assert torch.equal(a, b.detach())


# ---- the full size against the fp64 table ----------------------------------------------------------------------------------
def _sample_units(model, x, count=2048):
    """>= count units covering every level, the most active unit and a never-active unit if there is one"""
    cnt = gpu_z(model, x).sum(0)
    H, n = model.hidden_dim, model.n_bits
    level = U.level_of_units(H, n)
    g = torch.Generator().manual_seed(5)
    picks = [torch.tensor([int(cnt.argmax())])]
    never = (cnt == 0).nonzero().flatten().cpu()
    if never.numel():
        picks.append(never[:1])
    for i in range(n):
        ids = (level == i).nonzero().flatten()
        picks.append(ids[torch.randperm(ids.numel(), generator=g)[:count // n]])
    units = torch.unique(torch.cat(picks))
    assert units.numel() >= count and set(level[units].tolist()) == set(range(n))
    return units, cnt


@pytest.mark.parametrize("sigmas,grad_path", [(-2.5, "lists"), (0.0, "dense")], ids=["sparse-lists", "dense-dense"])
def test_full_size_against_fp64(sigmas, grad_path):
    """B = 8192, H = 32768, D = 512, n_bits = 4: every gradient of a sample of >= 2048 units (all D columns) and decoder.bias
    whole against the fp64 table on the GPU's own z bits, before and after apply_secant_grad(); TOL = 1e-5 applies."""
    B, H, D, n = 8192, 32768, 512, 4
    model = make_q(U.q_params(731, D, H, sigmas), D, H, n, grad_path=grad_path)
    x = torch.from_numpy(S.activations(731, B, D)).to(DEV)
    units, cnt = _sample_units(model, x)
    got, _ = check_step(model, x, f"full size {grad_path}", units=units)
    assert model.last_decoder_grad_path == grad_path
    never = (cnt == 0)
    if bool(never.any()):
        assert float(got["decoder.weight"][never].abs().max()) == 0.0
        assert float(got["decoder.weight_mirror"][never].abs().max()) == 0.0
    model.decoder_grad_path = "auto"
    step(model, x)
    assert model.last_decoder_grad_path == grad_path          # what "auto" picks at this density


# ---- the two decoder-gradient paths -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigmas", [-2.5, 0.0], ids=["sparse", "dense"])
def test_paths_agree_and_are_reproducible(sigmas):
    B, H, D, n = 1000, 4096, 128, 4
    sd = U.q_params(741, D, H, sigmas)
    x = torch.from_numpy(S.activations(741, B, D)).to(DEV)
    runs = {}
    for path in GRAD_PATHS:
        model = make_q(sd, D, H, n, grad_path=path)
        two = []
        for _ in range(2):
            step(model, x)
            model.decoder.apply_secant_grad()
            two.append(grads_of(model))
        for k in two[0]:
            assert torch.equal(two[0][k], two[1][k]), f"{path}: {k} differs between two runs"
        runs[path] = two[0]
    never = gpu_z(model, x).sum(0) == 0
    for path in GRAD_PATHS:
        for k in ("decoder.weight", "decoder.weight_mirror"):
            if bool(never.any()):
                assert float(runs[path][k][never].abs().max()) == 0.0, f"{path}: a never-active unit has a {k} gradient"
    assert_close(runs["dense"], runs["lists"], list(U.PARAM_KEYS), what=f"dense vs lists ({sigmas})")
    for k in ("encoder.0.weight", "encoder.0.bias", "decoder.bias"):
        assert torch.equal(runs["dense"][k], runs["lists"][k])


# ---- edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_path", GRAD_PATHS)
@pytest.mark.parametrize("B,H,D,n", [(1, 256, 64, 4), (1000, 512, 64, 4), (8191, 256, 32, 4), (8, 1000, 32, 4), (40, 64, 4096, 2),
                                     (300, 96, 64, 1)])
def test_edge_shapes(B, H, D, n, grad_path):
    """B = 1; B not a multiple of the 32-row K slice; a padded model (H = 1000: levels 125, 125, 250, 500); D = 32 and the
    widest D the kernels accept (4096); one level"""
    model = make_q(U.q_params(751, D, H, -1.0), D, H, n, grad_path=grad_path)
    x = torch.from_numpy(S.activations(751, B, D)).to(DEV)
    check_step(model, x, f"B={B} H={H} D={D} n={n} {grad_path}", want_dx=True)


@pytest.mark.parametrize("grad_path", GRAD_PATHS)
def test_unit_active_in_every_row_and_in_none(grad_path):
    B, H, D, n = 700, 256, 64, 4
    sd = U.q_params(752, D, H, -2.5)
    sd["encoder.0.bias"][[3, 40, 200]] = 10.0
    sd["encoder.0.bias"][[5, 41, 201]] = -10.0
    model = make_q(sd, D, H, n, grad_path=grad_path)
    x = torch.from_numpy(S.activations(752, B, D)).to(DEV)
    cnt = gpu_z(model, x).sum(0)
    assert cnt[[3, 40, 200]].tolist() == [B] * 3 and cnt[[5, 41, 201]].tolist() == [0] * 3
    got, _ = check_step(model, x, f"always / never active {grad_path}")
    for k in ("decoder.weight", "decoder.weight_mirror"):
        assert float(got[k][[5, 41, 201]].abs().max()) == 0.0 and float(got[k][3].abs().max()) > 0.0


@pytest.mark.parametrize("grad_path", GRAD_PATHS)
def test_missing_incoming_gradients(grad_path):
    B, H, D, n = 64, 512, 64, 4
    model = make_q(U.q_params(753, D, H, -1.0), D, H, n, grad_path=grad_path)
    x = torch.from_numpy(S.activations(753, B, D)).to(DEV)
    keys = list(U.PARAM_KEYS)
    # only result[2]
    model.zero_grad(set_to_none=True)
    groups, levels = model.forward_train(x)
    w = torch.from_numpy(S.normal(753, (B, D), stream=3)).to(DEV)
    (levels[2] * w).sum().backward()
    G = torch.zeros((n, B, D), dtype=torch.float64, device=DEV)
    G[2] = w.double()
    assert_close(grads_of(model), restated(model, x, levels, G=G, gg=None), keys, what=f"only result[2] {grad_path}")
    # only latent_group[1]: no reconstruction gradient at all
    model.zero_grad(set_to_none=True)
    groups, levels = model.forward_train(x)
    (groups[1] * 3.0).backward()
    gg = torch.tensor([0.0, 3.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
    got = grads_of(model)
    assert_close(got, restated(model, x, levels, G=None, gg=gg), keys, what=f"only latent_group[1] {grad_path}")
    assert float(got["decoder.weight"].abs().max()) == 0.0 and float(got["decoder.bias"].abs().max()) == 0.0
    lv = U.level_of_units(H, n).to(DEV)
    assert float(got["encoder.0.weight"][lv != 1].abs().max()) == 0.0


def test_second_backward_and_missing_context_raise():
    D, H = 64, 256
    model = make_q(U.q_params(754, D, H, -1.0), D, H, 4)
    x = torch.from_numpy(S.activations(754, 16, D)).to(DEV)
    with pytest.raises(RuntimeError, match="forward_train"):
        model.decoder.apply_secant_grad()
    model(x)
    with pytest.raises(RuntimeError, match="forward_train"):          # forward() leaves no context
        model.decoder.apply_secant_grad()
    groups, levels = model.forward_train(x)
    with pytest.raises(RuntimeError, match="grad"):                   # no .grad yet
        model.decoder.apply_secant_grad()
    loss = q_loss(x, groups, levels)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


def test_limits_raise_value_error():
    with pytest.raises(ValueError, match="multiple of 4 up to 4096"):
        make_q(U.q_params(755, 4100, 64, -1.0), 4100, 64, 2).forward_train(torch.zeros((4, 4100), device=DEV))
    with pytest.raises(ValueError, match="multiple of 4 up to 4096"):
        make_q(U.q_params(755, 30, 64, -1.0), 30, 64, 2).forward_train(torch.zeros((4, 30), device=DEV))
    m = make_q(U.q_params(755, 64, 32768, -2.5), 64, 32768, 4, grad_path="lists")
    with pytest.raises(ValueError, match="2\\^31"):
        m.forward_train(torch.zeros((65536, 64), device=DEV))
    with pytest.raises(ValueError, match="at least one row"):
        m.forward_train(torch.zeros((0, 64), device=DEV))
    with pytest.raises(ValueError, match="expected \\[batch, 64\\]"):
        m.forward_train(torch.zeros((4, 32), device=DEV))


# ---- the reference trainer's loops -------------------------------------------------------------------------------------------
def _run_loop(model, x, loss_fn, secant, lr, steps):
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    ptrs = [p.data_ptr() for p in model.parameters()]
    losses = []
    for _ in range(steps):
        groups, levels = model.forward_train(x)
        loss = loss_fn(x, groups, levels, U.LOOP["lam"])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        secant()
        opt.step()
        losses.append(float(loss.item()))
    assert ptrs == [p.data_ptr() for p in model.parameters()], "a parameter moved"
    trained = [p for p in model.parameters() if p.grad is not None]      # stages past the first have no decoder bias gradient
    assert len(opt.state) == len(trained) and all(int(s["step"]) == steps for s in opt.state.values())
    return np.array(losses)


@pytest.mark.parametrize("name", sorted(U.LOOP_CASES))
def test_adam_loop_of_the_reference_trainer(name):
    """30 steps of the q_sae / rq_sae branch (forward_train, loss, zero_grad, backward, apply_secant_grad, Adam step) on a
    fixed batch: the loss of every step within the fixture's bound (ten times the largest relative gap between the
    reference run in fp32 and in fp64, at least 1e-5) of the reference's, and falling."""
    meta, z = U.load_fixture(U.LOOP_FIXTURE)
    c = dict(U.LOOP, **meta["cases"][name])
    D, H, n = c["D"], c["H"], c["n_bits"]
    sd, x_np = U.case_inputs(c, c["seed"])
    x = torch.from_numpy(x_np).to(DEV)
    if c["kind"] == "rq":
        model = make_rq(sd, D, H, n)
        losses = _run_loop(model, x, rq_loss, model.apply_secant_grad, c["lr"], c["steps"])
        fresh = make_rq({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, D, H, n)
    else:
        model = make_q(sd, D, H, n)
        losses = _run_loop(model, x, q_loss, model.decoder.apply_secant_grad, c["lr"], c["steps"])
        fresh = make_q({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, D, H, n)
    ref = z[f"{name}.loss64"]
    rel = np.abs(losses - ref) / np.abs(ref)
    print(f"{name}: loss {losses[0]:.4f} -> {losses[-1]:.4f}; max relative distance to the reference {rel.max():.3g} "
          f"(bound {c['bound']:.3g}, reference fp32-vs-fp64 gap {c['gap']:.3g})")
    assert rel.max() <= c["bound"], f"step {int(rel.argmax())}: {rel.max():.3g} > {c['bound']:.3g}"
    assert losses[-1] < losses[0] and all(losses[i + 3] < losses[i] for i in range(0, c["steps"] - 3, 3))
    # every cached pack followed the steps
    for a, b in zip(sum(model(x), []), sum(fresh(x), [])):
        assert torch.equal(a, b)
