"""BinarySAE.forward_train and its HIP backward (csrc/train.hip) on the MI355X: the reference's own gradients, forward
parity with forward(), the full-size shape against the fp64 restatement, determinism, a unit selected by every row,
edge shapes, and a short training loop."""
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from quantizedsae_amd import BinarySAE, synthetic as S

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def make_model(sd, D, H, n_bits, gamma, k=None):
    m = BinarySAE(D, H, gamma=gamma, n_bits=n_bits)
    m.load_state_dict({name: torch.from_numpy(v) for name, v in sd.items()})
    if k is not None:
        m.k = k / H
        assert m.top_k == k
    return m.to(DEV)


def trainer_loss(x, latent, recon, pol, lam=1e-2, mu=0.0):
    loss = 0.5 * F.mse_loss(recon, x) + lam * pol
    if mu:
        loss = loss + mu * latent.abs().sum() / x.shape[0]
    return loss


def grads_of(model):
    return {name: p.grad.detach().clone() for name, p in model.named_parameters()}


def restated(model, x, lam=1e-2, mu=0.0, want_dx=False):
    """fp64 gradients of trainer_loss on the GPU's own selection (train_util)."""
    lin, dec = model.encoder.linear, model.decoder
    with torch.no_grad():
        idx, val, _ = model.forward_compact(x)
    xc = x.detach().cpu()
    args = (lin.weight.detach().cpu(), lin.bias.detach().cpu(), dec.weight.detach().cpu(), dec.bias.detach().cpu())
    val64, recon64, _ = U.forward64(xc, *args, dec.n_bits, dec.gamma, idx.cpu())
    gR, gL, gP = U.trainer_loss_grads(xc, recon64, val.cpu(), lam, mu)
    g = U.grads64(xc, args[0], args[2], dec.n_bits, dec.gamma, idx.cpu(), val.cpu(), gR, gL, gP, want_dx=want_dx)
    if want_dx:
        g["x"] = g["x"] - gR
    return g


def assert_close(got: dict, want: dict, keys, tol=TOL, what=""):
    for key in keys:
        err = U.max_rel_err(got[key].detach().cpu(), want[key])
        assert err <= tol, f"{what} {key}: max |err| / max |g| = {err:.3g}"


def train_step_grads(model, x, lam=1e-2, mu=0.0, dense_latent=True):
    model.zero_grad(set_to_none=True)
    latent, recon, pol = model.forward_train(x, dense_latent=dense_latent)
    trainer_loss(x, latent, recon, pol, lam, mu).backward()
    return grads_of(model)


# ---- the reference's gradients -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_gradients_match_reference_fixtures(name):
    meta, z = U.load_fixture(name)
    sd, x_np = U.case_inputs(meta, meta["seed"])
    model = make_model(sd, meta["D"], meta["H"], meta["n_bits"], meta["gamma"], k=meta["k"])
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(meta["x_grad"])
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x)
    assert np.array_equal(np.sort(idx.cpu().numpy(), 1), np.sort(z["idx"], 1)), "selection differs from the reference"
    latent, recon, pol = model.forward_train(x)
    loss = trainer_loss(x, latent, recon, pol, meta["lam"], meta["mu"])
    assert abs(loss.item() - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    loss.backward()
    got = grads_of(model)
    keys = list(U.GRAD_KEYS)
    if meta["x_grad"]:
        got["x"] = x.grad
        keys.append("x")
    assert_close(got, {k: z["grad." + k] for k in keys}, keys, what=name)


# ---- forward parity -------------------------------------------------------------------------------------------------------
PARITY = [(64, 4096, "auto"), (8192, 32768, "auto"), (8192, 32768, "fused")]


@pytest.mark.parametrize("B,H,path", PARITY, ids=[f"{b}x{h}-{p}" for b, h, p in PARITY])
def test_forward_train_outputs_equal_soft_forward(B, H, path):
    D, n = 512, 4
    sd = S.binary_sae_params(11, D, H, n, logit_std=1.0, dec_bias_std=0.1)
    model = make_model(sd, D, H, n, 4.0)
    model.latent_path = path
    x = torch.from_numpy(S.activations(12, B, D)).to(DEV)
    latent, recon, pol = model.forward_train(x)
    assert latent.grad_fn is not None and recon.grad_fn is not None and pol.grad_fn is not None
    none, recon2, _ = model.forward_train(x, dense_latent=False)
    model.decoder.decode_mode = "soft"
    want_latent, want_recon, want_pol = model(x)
    print(f"path {model.resolved_latent_path(B)}")
    assert none is None
    assert torch.equal(latent.detach(), want_latent) and torch.equal(recon.detach(), want_recon)
    assert torch.equal(recon2.detach(), want_recon)
    a, b = np.float32(pol.item()), np.float32(want_pol.item())
    assert abs(a - b) <= np.spacing(b), (a, b)


# ---- full size -----------------------------------------------------------------------------------------------------------
def test_full_size_gradients_against_fp64():
    B, D, H, n = 8192, 512, 32768, 4
    sd = S.binary_sae_params(21, D, H, n, logit_std=1.0, dec_bias_std=0.1)
    model = make_model(sd, D, H, n, 4.0)
    x = torch.from_numpy(S.activations(22, B, D)).to(DEV).requires_grad_(True)
    mu = 1e-3
    got = train_step_grads(model, x, mu=mu)
    got["x"] = x.grad
    want = restated(model, x.detach(), mu=mu, want_dx=True)
    assert_close(got, want, list(U.GRAD_KEYS) + ["x"], what="full size")
    rows = np.arange(0, B, B // 64)
    lin, dec = model.encoder.linear, model.decoder
    ref = oracle.binary_forward(x.detach()[rows].cpu().numpy(), lin.weight.detach().cpu().numpy(),
                                lin.bias.detach().cpu().numpy(), dec.weight.detach().cpu().numpy(),
                                dec.bias.detach().cpu().numpy(), n_bits=n, gamma=4.0, k=model.top_k, soft=True)
    with torch.no_grad():
        latent, recon, _ = model.forward_train(x.detach())
    assert np.array_equal(latent[rows].cpu().numpy(), ref["latent"])          # the selection, bit for bit
    # (the oracle's soft table rounds the host's expf: the reconstruction agrees to rounding, not bit for bit)
    assert np.allclose(recon[rows].cpu().numpy(), ref["reconstruction"], rtol=1e-5, atol=1e-5)


# ---- determinism and a unit selected by every row ------------------------------------------------------------------------
def test_backward_is_bitwise_reproducible():
    B, D, H, n = 4096, 512, 8192, 4
    sd = S.binary_sae_params(31, D, H, n, logit_std=1.0, enc_bias_std=0.05)
    sd["encoder.0.bias"][[5, 77]] += 3.0                       # two long lists, split into chunks
    model = make_model(sd, D, H, n, 4.0)
    x = torch.from_numpy(S.activations(32, B, D)).to(DEV).requires_grad_(True)
    g1 = train_step_grads(model, x, mu=1e-3)
    dx1 = x.grad.clone()
    x.grad = None
    g2 = train_step_grads(model, x, mu=1e-3)
    for key in g1:
        assert torch.equal(g1[key], g2[key]), key
    assert torch.equal(dx1, x.grad)


def test_unit_selected_by_every_row():
    B, D, H, n = 65536, 64, 4096, 4
    sd = S.binary_sae_params(41, D, H, n, logit_std=1.0)
    sd["encoder.0.bias"][7] = 100.0
    model = make_model(sd, D, H, n, 4.0)
    x = torch.from_numpy(S.activations(42, B, D)).to(DEV)
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x)
    assert bool((idx == 7).any(1).all()), "unit 7 is not in every row"
    got = train_step_grads(model, x, dense_latent=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        train_step_grads(model, x, dense_latent=False)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    print(f"hot unit: B = {B}, list of 65536 entries: {ms:.2f} ms per forward_train + backward")
    assert ms < 200.0
    want = restated(model, x)
    assert_close(got, want, U.GRAD_KEYS, what="hot unit")


# ---- edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(32, 1), (48, 2), (32, 4), (48, 8), (64, 8)])
def test_narrow_rows_and_every_n_bits(D, n):
    B, H = 96, 1024
    sd = S.binary_sae_params(50 + D + n, D, H, n, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1)
    model = make_model(sd, D, H, n, 2.0, k=16)
    x = torch.from_numpy(S.activations(51, B, D)).to(DEV).requires_grad_(True)
    got = train_step_grads(model, x, mu=1e-3)
    got["x"] = x.grad
    want = restated(model, x.detach(), mu=1e-3, want_dx=True)
    assert_close(got, want, list(U.GRAD_KEYS) + ["x"], what=f"D={D} n={n}")


def test_k_zero():
    B, D, H, n = 32, 64, 256, 4
    sd = S.binary_sae_params(61, D, H, n, logit_std=1.0, dec_bias_std=0.1)
    model = make_model(sd, D, H, n, 4.0)
    assert model.top_k == 0
    x = torch.from_numpy(S.activations(62, B, D)).to(DEV).requires_grad_(True)
    latent, recon, pol = model.forward_train(x)
    assert not bool(latent.any())
    trainer_loss(x, latent, recon, pol).backward()
    lin, dec = model.encoder.linear, model.decoder
    assert not bool(lin.weight.grad.any()) and not bool(lin.bias.grad.any())
    gR = (recon.detach().double() - x.detach().double()) / (B * D)
    assert U.max_rel_err(dec.bias.grad.cpu(), gR.sum(0).cpu()) <= TOL
    want = U.grads64(x.detach().cpu(), lin.weight.detach().cpu(), dec.weight.detach().cpu(), n, 4.0,
                     torch.zeros((B, 0), dtype=torch.long), torch.zeros((B, 0)), None, None, 1e-2)
    assert U.max_rel_err(dec.weight.grad.cpu(), want["decoder.weight"]) <= TOL
    assert torch.allclose(x.grad, -gR.float())


def test_missing_incoming_gradients():
    B, D, H, n = 128, 64, 2048, 4
    sd = S.binary_sae_params(71, D, H, n, logit_std=1.0, enc_bias_std=0.05)
    model = make_model(sd, D, H, n, 4.0, k=8)
    lin, dec = model.encoder.linear, model.decoder
    x = torch.from_numpy(S.activations(72, B, D)).to(DEV)
    args = (x.cpu(), lin.weight.detach().cpu(), dec.weight.detach().cpu(), n, 4.0)
    with torch.no_grad():
        idx, val, _ = model.forward_compact(x)
    # polarize only: no recon / latent gradient
    _, _, pol = model.forward_train(x)
    pol.backward()
    want = U.grads64(*args, idx.cpu(), val.cpu(), None, None, 1.0)
    assert U.max_rel_err(dec.weight.grad.cpu(), want["decoder.weight"]) <= TOL
    assert not bool(lin.weight.grad.any()) and not bool(dec.bias.grad.any())
    # latent only: no recon / polarize gradient
    model.zero_grad(set_to_none=True)
    latent, _, _ = model.forward_train(x)
    latent.abs().sum().backward()
    want = U.grads64(*args, idx.cpu(), val.cpu(), None, torch.sign(val.cpu().double()), None)
    assert_close(grads_of(model), want, ("encoder.0.weight", "encoder.0.bias"), what="latent only")
    assert not bool(dec.weight.grad.any()) and not bool(dec.bias.grad.any())


def test_unsupported_shape_raises_value_error():
    model = BinarySAE(50, 1024, gamma=4.0, n_bits=4).to(DEV)
    with pytest.raises(ValueError, match="multiple of 4"):
        model.forward_train(torch.randn(8, 50, device=DEV))


# ---- the kernels' limits (train.hip: kTrainMaxD, kTrainMaxK, kTrainChunk, kColRows) ----------------------------------------
def set_k(model, k):
    model.k = (k + 0.5) / model.hidden_dim
    assert model.top_k == k
    return model


def check_step(model, x, what, mu=1e-3):
    x = x.requires_grad_(True)
    got = train_step_grads(model, x, mu=mu)
    got["x"] = x.grad
    want = restated(model, x.detach(), mu=mu, want_dx=True)
    assert_close(got, want, list(U.GRAD_KEYS) + ["x"], what=what)


def test_widest_rows_with_the_largest_k():
    """D = 4096 and k = 256 (both limits), over H = 1000 units (not a multiple of 64)."""
    B, D, H, n = 32, 4096, 1000, 4
    sd = S.binary_sae_params(91, D, H, n, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1)
    model = set_k(make_model(sd, D, H, n, 2.0), 256)
    check_step(model, torch.from_numpy(S.activations(92, B, D)).to(DEV), "D=4096 k=256")


@pytest.mark.parametrize("N", [255, 256, 257, 512, 513])
def test_unit_lists_at_the_chunk_splits(N):
    """Unit 7 is selected by exactly N rows (encoder row 100 e0, zero bias, x[:, 0] = 1 on N rows and 0 elsewhere): its list
    is summed in chunks of kTrainChunk = 256 entries, split at 256 and 512."""
    B, D, H, n, u = 600, 64, 1024, 4, 7
    sd = S.binary_sae_params(100 + N, D, H, n, logit_std=1.0, dec_bias_std=0.1)
    sd["encoder.0.weight"][u] = 0.0
    sd["encoder.0.weight"][u, 0] = 100.0
    model = set_k(make_model(sd, D, H, n, 2.0), 4)
    x = S.activations(200 + N, B, D)
    x[:, 0] = 0.0
    x[np.random.default_rng(N).permutation(B)[:N], 0] = 1.0
    x = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x)
    assert int((idx == u).sum()) == N
    check_step(model, x, f"list of {N}")


@pytest.mark.parametrize("B", [256, 257])
def test_one_unit_in_every_row_at_the_split_switch(B):
    """k = 1 and unit 7 on top of every row: B k = 256 keeps its list in one chunk (no final launch), 257 splits it."""
    D, H, n = 64, 1024, 4
    sd = S.binary_sae_params(300 + B, D, H, n, logit_std=1.0, dec_bias_std=0.1)
    sd["encoder.0.bias"][7] = 100.0
    model = set_k(make_model(sd, D, H, n, 2.0), 1)
    x = torch.from_numpy(S.activations(301, B, D)).to(DEV)
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x)
    assert bool((idx[:, 0] == 7).all())
    check_step(model, x, f"B k = {B}")


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_batches_around_the_column_sum_partials(B):
    D, H, n = 64, 1024, 4
    sd = S.binary_sae_params(400 + B, D, H, n, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1)
    model = set_k(make_model(sd, D, H, n, 2.0), 8)
    check_step(model, torch.from_numpy(S.activations(401, B, D)).to(DEV), f"B={B}")


def test_past_the_limits_raises_value_error():
    model = BinarySAE(4100, 1024, gamma=4.0, n_bits=4).to(DEV)
    with pytest.raises(ValueError, match="4096"):
        model.forward_train(torch.randn(8, 4100, device=DEV))
    model = set_k(BinarySAE(64, 1024, gamma=4.0, n_bits=4).to(DEV), 257)
    with pytest.raises(ValueError, match="top-k <= 256"):
        model.forward_train(torch.randn(8, 64, device=DEV))


# ---- a training loop ----------------------------------------------------------------------------------------------------
def test_sgd_step_cache_invalidation_and_adam_loop():
    B, D, H, n, lr = 512, 128, 4096, 4, 1e-2
    sd = S.binary_sae_params(81, D, H, n, logit_std=1.0, enc_bias_std=0.05, dec_bias_std=0.1)
    model = make_model(sd, D, H, n, 4.0, k=16)
    x = torch.from_numpy(S.activations(82, B, D)).to(DEV)
    model(x)                                                   # fill the packed / prefilter caches of the old weights
    before = {name: p.detach().clone() for name, p in model.named_parameters()}
    want = restated(model, x)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    train_step_grads(model, x)
    opt.step()
    for name, p in model.named_parameters():
        step64 = before[name].cpu().double() - lr * want[name]
        scale = float(want[name].abs().max())
        err = float((p.detach().cpu().double() - step64).abs().max())
        assert err <= lr * TOL * scale + 2 * float(np.spacing(np.float32(before[name].abs().max().item()))), name
    fresh = BinarySAE(D, H, gamma=4.0, n_bits=n)
    fresh.load_state_dict({k_: v.detach().cpu() for k_, v in model.state_dict().items()})
    fresh.k = model.k
    fresh = fresh.to(DEV)
    for a, b in zip(model(x), fresh(x)):
        assert torch.equal(a, b)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for step in range(50):
        xb = torch.from_numpy(S.activations(1000 + step, B, D)).to(DEV)
        opt.zero_grad(set_to_none=True)
        latent, recon, pol = model.forward_train(xb, dense_latent=False)
        loss = trainer_loss(xb, latent, recon, pol)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("adam trajectory: " + " ".join(f"{v:.4f}" for v in losses))
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
