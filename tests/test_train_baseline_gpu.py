"""BaselineSparseAutoencoder.forward_train, its HIP backward and normalize_decoder_weights (csrc/train.hip) on the MI355X:
the reference's own gradients, forward parity with forward() on every latent path, the full-size shape against the fp64
restatement, determinism, units selected by every row, negative selections, edge shapes, missing incoming gradients, the
normalisation kernel and its cached table, and the reference trainer's loop."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantizedsae_amd import BaselineSparseAutoencoder, ops, synthetic as S

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_baseline_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5          # max |err| / max |g| per tensor: the project's training tolerance
NORM_TOL = 1e-5     # |W_gpu - W_fp64| elementwise (entries of a unit-norm column are at most 1)


def make_model(sd, D, H, k=32, path="auto"):
    m = BaselineSparseAutoencoder(D, H)
    m.load_state_dict({name: torch.from_numpy(np.ascontiguousarray(v)) for name, v in sd.items()})
    m.topk = k
    m.latent_path = path
    return m.to(DEV)


def fresh_copy(model):
    """A new model loaded from the state_dict of `model` (nothing cached)."""
    H, D = model.encoder.linear.weight.shape
    m = BaselineSparseAutoencoder(D, H)
    m.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    m.topk, m.latent_path = model.topk, model.latent_path
    return m.to(DEV)


def trainer_loss(x, h, recon, mu=0.0):
    loss = F.mse_loss(recon, x)
    if mu:
        loss = loss + mu * h.abs().sum() / x.shape[0]
    return loss


def grads_of(model):
    return {name: p.grad.detach().clone() for name, p in model.named_parameters()}


def params_cpu(model):
    lin, dec = model.encoder.linear, model.decoder
    return (lin.weight.detach().cpu(), lin.bias.detach().cpu(), dec.weight.detach().cpu(), dec.bias.detach().cpu())


def restated(model, x, mu=0.0, want_dx=False):
    """fp64 gradients of trainer_loss on the GPU's own selection (train_baseline_util)."""
    with torch.no_grad():
        idx, val, _ = model.forward_compact(x)
    xc = x.detach().cpu()
    W, b, Wd, bd = params_cpu(model)
    _, recon64 = U.forward64(xc, W, b, Wd, bd, idx.cpu())
    gR, gL = U.trainer_loss_grads(xc, recon64, val.cpu(), mu)
    g = U.grads64(xc, W, Wd, idx.cpu(), val.cpu(), gR, gL, want_dx=want_dx)
    if want_dx:
        g["x"] = g["x"] - gR
    return g


def assert_close(got: dict, want: dict, keys, tol=TOL, what=""):
    errs = {key: U.max_rel_err(got[key].detach().cpu(), want[key]) for key in keys}
    print(what, " ".join(f"{k}: {e:.3g}" for k, e in errs.items()))
    for key, err in errs.items():
        assert err <= tol, f"{what} {key}: max |err| / max |g| = {err:.3g}"


def train_step_grads(model, x, mu=0.0, dense_latent=True):
    model.zero_grad(set_to_none=True)
    h, recon = model.forward_train(x, dense_latent=dense_latent)
    trainer_loss(x, h, recon, mu).backward()
    return grads_of(model)


def check_step(model, x, what, mu=1e-3):
    x = x.requires_grad_(True)
    got = train_step_grads(model, x, mu=mu)
    got["x"] = x.grad
    want = restated(model, x.detach(), mu=mu, want_dx=True)
    assert_close(got, want, list(U.GRAD_KEYS) + ["x"], what=what)
    return got


# ---- the reference's gradients -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_gradients_match_reference_fixtures(name):
    meta, z = U.load_fixture(name)
    sd, x_np = U.case_inputs(meta, meta["seed"])
    model = make_model(sd, meta["D"], meta["H"], k=meta["k"])
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(meta["x_grad"])
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x)
    assert np.array_equal(np.sort(idx.cpu().numpy(), 1), np.sort(z["idx"], 1)), "selection differs from the reference"
    h, recon = model.forward_train(x)
    loss = trainer_loss(x, h, recon, meta["mu"])
    assert abs(loss.item() - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    loss.backward()
    got = grads_of(model)
    keys = list(U.GRAD_KEYS)
    if meta["x_grad"]:
        got["x"] = x.grad
        keys.append("x")
    assert_close(got, {k: z["grad." + k] for k in keys}, keys, what=name)


# ---- forward parity -------------------------------------------------------------------------------------------------------
PARITY = [(96, 2048, "auto"), (96, 2048, "inplace"), (96, 2048, "fused"), (96, 2048, "prefilter"),
          (8192, 32768, "auto"), (8192, 32768, "prefilter"), (8192, 32768, "fused"), (8192, 32768, "inplace")]


@pytest.mark.parametrize("B,H,path", PARITY, ids=[f"{b}x{h}-{p}" for b, h, p in PARITY])
def test_forward_train_outputs_equal_forward(B, H, path):
    D = 512
    model = make_model(S.baseline_sae_params(11, D, H, bias_std=0.1), D, H, path=path)
    x = torch.from_numpy(S.activations(12, B, D)).to(DEV)
    h, recon = model.forward_train(x)
    assert h.grad_fn is not None and recon.grad_fn is not None
    none, recon2 = model.forward_train(x, dense_latent=False)
    assert none is None and recon2.grad_fn is not None
    want_h, want_recon = model(x)
    idx, val, recon3 = model.forward_compact(x)
    assert torch.equal(h.detach(), want_h) and torch.equal(recon.detach(), want_recon)
    assert torch.equal(recon2.detach(), recon3)
    assert torch.equal(recon2.detach(), want_recon)


def test_topk_is_read_per_call():
    D, H, B = 64, 1024, 32
    model = make_model(S.baseline_sae_params(13, D, H, bias_std=0.1), D, H, k=8)
    x = torch.from_numpy(S.activations(14, B, D)).to(DEV)
    h8, _ = model.forward_train(x)
    model.topk = 16
    h16, recon16 = model.forward_train(x)
    assert int((h8 != 0).sum(1).max()) <= 8 and int((h16 != 0).sum(1).max()) <= 16
    assert int((h16 != 0).sum()) > int((h8 != 0).sum())
    want_h, want_recon = model(x)
    assert torch.equal(h16.detach(), want_h) and torch.equal(recon16.detach(), want_recon)
    check_step(model, x, "topk 16")


# ---- full size -----------------------------------------------------------------------------------------------------------
def test_full_size_gradients_against_fp64():
    B, D, H, k = 8192, 512, 32768, 32
    model = make_model(S.baseline_sae_params(21, D, H, bias_std=0.1), D, H, k=k)
    x = torch.from_numpy(S.activations(22, B, D)).to(DEV)
    got = check_step(model, x, "full size", mu=1e-3)
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x.detach())
    unused = torch.ones(H, dtype=torch.bool, device=DEV)
    unused[idx.long().reshape(-1)] = False
    print(f"full size: {int(unused.sum())} of {H} units unselected")
    assert not bool(got["encoder.0.weight"][unused].any()) and not bool(got["encoder.0.bias"][unused].any())
    assert not bool(got["decoder.weight"][:, unused].any())


# ---- determinism, unselected units, hot units --------------------------------------------------------------------------------
def test_backward_is_bitwise_reproducible():
    B, D, H = 4096, 512, 8192
    sd = S.baseline_sae_params(31, D, H, bias_std=0.05)
    sd["encoder.0.bias"][[5, 77]] += 3.0                       # two long lists, split into chunks
    model = make_model(sd, D, H)
    x = torch.from_numpy(S.activations(32, B, D)).to(DEV).requires_grad_(True)
    g1 = train_step_grads(model, x, mu=1e-3)
    dx1 = x.grad.clone()
    x.grad = None
    g2 = train_step_grads(model, x, mu=1e-3)
    for key in g1:
        assert torch.equal(g1[key], g2[key]), key
    assert torch.equal(dx1, x.grad)


def test_rows_and_columns_of_unselected_units_are_exactly_zero():
    """The outputs come from torch.empty: a unit nobody selected must still have its row of dW_enc and its column of dW_dec
    written (with zeros).  The buffers are poisoned first so that stale memory cannot pass for a zero."""
    B, D, H, k = 16, 64, 4096, 4
    model = make_model(S.baseline_sae_params(33, D, H, bias_std=0.1), D, H, k=k)
    x = torch.from_numpy(S.activations(34, B, D)).to(DEV)
    for _ in range(4):
        poison = [torch.full((H, D), float("nan"), device=DEV) for _ in range(8)]
        del poison
    got = train_step_grads(model, x, mu=1e-3)
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x)
    unused = torch.ones(H, dtype=torch.bool, device=DEV)
    unused[idx.long().reshape(-1)] = False
    assert int(unused.sum()) >= H - B * k
    for key in U.GRAD_KEYS:
        assert bool(torch.isfinite(got[key]).all()), key
    assert not bool(got["encoder.0.weight"][unused].any()) and not bool(got["encoder.0.bias"][unused].any())
    assert not bool(got["decoder.weight"][:, unused].any())
    assert bool(got["decoder.weight"][:, ~unused].any(0).all())
    assert_close(got, restated(model, x, mu=1e-3), U.GRAD_KEYS, what="sparse use")


@pytest.mark.parametrize("N", [255, 256, 257, 513])
def test_unit_selected_by_every_row(N):
    """A huge encoder bias puts unit 7 into every one of the N rows: its list has N entries, summed in chunks of 256 whose
    partials are added in chunk order (split at 256 and 512)."""
    D, H, u = 64, 1024, 7
    sd = S.baseline_sae_params(100 + N, D, H, bias_std=0.1)
    sd["encoder.0.bias"][u] = 100.0
    model = make_model(sd, D, H, k=4)
    x = torch.from_numpy(S.activations(200 + N, N, D)).to(DEV)
    with torch.no_grad():
        idx, _, _ = model.forward_compact(x)
    assert int((idx == u).sum()) == N and bool((idx == u).any(1).all())
    check_step(model, x, f"list of {N}")


def test_all_selected_values_negative():
    """No ReLU in this model: with an encoder bias of -10 everywhere every selected latent is negative, and the L1 term's
    gradient is -mu / B at every selected entry."""
    B, D, H = 96, 64, 1024
    sd = S.baseline_sae_params(41, D, H, bias_std=0.1)
    sd["encoder.0.bias"][:] = -10.0
    model = make_model(sd, D, H, k=8)
    x = torch.from_numpy(S.activations(42, B, D)).to(DEV)
    with torch.no_grad():
        _, val, _ = model.forward_compact(x)
    assert bool((val < 0).all())
    check_step(model, x, "negative selection", mu=3e-3)


# ---- edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 48])
def test_narrow_rows(D):
    B, H = 96, 1024
    model = make_model(S.baseline_sae_params(50 + D, D, H, bias_std=0.1), D, H, k=16)
    check_step(model, torch.from_numpy(S.activations(51, B, D)).to(DEV), f"D={D}")


def test_widest_rows_with_the_largest_k():
    """D = 4096 and k = 256 (both limits), over H = 1000 units (not a multiple of 32: partial transpose tiles)."""
    B, D, H = 32, 4096, 1000
    model = make_model(S.baseline_sae_params(91, D, H, bias_std=0.1), D, H, k=256)
    check_step(model, torch.from_numpy(S.activations(92, B, D)).to(DEV), "D=4096 k=256")


def test_one_row():
    D, H = 64, 1024
    model = make_model(S.baseline_sae_params(93, D, H, bias_std=0.1), D, H, k=8)
    check_step(model, torch.from_numpy(S.activations(94, 1, D)).to(DEV), "B=1")


def test_x_requires_grad():
    B, D, H = 64, 128, 2048
    model = make_model(S.baseline_sae_params(95, D, H, bias_std=0.1), D, H, k=8)
    x = torch.from_numpy(S.activations(96, B, D)).to(DEV)
    h, recon = model.forward_train(x)                                   # x without grad: nothing flows back to it
    trainer_loss(x, h, recon).backward()
    assert x.grad is None
    x = x.clone().requires_grad_(True)
    got = train_step_grads(model, x, mu=1e-3)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype
    want = restated(model, x.detach(), mu=1e-3, want_dx=True)
    got["x"] = x.grad
    assert_close(got, want, ["x"], what="dx")
    # parameters frozen: only dx is asked for
    for p in model.parameters():
        p.requires_grad_(False)
    x2 = x.detach().clone().requires_grad_(True)
    h, recon = model.forward_train(x2)
    trainer_loss(x2, h, recon, 1e-3).backward()
    assert torch.equal(x2.grad, x.grad)


def test_missing_incoming_gradients():
    B, D, H, k = 128, 64, 2048, 8
    model = make_model(S.baseline_sae_params(71, D, H, bias_std=0.05), D, H, k=k)
    lin, dec = model.encoder.linear, model.decoder
    x = torch.from_numpy(S.activations(72, B, D)).to(DEV)
    with torch.no_grad():
        idx, val, _ = model.forward_compact(x)
    W, b, Wd, bd = params_cpu(model)
    # a loss on h only: nothing reaches the decoder
    h, _ = model.forward_train(x)
    h.abs().sum().backward()
    want = U.grads64(x.cpu(), W, Wd, idx.cpu(), val.cpu(), None, torch.sign(val.cpu().double()))
    assert_close(grads_of(model), want, ("encoder.0.weight", "encoder.0.bias"), what="latent only")
    assert dec.weight.grad is not None and dec.bias.grad is not None
    assert dec.weight.grad.shape == dec.weight.shape
    assert not bool(dec.weight.grad.any()) and not bool(dec.bias.grad.any())
    # a loss on the reconstruction only, without the dense latent
    model.zero_grad(set_to_none=True)
    none, recon = model.forward_train(x, dense_latent=False)
    F.mse_loss(recon, x).backward()
    _, recon64 = U.forward64(x.cpu(), W, b, Wd, bd, idx.cpu())
    gR, _ = U.trainer_loss_grads(x.cpu(), recon64, val.cpu())
    want = U.grads64(x.cpu(), W, Wd, idx.cpu(), val.cpu(), gR, None)
    assert_close(grads_of(model), want, U.GRAD_KEYS, what="recon only")
    # a latent gradient that is dense: only the selected entries count (the scatter_ backward)
    model.zero_grad(set_to_none=True)
    h, _ = model.forward_train(x)
    wgt = torch.from_numpy(S.activations(73, B, H)).to(DEV)
    (h * wgt).sum().backward()
    sel = torch.gather(wgt.cpu().double(), 1, idx.cpu().long())
    want = U.grads64(x.cpu(), W, Wd, idx.cpu(), val.cpu(), None, sel)
    assert_close(grads_of(model), want, ("encoder.0.weight", "encoder.0.bias"), what="dense latent gradient")


def test_past_the_limits_raises_value_error():
    model = BaselineSparseAutoencoder(50, 1024).to(DEV)
    with pytest.raises(ValueError):
        model.forward_train(torch.randn(8, 50, device=DEV))
    model = BaselineSparseAutoencoder(4100, 1024).to(DEV)
    with pytest.raises(ValueError, match="4096"):
        model.forward_train(torch.randn(8, 4100, device=DEV))
    model = BaselineSparseAutoencoder(64, 1024).to(DEV)
    model.topk = 257
    with pytest.raises(ValueError, match="topk <= 256"):
        model.forward_train(torch.randn(8, 64, device=DEV))
    model.topk = 8
    with pytest.raises(ValueError, match="expected"):
        model.forward_train(torch.randn(8, 32, device=DEV))
    i32 = dict(dtype=torch.int32, device=DEV)
    f = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(ValueError):                                   # D % 4 != 0
        ops.train_table_unit_grad(torch.zeros(65, **i32), torch.zeros(32, **i32), f(4, 8), f(4, 8), f(4, 50), None)
    with pytest.raises(ValueError):                                   # k > 256
        ops.train_table_unit_grad(torch.zeros(65, **i32), torch.zeros(4 * 260, **i32), f(4, 260), f(4, 260), f(4, 64), None)
    with pytest.raises(ValueError):                                   # entries do not match B k
        ops.train_table_unit_grad(torch.zeros(65, **i32), torch.zeros(31, **i32), f(4, 8), f(4, 8), f(4, 64), None)
    with pytest.raises(ValueError):                                   # H % 4 != 0
        ops.normalize_columns_table(f(64, 66))
    with pytest.raises(ValueError):                                   # not contiguous
        ops.normalize_columns_table(f(64, 128)[:, :64])


# ---- the low-level op --------------------------------------------------------------------------------------------------------
def test_table_unit_grad_nullable_outputs_and_transposed_layout():
    B, D, H, k = 300, 96, 520, 8                                   # H not a multiple of 32, D not a multiple of 64
    g = torch.Generator().manual_seed(5)
    idx = torch.stack([torch.randperm(H, generator=g)[:k] for _ in range(B)]).to(torch.int32).to(DEV)
    val, gv = torch.randn(B, k, generator=g).to(DEV), torch.randn(B, k, generator=g).to(DEV)
    x, gR = torch.randn(B, D, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    off, ent = ops.train_csr(idx, H)
    dW, db, dWd = ops.train_table_unit_grad(off, ent, val, gv, x, gR)
    flat = idx.long().reshape(-1).cpu()
    want_T = torch.zeros(H, D, dtype=torch.float64).index_add_(
        0, flat, (val.cpu().double()[:, :, None] * gR.cpu().double()[:, None, :]).reshape(-1, D))
    want_W = torch.zeros(H, D, dtype=torch.float64).index_add_(
        0, flat, (gv.cpu().double()[:, :, None] * x.cpu().double()[:, None, :]).reshape(-1, D))
    assert dWd.shape == (D, H) and dWd.is_contiguous()
    assert U.max_rel_err(dWd.cpu(), want_T.t()) <= TOL and U.max_rel_err(dW.cpu(), want_W) <= TOL
    a, b, c = ops.train_table_unit_grad(off, ent, val, gv, x, gR, want_encoder=False)
    assert a is None and b is None and torch.equal(c, dWd)
    a, b, c = ops.train_table_unit_grad(off, ent, val, gv, x, gR, want_decoder=False)
    assert c is None and torch.equal(a, dW) and torch.equal(b, db)
    a, b, c = ops.train_table_unit_grad(off, ent, val, gv, x, None)
    assert torch.equal(a, dW) and torch.equal(b, db) and c.shape == (D, H) and not bool(c.any())


# ---- normalisation -----------------------------------------------------------------------------------------------------------
def test_normalize_matches_the_reference_fixture_and_fp64():
    meta, z = U.load_fixture(U.NORMALIZED_CASE)
    sd, x_np = U.case_inputs(meta, meta["seed"])
    model = make_model(sd, meta["D"], meta["H"], k=meta["k"])
    x = torch.from_numpy(x_np).to(DEV)
    model(x)                                                   # fill the table cache of the old weights
    ptr, param = model.decoder.weight.data_ptr(), model.decoder.weight
    model.normalize_decoder_weights()
    assert model.decoder.weight is param and model.decoder.weight.data_ptr() == ptr
    got = model.decoder.weight.detach().cpu().double()
    e_fix = float((got - torch.from_numpy(z["normalized.decoder.weight"]).double()).abs().max())
    e_64 = float((got - U.normalize64(sd["decoder.weight"])).abs().max())
    print(f"normalise d64: vs fixture {e_fix:.3g}, vs fp64 {e_64:.3g}")
    assert e_fix <= NORM_TOL and e_64 <= NORM_TOL
    fresh = fresh_copy(model)
    for a, b in zip(model(x), fresh(x)):
        assert torch.equal(a, b)
    assert torch.equal(model._table(), model.decoder.weight.detach().t().contiguous())


@pytest.mark.parametrize("D,H", [(512, 32768), (512, 1000), (4, 64), (1, 4), (7, 36), (640, 256), (1030, 68)])
def test_normalize_op_shapes(D, H):
    g = torch.Generator().manual_seed(D * 131 + H)
    W0 = torch.randn(D, H, generator=g) * (torch.rand(1, H, generator=g) * 4 + 0.01)
    W0[:, 1] = 0.0                                             # a zero column stays zero
    W0[:, 2] = 1e-12                                           # a column under the clamp is divided by 1e-8
    W0[D // 2, 3] = float("nan")                               # a NaN column stays NaN
    W = W0.to(DEV)
    ptr = W.data_ptr()
    table = ops.normalize_columns_table(W)
    assert W.data_ptr() == ptr and table.shape == (H, D)
    want = U.normalize64(W0)
    ok = torch.ones(H, dtype=torch.bool)
    ok[3] = False
    assert torch.equal(table[ok], W.t()[ok]) and bool(torch.isnan(table[3]).all())
    err = float((W.cpu().double() - want)[:, ok].abs().max())
    print(f"normalise {D}x{H}: max |err| = {err:.3g}")
    assert err <= NORM_TOL
    assert not bool(W[:, 1].any())
    assert bool(torch.isnan(W[:, 3]).all())
    norms = W.cpu().double().norm(dim=0)
    live = ok.clone()
    live[1] = live[2] = False
    assert float((norms[live] - 1).abs().max()) <= 1e-5
    W2 = W0.to(DEV)
    assert ops.normalize_columns_table(W2, want_table=False) is None and torch.equal(W2[:, ok], W[:, ok])


def test_normalize_is_reproducible_and_idempotent_to_rounding():
    D, H = 512, 8192
    W0 = torch.from_numpy(S.baseline_sae_params(61, D, H)["decoder.weight"]).to(DEV)
    a, b = W0.clone(), W0.clone()
    ta, tb = ops.normalize_columns_table(a), ops.normalize_columns_table(b)
    assert torch.equal(a, b) and torch.equal(ta, tb)
    ops.normalize_columns_table(b)
    assert float((a - b).abs().max()) <= 1e-6


def test_normalize_falls_back_when_hidden_dim_is_not_a_multiple_of_4():
    D, H = 64, 1022
    sd = S.baseline_sae_params(62, D, H, bias_std=0.1)
    model = BaselineSparseAutoencoder(D, H)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(DEV)
    model.normalize_decoder_weights()
    err = float((model.decoder.weight.detach().cpu().double() - U.normalize64(sd["decoder.weight"])).abs().max())
    assert err <= NORM_TOL


def test_optimizer_step_and_normalisation_are_picked_up_by_the_next_forward():
    """Every derived copy (prefilter pack, K-interleave, decoder table) follows an optimizer step and a normalisation."""
    B, D, H = 2048, 512, 8192                                   # large enough for the prefilter path under "auto"
    for path in ("auto", "fused", "inplace"):
        model = make_model(S.baseline_sae_params(63, D, H, bias_std=0.1), D, H, path=path)
        x = torch.from_numpy(S.activations(64, B, D)).to(DEV)
        model(x)
        model.forward_compact(x)
        opt = torch.optim.SGD(model.parameters(), lr=0.5)
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        grads = train_step_grads(model, x)
        opt.step()
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), before[n] - 0.5 * grads[n]), n
            assert not torch.equal(p.detach(), before[n]), n
        fresh = fresh_copy(model)
        h, recon = model.forward_train(x)
        for a, b in zip((h.detach(), recon.detach()), fresh(x)):
            assert torch.equal(a, b), path
        for a, b in zip(model(x), fresh(x)):
            assert torch.equal(a, b), path
        model.normalize_decoder_weights()
        fresh = fresh_copy(model)
        h, recon = model.forward_train(x)
        for a, b in zip((h.detach(), recon.detach()), fresh(x)):
            assert torch.equal(a, b), path
        for a, b in zip(model.forward_compact(x), fresh.forward_compact(x)):
            assert torch.equal(a, b), path


# ---- the reference trainer's loop ------------------------------------------------------------------------------------------
def test_adam_loop_of_the_reference_trainer():
    """trainer.py:166-173 on a fixed batch: forward, mse, zero_grad, backward, Adam step, normalize_decoder_weights.  The
    reference itself, at exactly this recipe on the CPU: the loss falls from 1.010 to 0.662 and never exceeds 1.06."""
    D, H, k, B, lr = 64, 1024, 8, 256, 1e-3
    model = make_model(S.baseline_sae_params(611, D, H, bias_std=0.1), D, H, k=k)
    x = torch.from_numpy(S.activations(611, B, D)).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    ptr, param = model.decoder.weight.data_ptr(), model.decoder.weight
    losses = []
    for step in range(30):
        latent, recon = model.forward_train(x)
        loss = F.mse_loss(recon, x)
        opt.zero_grad()
        loss.backward()
        opt.step()
        model.normalize_decoder_weights()
        losses.append(loss.item())
        norms = model.decoder.weight.detach().double().norm(dim=0)
        assert float((norms - 1).abs().max()) <= 1e-5, step
    with torch.no_grad():
        losses.append(F.mse_loss(model(x)[1], x).item())
    print("adam trajectory: " + " ".join(f"{v:.4f}" for v in losses))
    assert losses[29] < losses[0] and losses[-1] < losses[0]
    assert max(losses) <= 1.06
    assert model.decoder.weight is param and model.decoder.weight.data_ptr() == ptr
    assert len(opt.state[param]) > 0
    fresh = fresh_copy(model)
    for a, b in zip(model(x), fresh(x)):
        assert torch.equal(a, b)
