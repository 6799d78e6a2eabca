"""BinaryLatentSAE.forward_train and its HIP backward (csrc/train_gemm.hip) on the MI355X: forward parity with forward(), the
binarise kernel at the cutoff, the reference's own gradients, the tile edges of each new kernel against the fp64 table, one
real-width step, determinism, needs_input_grad, refusals and the trainer loop against the reference's fp64 loss curve."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantizedsae_amd import optim as qoptim, torch_ops as ops
from quantizedsae_amd.sae import BinaryLatentSAE
from quantizedsae_amd.sae.binary_latent import _GE_HALF_CUTOFF

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_blatent_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5          # max |err| / max |g| per tensor: the project's training tolerance (test_train_ternary_gpu.py and siblings)
WIDE = dict(B=1024, D=512, H=32768, seed=921)
KEYS = U.PARAM_KEYS + ("x",)


def make(sd, D, H):
    m = BinaryLatentSAE(D, H)
    m.load_state_dict({name: torch.from_numpy(np.ascontiguousarray(v)) for name, v in sd.items()})
    return m.to(DEV)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32)


def grads_of(model):
    return {name: (p.grad.detach().clone() if p.grad is not None else None) for name, p in model.named_parameters()}


def step(model, x, want_dx=True):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(want_dx)
    z, recon = model.forward_train(xr)
    loss = F.mse_loss(recon, x)
    loss.backward()
    g = grads_of(model)
    g["x"] = xr.grad
    return z, recon.detach(), loss.detach(), g


def assert_close(got: dict, want: dict, keys, what=""):
    errs = {key: U.max_rel_err(got[key], want[key]) for key in keys}
    print(what, " ".join(f"{k}: {e:.3g}" for k, e in errs.items()))
    for key, err in errs.items():
        assert err <= TOL, f"{what} {key}: max |err| / max |g| = {err:.3g}"


# ---- forward parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,B", [(64, 256, 24), (36, 96, 7), (512, 1024, 64)])
def test_forward_train_equals_forward_bit_for_bit(D, H, B):
    model = make(U.blatent_params(931, D, H), D, H)
    x = torch.from_numpy(U.S.activations(931, B, D)).to(DEV)
    z0, r0 = model(x)
    z1, r1 = model.forward_train(x)
    assert r1.grad_fn is not None and not z1.requires_grad and z1.grad_fn is None
    assert torch.equal(bits(z0), bits(z1)) and torch.equal(bits(r0), bits(r1))
    assert 0.2 < float(z1.mean()) < 0.8 and float(r0.abs().max()) > 0


# ---- the binarise kernel -------------------------------------------------------------------------------------------------
def test_binarize_matches_threshold_ge_and_packbits_at_the_cutoff():
    B, H = 5, 1056
    pre = torch.from_numpy(U.S.normal(941, (B, H), stream=1)).mul_(1e-6)
    cut_bits = 0xB43FFFFE
    # the cutoff, one ulp below it (more negative), one ulp above it, -0.0, +0.0, nan, -nan, +inf, -inf, the smallest denormals
    specials = torch.from_numpy(np.array([cut_bits, cut_bits + 1, cut_bits - 1, 0x80000000, 0x00000000, 0x7FC00000, 0xFFC00000,
                                          0x7F800000, 0xFF800000, 0x00000001, 0x80000001], dtype=np.uint32).view(np.float32).copy())
    expect = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0])
    flat = pre.view(-1)
    at = torch.arange(len(specials))
    flat[37 * at + 3] = specials                          # spread over words and rows ..
    flat[B * H - 1 - 5 * at] = specials                   # .. and the last word of the last row
    pre = pre.to(DEV)
    assert int(bits(pre).view(-1)[3]) == cut_bits - (1 << 32) and int(bits(pre).view(-1)[40]) == cut_bits + 1 - (1 << 32)
    assert int(bits(pre).view(-1)[3]) == int(torch.tensor([_GE_HALF_CUTOFF]).view(torch.int32)[0])
    latent, zb = ops.blatent_binarize(pre, _GE_HALF_CUTOFF)
    want = ops.threshold_ge(pre, _GE_HALF_CUTOFF)
    assert torch.equal(bits(latent), bits(want))
    assert torch.equal(latent.view(-1)[(37 * at + 3).to(DEV)].cpu(), expect)
    assert torch.equal(latent.view(-1)[(B * H - 1 - 5 * at).to(DEV)].cpu(), expect)
    packed = np.packbits(want.cpu().numpy() != 0, axis=1, bitorder="little").view(np.uint32)
    assert zb.dtype == torch.int32 and tuple(zb.shape) == (B, H // 32)
    assert np.array_equal(zb.cpu().numpy().view(np.uint32), packed)
    none, zb2 = ops.blatent_binarize(pre, _GE_HALF_CUTOFF, want_latent=False)              # the latent pointer is nullable
    assert none is None and torch.equal(zb, zb2)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.blatent_binarize(pre[:, :100].contiguous(), _GE_HALF_CUTOFF)


# ---- the reference's gradients ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_gradients_match_reference_fixtures(name):
    meta, fx = U.load_fixture(name)
    D, H, B = meta["D"], meta["H"], meta["B"]
    sd, _ = U.case_inputs(meta, meta["seed"])
    model = make(sd, D, H)
    x = torch.from_numpy(fx["x"]).to(DEV).requires_grad_(True)
    z, recon = model.forward_train(x)
    assert np.array_equal(z.cpu().numpy(), U.unpack_latent(fx["binary_latent"], H))       # every bit: no element is excluded
    loss = F.mse_loss(recon, x.detach())
    loss.backward()
    e_recon = U.max_rel_err(recon, fx["recon"])
    e_loss = abs(loss.item() - float(fx["loss"])) / abs(float(fx["loss"]))
    print(f"{name} recon: {e_recon:.3g} loss: {e_loss:.3g}")
    assert e_recon <= TOL and e_loss <= TOL
    got = grads_of(model)
    got["x"] = x.grad
    assert_close(got, {k: fx["grad." + k] for k in KEYS}, KEYS, what=name)


# ---- tile edges of each new kernel on its own ------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [32, 96, 1056])
@pytest.mark.parametrize("D", [4, 36, 64])
@pytest.mark.parametrize("B", [1, 24, 257])
def test_kernels_at_tile_edges_against_fp64(B, D, H):
    seed = 951 + B + D + H
    sd = U.blatent_params(seed, D, H)
    x = torch.from_numpy(U.S.activations(seed, B, D)).to(DEV)
    G = torch.from_numpy(U.S.normal(seed, (B, D), stream=11)).to(DEV)
    W_e, b_e, W_d = (torch.from_numpy(sd[k]).to(DEV) for k in U.PARAM_KEYS[:3])
    pre = ops.encode_dense(x, W_e, b_e, ops.ACT_NONE)
    latent, zb = ops.blatent_binarize(pre, _GE_HALF_CUTOFF)
    assert np.array_equal(zb.cpu().numpy().view(np.uint32),
                          np.packbits(latent.cpu().numpy() != 0, axis=1, bitorder="little").view(np.uint32))
    if H >= 96 and B >= 24:
        assert bool((zb[:, -1] != 0).any())                      # the last bit word is live
    want = U.grads64(x, W_e, b_e, W_d, latent, G, want_dx=False)
    # dweight on its own
    dwd = ops.train_blatent_dweight(G, zb, H)
    assert tuple(dwd.shape) == (D, H)
    # dpre on its own, in place, against the table from the pre-activation the kernel itself read
    p = torch.sigmoid(pre.double())
    dpre64 = (G.double() @ W_d.double()) * (p * (1 - p))
    before = pre.clone()
    out = ops.train_blatent_dpre(pre, G, W_d)
    assert out.data_ptr() == pre.data_ptr() and not torch.equal(before, pre)
    errs = {"dweight": U.max_rel_err(dwd, want["decoder.weight"]), "dpre": U.max_rel_err(pre, dpre64)}
    print(f"B {B} D {D} H {H}:", " ".join(f"{k}: {e:.3g}" for k, e in errs.items()))
    assert errs["dweight"] <= TOL and errs["dpre"] <= TOL


# ---- one real-width case ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    B, D, H, seed = (WIDE[k] for k in ("B", "D", "H", "seed"))
    model = make(U.blatent_params(seed, D, H), D, H)
    x = torch.from_numpy(U.S.activations(seed, B, D)).to(DEV)
    first = step(model, x)
    return model, x, first


def test_real_width_gradients_against_fp64_table(wide):
    """B = 1024, D = 512, H = 32768: every element of every gradient and dx against the fp64 table on the forward's own latent."""
    model, x, (z, recon, loss, got) = wide
    B, D = WIDE["B"], WIDE["D"]
    lin, dec = model.encoder.linear, model.decoder
    frac = float(z.mean())
    assert 0.4 < frac < 0.6, frac
    recon64 = U.forward64(z, dec.weight, dec.bias)
    assert U.max_rel_err(recon, recon64) <= TOL
    G = U.trainer_incoming(x, recon, B, D)
    want = U.grads64(x, lin.weight, lin.bias, dec.weight, z, G, chunk=4096)
    assert_close(got, want, KEYS, what=f"real width (active {frac:.3f})")


def test_real_width_step_is_bitwise_reproducible(wide):
    model, x, (z0, r0, l0, g0) = wide
    z1, r1, l1, g1 = step(model, x)
    assert torch.equal(bits(z0), bits(z1)) and torch.equal(bits(r0), bits(r1)) and torch.equal(bits(l0), bits(l1))
    for k in KEYS:
        assert g0[k] is not None and torch.equal(bits(g0[k]), bits(g1[k])), k


# ---- needs_input_grad, second backward, refusals -------------------------------------------------------------------------
def test_needs_input_grad_and_second_backward():
    meta, fx = U.load_fixture("train_blatent_d64")
    D, H, B = meta["D"], meta["H"], meta["B"]
    sd, _ = U.case_inputs(meta, meta["seed"])
    x = torch.from_numpy(fx["x"]).to(DEV)
    model = make(sd, D, H)
    lin, dec = model.encoder.linear, model.decoder
    _, _, _, full = step(model, x)
    # x without requires_grad gets none; the parameter gradients are the same bits
    _, _, _, g = step(model, x, want_dx=False)
    assert g["x"] is None
    for k in U.PARAM_KEYS:
        assert torch.equal(bits(g[k]), bits(full[k])), k
    # a frozen encoder gets nothing and the saved pre-activation is not touched
    model.zero_grad(set_to_none=True)
    lin.weight.requires_grad_(False)
    lin.bias.requires_grad_(False)
    z, recon = model.forward_train(x)
    pre = recon.grad_fn.pre
    pre0 = pre.clone()
    F.mse_loss(recon, x).backward(retain_graph=True)
    assert lin.weight.grad is None and lin.bias.grad is None
    assert recon.grad_fn.pre is pre and torch.equal(bits(pre), bits(pre0))
    assert torch.equal(bits(pre0), bits(ops.encode_dense(x, lin.weight.detach(), lin.bias.detach(), ops.ACT_NONE)))
    assert torch.equal(bits(dec.weight.grad), bits(full["decoder.weight"]))
    assert torch.equal(bits(dec.bias.grad), bits(full["decoder.bias"]))
    F.mse_loss(recon, x).backward()                             # nothing was consumed: a second backward is fine here
    lin.weight.requires_grad_(True)
    lin.bias.requires_grad_(True)
    # a frozen decoder gets nothing; the encoder's gradients are the same bits
    model.zero_grad(set_to_none=True)
    dec.weight.requires_grad_(False)
    dec.bias.requires_grad_(False)
    z, recon = model.forward_train(x)
    F.mse_loss(recon, x).backward()
    assert dec.weight.grad is None and dec.bias.grad is None
    assert torch.equal(bits(lin.weight.grad), bits(full["encoder.0.weight"]))
    assert torch.equal(bits(lin.bias.grad), bits(full["encoder.0.bias"]))
    dec.weight.requires_grad_(True)
    dec.bias.requires_grad_(True)
    # the pre-activation became its gradient in place: a second backward through the same step says so
    model.zero_grad(set_to_none=True)
    z, recon = model.forward_train(x)
    loss = F.mse_loss(recon, x)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a second time: the saved pre-activation was turned into its gradient in place"):
        loss.backward()
    # fp64 input: x.grad comes back in the dtype x came in
    xd = x.double().requires_grad_(True)
    z, recon = model.forward_train(xd)
    F.mse_loss(recon, x).backward()
    assert xd.grad.dtype == torch.float64 and U.max_rel_err(xd.grad, full["x"]) <= TOL


def test_forward_train_refusals():
    with pytest.raises(ValueError, match="multiple of 4 up to 4096"):
        BinaryLatentSAE(66, 256).to(DEV).forward_train(torch.zeros(2, 66, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4 up to 4096"):
        BinaryLatentSAE(4100, 32).to(DEV).forward_train(torch.zeros(2, 4100, device=DEV))
    with pytest.raises(ValueError, match="hidden_dim a multiple of 32"):
        BinaryLatentSAE(64, 100).to(DEV).forward_train(torch.zeros(2, 64, device=DEV))
    m = BinaryLatentSAE(64, 256).to(DEV)
    with pytest.raises(ValueError, match=r"expected \[batch, 64\]"):
        m.forward_train(torch.zeros(2, 32, device=DEV))
    with pytest.raises(ValueError, match="empty batch"):
        m.forward_train(torch.zeros(0, 64, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_train(torch.zeros(2, 64))
    z, recon = m(torch.zeros(2, 64, device=DEV))                # forward() is unchanged: no graph
    assert recon.grad_fn is None and not recon.requires_grad


# ---- the trainer loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["torch", "qsae"])
def test_trainer_loop_reproduces_reference_loss_curve(which):
    """forward_train, F.mse_loss, backward, Adam(lr = 1e-3) on a fixed batch against the reference's fp64 loss curve, within
    max(10 * gap, 1e-5) relative (gap = the reference's own fp32-versus-fp64 deviation), with torch's Adam and with the
    package's."""
    meta, fx = U.load_fixture(U.LOOP_FIXTURE)
    D, H, B = meta["D"], meta["H"], meta["B"]
    model = make(U.blatent_params(meta["seed"], D, H), D, H)
    x = torch.from_numpy(U.S.activations(meta["seed"], B, D)).to(DEV)
    Adam = torch.optim.Adam if which == "torch" else qoptim.Adam
    opt = Adam(model.parameters(), lr=meta["lr"])
    losses = []
    for _ in range(meta["steps"]):
        z, recon = model.forward_train(x)
        loss = F.mse_loss(recon, x)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).double().cpu().numpy()
    rel = np.abs(losses - fx["loss64"]) / np.abs(fx["loss64"])
    bound = max(10 * meta["gap"], 1e-5)
    print(f"loop ({which} Adam): loss {losses[0]:.5f} -> {losses[-1]:.5f}  max relative deviation from fp64 {rel.max():.3g} "
          f"(bound {bound:.3g})")
    assert losses[-1] < losses[0]
    assert rel.max() <= bound, f"max relative deviation {rel.max():.3g} at step {int(rel.argmax())}"
