"""TernarySparseAutoencoder.forward_train, its HIP backward (csrc/train_gemm.hip, csrc/train.hip) and the RigL mask kernels
(csrc/train_mask.hip) on the MI355X: the reference's own gradients and masks, forward parity with forward(), the three
backward kernels on their own at the tile edges against fp64, the full size against the fp64 table and against the exact mask
restatement, determinism, missing incoming gradients, refusals, cache
invalidation and the reference trainer's t_sae loop."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantizedsae_amd import TernarySparseAutoencoder, ops, synthetic as S

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_ternary_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5          # max |err| / max |g| per tensor: the project's training tolerance (test_train_gpu.py, test_train_baseline_gpu.py)
FULL = dict(B=8192, D=512, H=32768, seed=731)


def make(sd, D, H, precision="auto"):
    m = TernarySparseAutoencoder(D, H)
    m.load_state_dict({name: torch.from_numpy(np.ascontiguousarray(v)) for name, v in sd.items()})
    m.decoder.precision = precision
    return m.to(DEV)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32)


def grads_of(model):
    return {name: (p.grad.detach().clone() if p.grad is not None else None) for name, p in model.named_parameters()}


def fixture_model(name):
    meta, z = U.load_fixture(name)
    sd, x_np = U.masked_params(meta, meta["seed"])
    return meta, z, make(sd, meta["D"], meta["H"]), torch.from_numpy(x_np).to(DEV)


def assert_close(got: dict, want: dict, keys, what=""):
    errs = {key: U.max_rel_err(got[key], want[key]) for key in keys}
    print(what, " ".join(f"{k}: {e:.3g}" for k, e in errs.items()))
    for key, err in errs.items():
        assert err <= TOL, f"{what} {key}: max |err| / max |g| = {err:.3g}"


# ---- forward parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,D,H,B", [("fp32", 64, 256, 24), ("fp32", 32, 1000, 8), ("fp32", 512, 1024, 64),
                                             ("split", 512, 1024, 64), ("auto", 512, 2048, 128)])
def test_forward_train_equals_forward_bit_for_bit(precision, D, H, B):
    model = make(S.ternary_sae_params(741, D, H), D, H, precision)
    model.decoder.init_mask(U.SPARSITY)
    x = torch.from_numpy(S.activations(741, B, D)).to(DEV)
    assert model.decoder.resolved_precision(B) == ("fp32" if precision == "fp32" else "split")
    h0, r0 = model(x)
    h1, r1 = model.forward_train(x)
    assert h1.grad_fn is not None and r1.grad_fn is not None
    assert torch.equal(bits(h0), bits(h1)) and torch.equal(bits(r0), bits(r1))
    assert float(r0.abs().max()) > 0


# ---- the reference's gradients ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_gradients_match_reference_fixtures(name):
    meta, z, model, x = fixture_model(name)
    assert torch.equal(model.decoder.mask.cpu(), torch.from_numpy(U.unpack_mask(z["mask"], meta["D"], meta["H"])))
    x.requires_grad_(True)
    h, recon = model.forward_train(x)
    assert U.max_rel_err(h, z["h"]) <= TOL and U.max_rel_err(recon, z["recon"]) <= TOL
    assert torch.equal(h.detach().cpu() > 0, torch.from_numpy(z["h"]) > 0)
    loss = F.mse_loss(recon, x.detach())
    if meta["l1"] > 0:
        loss = loss + meta["l1"] * h.abs().mean()
    loss.backward()
    assert abs(loss.item() - float(z["loss"])) <= TOL * abs(float(z["loss"]))
    got = grads_of(model)
    got["x"] = x.grad
    assert_close(got, {k: z["grad." + k] for k in U.PARAM_KEYS + ("x",)}, U.PARAM_KEYS + ("x",), what=name)
    dec = model.decoder
    assert U.max_rel_err(dec.activation_mean, z["a"]) <= TOL and U.max_rel_err(dec.output_grad_mean, z["delta"]) <= TOL
    assert dec.input_activations is None and dec.output_grad is None
    assert sorted(model.state_dict()) == ["decoder.mask", "decoder.weight", "encoder.0.bias", "encoder.0.weight"]
    # the backward's gradient is already masked: mask_grad() changes nothing, twice
    before = bits(dec.weight.grad).clone()
    assert bool((dec.weight.grad[dec.mask == 0] == 0).all())
    dec.mask_grad()
    dec.mask_grad()
    assert torch.equal(before, bits(dec.weight.grad))


def test_missing_incoming_gradients():
    meta, z, model, x = fixture_model("train_ternary_d64_l1")
    lin, dec = model.encoder.linear, model.decoder
    B, D, H = meta["B"], meta["D"], meta["H"]
    # gh only: recon unused -> no gradient reaches decoder.weight through the contraction (zeros), delta stays unset
    h, recon = model.forward_train(x)
    (meta["l1"] * h.abs().mean()).backward()
    gh = U.l1_incoming(x, lin.weight, lin.bias, meta["l1"])
    want = U.grads64(x, lin.weight, lin.bias, dec.weight, dec.mask, None, gh, active=h.detach() > 0)
    got = grads_of(model)
    assert_close(got, want, ("encoder.0.weight", "encoder.0.bias"), what="gh only")
    assert got["decoder.weight"] is None or not bool(got["decoder.weight"].any())
    assert dec.output_grad_mean is None
    # G only
    model.zero_grad(set_to_none=True)
    h, recon = model.forward_train(x)
    F.mse_loss(recon, x).backward()
    G = U.trainer_incoming(x, recon.detach(), B, D)
    want = U.grads64(x, lin.weight, lin.bias, dec.weight, dec.mask, G, None, active=h.detach() > 0)
    assert_close(grads_of(model), want, U.PARAM_KEYS, what="G only")
    assert U.max_rel_err(dec.output_grad_mean, G.mean(0)) <= TOL
    # needs_input_grad honoured: a frozen encoder gets nothing
    model.zero_grad(set_to_none=True)
    lin.weight.requires_grad_(False)
    lin.bias.requires_grad_(False)
    h, recon = model.forward_train(x)
    F.mse_loss(recon, x).backward()
    assert lin.weight.grad is None and lin.bias.grad is None
    assert U.max_rel_err(dec.weight.grad, want["decoder.weight"]) <= TOL


# ---- tile edges of each backward kernel on its own ---------------------------------------------------------------------------
def edge_seed(B, D, H):
    return 781 + B + D + H


@pytest.mark.parametrize("H", [4, 132, 1060])
@pytest.mark.parametrize("D", [4, 36, 132])
@pytest.mark.parametrize("B", [1, 24, 257])
def test_kernels_at_tile_edges_against_fp64(B, D, H):
    """train_ternary_rows, train_ternary_dweight and train_ternary_dpre as plain ops calls: B = 1, a partial second tile in every
    dimension (257 = 2 x 128 + 1 rows, D = 132, H = 1060), a K tail in both contractions (D = 36 and 132 against the 32-wide
    slice of dpre, B = 24 and 257 against that of dweight), D = 4 and H = 4.  Measured on an MI355X (max |err| / max |g| over
    the 27 shapes): see DESIGN.md section 4.13."""
    seed = edge_seed(B, D, H)
    sd = S.ternary_sae_params(seed, D, H)
    x = torch.from_numpy(S.activations(seed, B, D)).to(DEV)
    G = torch.from_numpy(S.normal(seed, (B, D), stream=11)).to(DEV)
    gh = torch.from_numpy(S.normal(seed, (B, H), stream=12)).to(DEV)
    # the ternary image, exactly, with the cutoff row of test_kernels_gpu.py::test_ternary_pack_and_decode
    w_np = sd["decoder.weight"].copy()
    row = np.array([0.5, -0.5, 0.49999997, -0.49999997, 0.0, -0.0, np.nan], dtype=np.float32)
    w_np.reshape(-1)[:row.size] = row
    w = torch.from_numpy(w_np).to(DEV)
    t_rows = ops.train_ternary_rows(w)
    w_cpu = torch.from_numpy(w_np)
    want_rows = (torch.sign(w_cpu) * (w_cpu.abs() >= U.THRESHOLD).float()).t()            # sae/ternary.py:47-49; torch.sign(nan) = 0
    assert tuple(t_rows.shape) == (H, D) and torch.equal(t_rows.cpu(), want_rows)          # by value: -1 * 0 = -0.0 equals 0.0
    assert want_rows.t().reshape(-1)[:row.size].tolist() == [1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert bool(((t_rows == 0) | (t_rows.abs() == 1)).all())
    # the rest runs on the model's own dictionary (no nan in a contraction operand)
    t_rows = ops.train_ternary_rows(torch.from_numpy(sd["decoder.weight"]).to(DEV))
    T64 = t_rows.double()                                                                 # [H, D], exact
    h = ops.encode_dense(x, torch.from_numpy(sd["encoder.0.weight"]).to(DEV), torch.from_numpy(sd["encoder.0.bias"]).to(DEV),
                         ops.ACT_RELU)
    pos = h > 0
    frac = float(pos.float().mean())
    if B * H >= 96:
        assert 0.2 <= frac <= 0.8, frac                       # a condition on the inputs: the gate is exercised both ways
    # dweight: the loaders and chain of train_gemm_tn, the mask on the store
    plain = ops.train_gemm_tn(G, h)
    assert tuple(plain.shape) == (D, H)
    ones = torch.ones((D, H), device=DEV)
    assert torch.equal(bits(ops.train_ternary_dweight(G, h, ones)), bits(plain))
    mask = torch.from_numpy((S.uniform01(seed, D * H, stream=13) < 0.3).astype(np.float32).reshape(D, H)).to(DEV)
    dw = ops.train_ternary_dweight(G, h, mask)
    assert torch.equal(bits(dw), bits(plain * mask))
    assert bool((bits(dw)[mask == 0] & 0x7FFFFFFF == 0).all())
    full64 = G.double().t() @ h.double()
    errs = {"dweight": U.max_rel_err(plain, full64), "dweight masked": U.max_rel_err(dw, full64 * mask.double())}
    # dpre: the four null combinations, on the h the kernel reads
    for with_G in (True, False):
        for with_gh in (True, False):
            dpre = ops.train_ternary_dpre(h, G if with_G else None, gh if with_gh else None, t_rows)
            want = torch.zeros((B, H), dtype=torch.float64, device=DEV)
            if with_G:
                want = want + G.double() @ T64.t()
            if with_gh:
                want = want + gh.double()
            want = want * pos
            assert tuple(dpre.shape) == (B, H) and bool((dpre[~pos] == 0).all())
            if not with_G and not with_gh:
                assert not bool(dpre.any())
            errs[f"dpre G {int(with_G)} gh {int(with_gh)}"] = U.max_rel_err(dpre, want)
    print(f"B {B} D {D} H {H} active {frac:.3f}:", " ".join(f"{k}: {e:.3g}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= TOL, f"B {B} D {D} H {H} {k}: max |err| / max |g| = {e:.3g}"


# ---- full size ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    B, D, H, seed = (FULL[k] for k in ("B", "D", "H", "seed"))
    model = make(S.ternary_sae_params(seed, D, H), D, H)
    model.decoder.init_mask(U.SPARSITY)
    x = torch.from_numpy(S.activations(seed, B, D)).to(DEV)
    return model, x


def full_step(model, x, l1=1e-3, want_dx=True):
    model.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(want_dx)
    h, recon = model.forward_train(xr)
    loss = F.mse_loss(recon, x) + l1 * h.abs().mean()
    loss.backward()
    g = grads_of(model)
    g["x"] = xr.grad
    return h.detach(), recon.detach(), g


def test_full_size_gradients_against_fp64_table(full):
    """B = 8192, D = 512, H = 32768: every unit of every gradient (and dx, a, delta) against the fp64 table on the forward's own
    ReLU pattern.  Measured on an MI355X (max |err| / max |g|): see DESIGN.md section 4.13."""
    model, x = full
    lin, dec = model.encoder.linear, model.decoder
    B, D, H = FULL["B"], FULL["D"], FULL["H"]
    l1 = 1e-3
    h, recon, got = full_step(model, x, l1)
    active = h > 0
    frac = float(active.float().mean())
    assert 0.2 < frac < 0.8, frac
    G = U.trainer_incoming(x, recon, B, D)

    def gh(units):
        return l1 * active[:, torch.as_tensor(units).to(DEV)].to(torch.float64) / (B * H)
    want = U.grads64(x, lin.weight, lin.bias, dec.weight, dec.mask, G, gh, want_dx=True, active=active, chunk=2048)
    got["a"], got["delta"], want["delta"] = dec.activation_mean, dec.output_grad_mean, G.mean(0)
    assert_close(got, want, U.PARAM_KEYS + ("x", "a", "delta"), what=f"full size (active {frac:.3f})")
    assert bool((got["decoder.weight"][dec.mask == 0] == 0).all())


def test_full_size_step_is_bitwise_reproducible(full):
    model, x = full
    dec = model.decoder
    w0, m0 = dec.weight.detach().clone(), dec.mask.clone()
    runs = []
    for _ in range(2):
        with torch.no_grad():
            dec.weight.copy_(w0)
            dec.mask.copy_(m0)
        _, _, g = full_step(model, x)
        dec.update_mask(0.3, U.SPARSITY)
        runs.append((g, dec.weight.detach().clone(), dec.mask.clone()))
    (g0, w_a, m_a), (g1, w_b, m_b) = runs
    for k in g0:
        assert torch.equal(bits(g0[k]), bits(g1[k])), k
    assert torch.equal(bits(w_a), bits(w_b)) and torch.equal(bits(m_a), bits(m_b))
    assert not torch.equal(m_a, m0)
    with torch.no_grad():
        dec.weight.copy_(w0)
        dec.mask.copy_(m0)


# ---- masks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.MASK_CASES))
def test_masks_match_reference_fixtures_bitwise(name):
    meta, z = U.load_fixture(name)
    D, H = meta["D"], meta["H"]
    w0, a, delta = U.mask_case_inputs(meta, meta["seed"])
    sd = S.ternary_sae_params(meta["seed"], D, H)
    sd["decoder.weight"] = w0
    model = make(sd, D, H)
    dec = model.decoder
    dec.init_mask(U.SPARSITY)
    assert torch.equal(dec.mask.cpu(), torch.from_numpy(U.unpack_mask(z["mask_init"], D, H)))
    if meta["ties"]:
        with torch.no_grad():
            dec.weight.copy_(torch.from_numpy(z["weight_before"]).to(DEV))
    assert torch.equal(bits(dec.weight).cpu(), torch.from_numpy(z["weight_before"]).view(torch.int32))
    if meta["stats"]:
        dec.activation_mean, dec.output_grad_mean = torch.from_numpy(a).to(DEV), torch.from_numpy(delta).to(DEV)
    dec.update_mask(meta["f_decay"], U.SPARSITY)
    assert torch.equal(dec.mask.cpu(), torch.from_numpy(U.unpack_mask(z["mask_after"], D, H)))
    assert torch.equal(bits(dec.weight).cpu(), torch.from_numpy(z["weight_after"]).view(torch.int32))
    assert int(dec.mask.sum()) == meta["active_after"]


def test_mask_ties_are_taken_in_ascending_flat_index():
    """Exactly-k selections with ties AT the boundary: quantised |w| and quantised statistics give thousands of equal keys."""
    D, H = 32, 1000
    sd = S.ternary_sae_params(751, D, H)
    sd["decoder.weight"] = (np.round(sd["decoder.weight"] * 8) / 8).astype(np.float32)
    model = make(sd, D, H)
    dec = model.decoder
    w0 = dec.weight.detach().clone()
    dec.init_mask(U.SPARSITY)
    w1, m1 = U.init_mask_ref(w0, U.SPARSITY)
    assert torch.equal(dec.mask, m1) and torch.equal(bits(dec.weight), bits(w1))
    assert int(dec.mask.sum()) == D * H - int(D * H * U.SPARSITY)
    a = torch.from_numpy(np.round(np.abs(S.normal(751, (H,), stream=5)) * 2) / 2).float().to(DEV)
    delta = torch.from_numpy(np.round(S.normal(751, (D,), stream=6) * 2) / 2).float().to(DEV)
    n = U.update_n(D * H, 0.3)
    w2, m2, info = U.update_mask_ref(w1, m1, a, delta, n)
    assert info["grow_key"] == info["grow_next_key"] and int(info["dropped"].sum()) > n      # ties at both boundaries
    dec.activation_mean, dec.output_grad_mean = a, delta
    dec.update_mask(0.3, U.SPARSITY)
    assert torch.equal(dec.mask, m2) and torch.equal(bits(dec.weight), bits(w2))


def test_full_size_masks_against_restatement(full):
    """512 x 32768: init_mask and update_mask against the util's exact restatement on the same device, every position
    compared (the restatement takes ties in ascending flat index, so no position is exempt)."""
    model, x = full
    D, H = FULL["D"], FULL["H"]
    dec = model.decoder
    w_raw = torch.from_numpy(S.ternary_sae_params(FULL["seed"], D, H)["decoder.weight"]).to(DEV)
    w1, m1 = U.init_mask_ref(w_raw, U.SPARSITY)
    w_saved, m_saved = dec.weight.detach().clone(), dec.mask.clone()
    assert torch.equal(m_saved, m1) and torch.equal(bits(w_saved), bits(w1))
    assert int(m1.sum()) == D * H - int(D * H * U.SPARSITY)
    a = torch.from_numpy(np.abs(S.normal(FULL["seed"], (H,), stream=5))).float().to(DEV)
    delta = (torch.from_numpy(S.normal(FULL["seed"], (D,), stream=6)).float() * 1e-3).to(DEV)
    try:
        for f_decay, stats in ((0.3, True), (0.1, True), (0.3, False), (0.0, True)):
            with torch.no_grad():
                dec.weight.copy_(w_saved)
                dec.mask.copy_(m_saved)
            dec.activation_mean, dec.output_grad_mean = (a, delta) if stats else (None, None)
            n = U.update_n(D * H, f_decay)
            w2, m2, info = U.update_mask_ref(w_saved, m_saved, a if stats else None, delta if stats else None, n)
            dec.update_mask(f_decay, U.SPARSITY)
            got_m, got_w = dec.mask, dec.weight.detach()
            dropped = (m_saved != 0) & ~((got_m != 0) & ~info["grown"].reshape(D, H))
            print(f"f_decay {f_decay} stats {stats}: n {n} dropped {int(info['dropped'].sum())} grown {int(info['grown'].sum())} "
                  f"active {int(got_m.sum())} mask differences {int((got_m != m2).sum())}")
            assert int(got_m.sum()) == int(m2.sum())
            assert torch.equal(dropped, info["dropped"].reshape(D, H))
            assert torch.equal(got_m, m2) and torch.equal(bits(got_w), bits(w2))
    finally:
        with torch.no_grad():
            dec.weight.copy_(w_saved)
            dec.mask.copy_(m_saved)
        dec.activation_mean = dec.output_grad_mean = None
        dec.invalidate_packed()


def test_update_mask_saturates_and_check_refuses():
    D, H = 64, 256
    model = make(S.ternary_sae_params(761, D, H), D, H)
    dec = model.decoder
    dec.init_mask(0.9)                                        # 1639 active
    active = int(dec.mask.sum())
    w0, m0 = dec.weight.detach().clone(), dec.mask.clone()
    n = U.update_n(D * H, 0.5)                                # 2457 > active
    assert n > active
    with pytest.raises(ValueError, match="above the"):
        dec.update_mask(0.5, U.SPARSITY, check=True)
    assert torch.equal(bits(dec.weight), bits(w0)) and torch.equal(dec.mask, m0)
    with pytest.raises(ValueError):
        dec.update_mask(5.0, U.SPARSITY)                      # n > numel: host arithmetic
    with pytest.raises(ValueError):
        dec.update_mask(-0.1, U.SPARSITY)
    assert torch.equal(bits(dec.weight), bits(w0)) and torch.equal(dec.mask, m0)
    dec.update_mask(0.5, U.SPARSITY)                          # default: every active position drops, nothing to grow from
    assert int(dec.mask.sum()) == 0 and not bool(dec.weight.detach().any())
    # thousands of ties at both boundaries: zero weights at the drop threshold, equal scores at the grow boundary
    with torch.no_grad():
        dec.weight.copy_(w0)
        dec.mask.fill_(1.0)
    dec.activation_mean = torch.ones(H, device=DEV)
    dec.output_grad_mean = torch.ones(D, device=DEV)
    w1, m1 = dec.weight.detach().clone(), dec.mask.clone()
    n = U.update_n(D * H, 0.3)
    w2, m2, info = U.update_mask_ref(w1, m1, dec.activation_mean, dec.output_grad_mean, n)
    assert int(info["dropped"].sum()) > n and info["grow_key"] == info["grow_next_key"]
    dec.update_mask(0.3, U.SPARSITY)
    assert torch.equal(dec.mask, m2) and torch.equal(bits(dec.weight), bits(w2))


def test_forward_train_refusals():
    with pytest.raises(ValueError, match="multiple of 4 up to"):
        TernarySparseAutoencoder(66, 256).to(DEV).forward_train(torch.zeros(2, 66, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4 up to"):
        TernarySparseAutoencoder(4100, 8).to(DEV).forward_train(torch.zeros(2, 4100, device=DEV))
    m = TernarySparseAutoencoder(64, 256).to(DEV)
    with pytest.raises(ValueError, match=r"expected \[batch, 64\]"):
        m.forward_train(torch.zeros(2, 32, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_train(torch.zeros(2, 64))


def test_forward_sees_mask_updates_without_cache_reset():
    D, H, B = 512, 1024, 64
    model = make(S.ternary_sae_params(771, D, H), D, H)
    x = torch.from_numpy(S.activations(771, B, D)).to(DEV)
    dec = model.decoder
    model(x)                                                   # fills the packed caches from the unmasked weights
    model.forward_train(x)
    for stage in ("init", "update"):
        if stage == "init":
            dec.init_mask(U.SPARSITY)
        else:
            h, recon = model.forward_train(x)
            F.mse_loss(recon, x).backward()
            dec.update_mask(0.3, U.SPARSITY)
        fresh = make({k: v.cpu().numpy() for k, v in model.state_dict().items()}, D, H)
        (h0, r0), (h1, r1) = model(x), fresh(x)
        assert torch.equal(bits(h0), bits(h1)) and torch.equal(bits(r0), bits(r1)), stage
        assert torch.equal(bits(dec.ternary_rows()), bits(fresh.decoder.ternary_rows())), stage
        assert torch.equal(bits(model.forward_train(x)[1]), bits(r1)), stage


# ---- the trainer loop ------------------------------------------------------------------------------------------------------------
def test_trainer_loop_reproduces_reference_loss_curve():
    """30 steps of the t_sae branch (forward, mse_loss, backward, mask_grad, Adam, update_mask) through this package against
    the reference's fp64 loss curve, within max(10 * gap, 1e-5) relative.  The number of positions where the final mask differs
    from the reference's is printed, not gated (expected 0): each single update is gated bitwise by the tests above."""
    meta, z = U.load_fixture(U.LOOP_FIXTURE)
    D, H, B = meta["D"], meta["H"], meta["B"]
    model = make(S.ternary_sae_params(meta["seed"], D, H), D, H)
    model.decoder.init_mask(meta["sparsity"])
    x = torch.from_numpy(S.activations(meta["seed"], B, D)).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=meta["lr"])
    losses = []
    for _ in range(meta["steps"]):
        _, recon = model.forward_train(x)
        loss = F.mse_loss(recon, x)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        model.decoder.mask_grad()
        opt.step()
        model.decoder.update_mask(meta["f_decay"], meta["sparsity"])
        losses.append(float(loss.item()))
    losses = np.array(losses)
    rel = np.abs(losses - z["loss64"]) / np.abs(z["loss64"])
    bound = max(10 * meta["gap"], 1e-5)
    final = model.decoder.mask.cpu().numpy()
    diff = int((final != U.unpack_mask(z["mask_final"], D, H)).sum())
    print(f"loop: loss {losses[0]:.4f} -> {losses[-1]:.4f}  max relative deviation from fp64 {rel.max():.3g} (bound {bound:.3g})  "
          f"final active {int(final.sum())}  mask differences {diff}")
    assert losses[-1] < losses[0]
    assert rel.max() <= bound, f"max relative deviation {rel.max():.3g} at step {int(rel.argmax())}"
    assert int(final.sum()) == meta["active_final"]
