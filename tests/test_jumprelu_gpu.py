"""JumpReLU on the GPU (csrc/jumprelu.hip, include/qsae_jump.h): both entry points between guard words, twice on one workspace of
exactly the sizer's bytes, bit for bit against the numpy restatement of tests/jumprelu_util.py; both front ends; the dispatcher
ops; and the two top-k model classes: forward_jumprelu, forward_train_jumprelu and every gradient against the existing ragged
ops driven by hand on the restated lists, the capped selection against the dense mask, all gradients against a dense fp64
formulation with the paper's straight-through estimator, and the Trainer's ``jumprelu``."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import batch_topk_util as BU  # noqa: E402
import guard_util as GU  # noqa: E402
import jumprelu_util as U  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import FeatureActivity, JumpReLU, Trainer, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64, F32 = torch.int32, torch.int64, torch.float32
NAMES = ("idx_sel", "val_sel", "counts", "idx_band", "counts_band", "l0", "report")


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def same(got, want, what=""):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = host(want) if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gb, wb = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
    assert np.array_equal(gb, wb), f"{what}: {int((gb != wb).sum())} bytes differ"


# ---- both entry points between guard words ------------------------------------------------------------------------------
KS, BS, HS = (1, 5, 64, 65, 256), (1, 3, 70), (8, 300)
GRAD_KINDS = ("mixed", "special", "mixed_no_gv", "mixed_no_g_l0")


def _expected_select(want):
    out = {n: torch.from_numpy(np.ascontiguousarray(w)) for n, w in zip(NAMES, want) if n != "l0"}
    out["l0"] = torch.tensor([want[5]], dtype=F32)
    return out


def _guard_select(kind, B, K, H, off=0):
    """``off``: every 4-byte operand starts that many bytes past a 16-byte boundary (the header asks for 4-byte alignment)"""
    def build():
        idx, val, theta, eps = U.case(kind, B, K, H, seed=3)
        want = U.jump_select(idx, val, theta, eps)

        def front(t):
            return dict(zip(NAMES, ops.jump_select(t["idx"], t["val"], t["theta"], float(eps))))
        return Call(f"{kind}_{B}x{K}_H{H}_off{off}", "qsaej_jump_select",
                    [Buf("idx", "in", dev(idx), offset_bytes=off), Buf("val", "in", dev(val), offset_bytes=off), B, K,
                     Buf("theta", "in", dev(theta), offset_bytes=off), H, float(eps), float(U.half_eps(eps)),
                     Buf("idx_sel", "out", shape=(B, K), dtype=I32, offset_bytes=off),
                     Buf("val_sel", "out", shape=(B, K), dtype=F32, offset_bytes=off),
                     Buf("counts", "out", shape=(B,), dtype=I32, offset_bytes=off),
                     Buf("idx_band", "out", shape=(B, K), dtype=I32, offset_bytes=off),
                     Buf("counts_band", "out", shape=(B,), dtype=I32, offset_bytes=off),
                     Buf("l0", "out", shape=(1,), dtype=F32, offset_bytes=off), Buf("report", "out", shape=(6,), dtype=I64),
                     WS, WS_BYTES, STREAM], front, sizer=("qsaej_jump_select_workspace_bytes", (B, K, H)),
                    expect=_expected_select(want))
    return build


def _guard_grad(kind, B, K, H, off=0):
    def build():
        idx, val, theta, eps = U.case(kind.split("_no_")[0], B, K, H, seed=3)
        sel = U.jump_select(idx, val, theta, eps)
        offsets, entries = BU.csr_ragged(sel[3], sel[4], H)
        rng = np.random.default_rng(B * K + H)
        gv = None if kind.endswith("no_gv") else rng.standard_normal((B, K)).astype(np.float32)
        g_l0 = None if kind.endswith("no_g_l0") else np.float32(0.375)
        want = U.threshold_grad(offsets, entries, gv, theta, g_l0, B, eps)

        def front(t):
            return {"dtheta": ops.jump_threshold_grad(t["offsets"], t["entries"], t.get("gv"), t["theta"], t.get("g_l0"), B, K, float(eps))}
        return Call(f"{kind}_{B}x{K}_H{H}_off{off}", "qsaej_threshold_grad",
                    [Buf("offsets", "in", dev(offsets), offset_bytes=off), Buf("entries", "in", dev(entries), offset_bytes=off),
                     Buf("gv", "in", dev(gv), offset_bytes=off) if gv is not None else None,
                     Buf("theta", "in", dev(theta), offset_bytes=off),
                     Buf("g_l0", "in", dev(np.array([g_l0], np.float32)), offset_bytes=off) if g_l0 is not None else None,
                     B, K, H, float(eps), Buf("dtheta", "out", shape=(H,), dtype=F32, offset_bytes=off), STREAM], front,
                    expect={"dtheta": torch.from_numpy(want)})
    return build


def _guard_cases():
    cases = {}
    for K in KS:
        for H in HS:
            for B in BS:
                for kind in U.KINDS:
                    cases[f"select_{kind}_{B}x{K}_H{H}"] = ("qsaej_jump_select", _guard_select(kind, B, K, H))
                for kind in GRAD_KINDS:
                    cases[f"grad_{kind}_{B}x{K}_H{H}"] = ("qsaej_threshold_grad", _guard_grad(kind, B, K, H))
            cases[f"select_special_70x{K}_H{H}_off4"] = ("qsaej_jump_select", _guard_select("special", 70, K, H, off=4))
            cases[f"grad_mixed_70x{K}_H{H}_off4"] = ("qsaej_threshold_grad", _guard_grad("mixed", 70, K, H, off=4))
    return cases


#: label -> (entry point, builder of its guard_util.Call); tests/test_jumprelu_host.py reads the entry points for its ledger.
#: Building a case touches the GPU; importing this table does not.
GUARD_CASES = _guard_cases()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("K", KS)
def test_entry_points_between_guard_words(K, H):
    labels = [label for label in sorted(GUARD_CASES) if label.replace("_off4", "").endswith(f"x{K}_H{H}")]
    assert len(labels) == len(BS) * (len(U.KINDS) + len(GRAD_KINDS)) + 2
    for label in labels:
        entry, build = GUARD_CASES[label]
        call = build()
        assert call.entry == entry
        GU.run_call(call, _lib.load(), DEV)


def test_hand_cases_and_both_front_ends():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    eps = 0.5
    theta = np.array([1.0, 2.0, 0.5, nan, inf, 0.0], np.float32)
    idx = np.array([[0, 1, -1, 6, 2, 0, 3, 4, 5]], dtype=np.int32)
    val = np.array([[1.0, nan, 9.0, 9.0, 0.75, 0.875, 7.0, inf, -0.0]], np.float32)
    want = U.jump_select(idx, val, theta, eps)
    assert want[0][0].tolist() == [2, 0, 1, -1, 6, 0, 3, 4, 5] and want[3][0].tolist() == [0, 0, 5, 1, -1, 6, 2, 3, 4]
    for mod in (ops, torch_ops):
        got = mod.jump_select(dev(idx), dev(val), dev(theta), eps)
        for g, w, name in zip(got, want, NAMES):
            same(g, np.array([w], np.float32) if name == "l0" else w, name)
        got = mod.jump_select(dev(idx), dev(val), dev(theta), eps, want_band=False)
        assert got[3] is None and got[4] is None
        same(got[0], want[0]), same(got[1], want[1]), same(got[2], want[2]), same(got[6], want[6])
    offsets, entries = np.array([0, 0, 2, 3], dtype=np.int32), np.array([1, 4, 2, -1, -1, -1], dtype=np.int32)
    gv = np.array([9, 0.5, -2.0, 9, 0.25, 9], np.float32).reshape(3, 2)
    for mod in (ops, torch_ops):
        d = mod.jump_threshold_grad(dev(offsets), dev(entries), dev(gv), dev(np.array([5.0, 2.0, 4.0], np.float32)),
                                    torch.full((1,), 3.0, device=DEV), 3, 2, 0.5)
        assert host(d).tolist() == [0.0, -7.0, 14.0] and not np.signbit(host(d)[0])
    # B == 0: the selection launches nothing, the gradient is zeros
    empty = ops.jump_threshold_grad(dev(np.zeros(4, np.int32)), dev(np.zeros(0, np.int32)), None, dev(theta[:3]), None, 0, 2, 0.5)
    assert host(empty).tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="bandwidth"):
        ops.jump_select(dev(idx), dev(val), dev(theta), 0.0)
    with pytest.raises(ValueError, match="expected two"):
        ops.jump_select(dev(idx), dev(val[:, :4]), dev(theta), 0.5)


def test_dispatcher_ops():
    idx, val, theta, eps = U.case("mixed", 70, 65, 300, seed=3)
    Q = torch.ops.qsae
    torch.library.opcheck(Q.jump_select.default, (dev(idx), dev(val), dev(theta), float(eps), True))
    torch.library.opcheck(Q.jump_select.default, (dev(idx), dev(val), dev(theta), float(eps), False))
    sel = U.jump_select(idx, val, theta, eps)
    offsets, entries = BU.csr_ragged(sel[3], sel[4], 300)
    torch.library.opcheck(Q.jump_threshold_grad.default, (dev(offsets), dev(entries), dev(val), dev(theta),
                                                          torch.full((1,), 0.5, device=DEV), 70, 65, float(eps)))
    torch.library.opcheck(Q.jump_threshold_grad.default, (dev(offsets), dev(entries), None, dev(theta), None, 70, 65, float(eps)))


# ---- the two top-k model classes ----------------------------------------------------------------------------------------
D_, H_, K_, CAP_, B_ = 32, 256, 8, 32, 70
EPS = 0.25                                                    # wide enough for a few hundred band entries at these shapes
L0_COEF = 0.05
CONFIG = {"input_dim": D_, "n_bits": 4, "hidden_dim": H_, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": K_,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": B_}
KIND = {"baseline_sae": "baseline", "b_sae": "binary"}
SEED = 11


def _state(kind: str):
    if kind == "baseline":
        return S.baseline_sae_params(SEED, D_, H_, bias_std=0.1)
    return S.binary_sae_params(SEED, D_, H_, 4, dec_bias_std=0.1, logit_std=0.5)


def _model(kind: str):
    if kind == "baseline":
        model = BaselineSparseAutoencoder(D_, H_)
        model.topk = K_
    else:
        model = BinarySAE(D_, H_, gamma=4.0, n_bits=4)
        model.k = (K_ + 0.5) / H_
        assert model.top_k == K_
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _state(kind).items()})
    return model.to(DEV)


def _controller(model, rows, cap=CAP_):
    """thresholds calibrated at the model's k on the batch, then jittered per unit"""
    jr = JumpReLU(model, cap=cap, bandwidth=EPS)
    before = jr.log_threshold.detach().clone()
    jr.calibrate(rows, K_)
    assert not torch.equal(jr.log_threshold.detach(), before) and len(set(host(jr.log_threshold).tolist())) == 1
    jitter = np.random.default_rng(5).standard_normal(H_).astype(np.float32) * np.float32(0.2)
    with torch.no_grad():
        jr.log_threshold += dev(jitter)
    return jr


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.fixture(scope="module")
def rows():
    return dev(S.activations(91, B_, D_))


def test_calibrate_is_the_batch_topk_threshold(rows):
    model = _model("baseline")
    jr = JumpReLU(model, cap=CAP_)
    jr.calibrate(rows, K_)
    _, val = model._select_cap(rows, CAP_, "test")
    report = BU.batch_select(host(val), B_ * K_)[2]
    m = np.array([report[3]], dtype=np.uint32).view(np.float32)[0]
    assert m > 0
    same(jr.log_threshold, torch.full((H_,), float(m), device=DEV).log(), "every threshold is the smallest selected value")
    # with every threshold at that value the selection holds what BatchTopK selects, minus the entries equal to it
    counts = host(model.forward_jumprelu(rows, jr)[2])
    assert int(counts.sum()) <= B_ * K_ and int(counts.sum()) >= B_ * K_ - 2
    # a selection whose smallest value is not > 0 -- every pre-activation of the batch -- leaves the thresholds as they are
    wide = JumpReLU(model, cap=H_)
    kept = wide.log_threshold.detach().clone()
    wide.calibrate(rows, H_)
    _, all_vals = model._select_cap(rows, H_, "test")
    assert float(all_vals.detach().min()) < 0
    same(wide.log_threshold, kept)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_jumprelu(sae_type, rows):
    model = _model(KIND[sae_type])
    jr = _controller(model, rows)
    idx_sel, val_sel, counts, recon = model.forward_jumprelu(rows, jr)
    idx, val = model._select_cap(rows, CAP_, "test")
    want = U.jump_select(host(idx), host(val), host(jr.thresholds()), EPS)
    same(idx_sel, want[0], "idx_sel"), same(val_sel, want[1], "val_sel"), same(counts, want[2], "counts")
    same(jr.report, want[6], "report"), same(jr.counts, want[2])
    assert len(set(want[2].tolist())) > 1 and 0 < int(want[2].sum()) < B_ * CAP_
    decoder, bias = model._nested_decoder()
    hd = (decoder[0], host(decoder[1])) + ((D_,) if decoder[0] == "packed" else ()) + tuple(decoder[2:])
    same(recon, BU.decode_ragged(want[0], want[1], want[2], hd, host(bias)), "decoded from what forward() decodes from")
    # ... and bit for bit the existing sparse decode of the masked list at width K (a finite dictionary)
    sel, _ = U.predicates(host(idx), host(val), host(jr.thresholds()), EPS)
    masked = dev(np.where(sel, host(val), np.float32(0)).astype(np.float32))
    if decoder[0] == "packed":
        plain = ops.decode_binary_sparse(idx, masked, decoder[1], D_, decoder[2], decoder[3], bias)
    else:
        plain = ops.decode_table_sparse(idx, masked, decoder[1], decoder[2], bias)
    same(recon, plain, "the masked width-K list")
    s = jr.summary()
    assert s["selected"] == int(want[2].sum()) and s["l0"] == s["selected"] / B_ and s["uncertified_rows"] == int(want[6][4])
    assert np.float32(s["theta_min"]) == host(jr.thresholds()).min()
    with pytest.raises(ValueError, match="expected \\[batch"):
        model.forward_jumprelu(rows[:, :8], jr)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_train_jumprelu_outputs_and_gradients(sae_type, rows):
    model = _model(KIND[sae_type])
    model.activity = FeatureActivity.for_model(model)
    jr = _controller(model, rows)
    x = rows.clone().requires_grad_()
    out = model.forward_train_jumprelu(x, jr)
    latent, recon, l0 = out[0], out[1], out[-1]
    assert len(out) == (4 if sae_type == "b_sae" else 3) and all(o.grad_fn is not None for o in out) and l0.dim() == 0
    lin, dec = model.encoder.linear, model.decoder
    theta = jr.thresholds()
    idx, val = model._select_cap(rows, CAP_, "test")
    want = U.jump_select(host(idx), host(val), host(theta), EPS)
    w_idx_sel, w_val_sel, w_counts, w_idx_band, w_counts_band, w_l0, w_report = want
    assert int(w_report[1]) > 50 and (w_counts_band > 0).sum() > 10      # the band is not empty: the threshold gradient is live
    same(jr.counts, w_counts, "counts"), same(jr.report, w_report, "report"), same(l0, np.float32(w_l0), "l0")
    same(latent, ops.densify(dev(w_idx_sel), dev(w_val_sel), H_), "latent")
    table, step, _ = model._nested_train_decoder()
    same(recon, BU.decode_ragged(w_idx_sel, w_val_sel, w_counts, ("table", host(table), step), host(dec.bias)), "reconstruction")
    assert np.array_equal(host(model.activity.fired), np.bincount(w_idx_sel[w_val_sel > 0], minlength=H_))
    g_const = torch.full((), L0_COEF, dtype=F32, device=DEV)
    trainer_loss(sae_type, out[:-1], rows, CONFIG, extra=[(l0, g_const)])
    got = _grads(model)
    # bit for bit the existing ragged ops driven by hand on the restated lists
    coef = 0.5 if sae_type == "b_sae" else 1.0
    g_recon = ops.trainer_loss(rows, [recon.detach()], 0, coef)[1][0]
    d_idx_sel, d_counts = dev(w_idx_sel), dev(w_counts)
    gv, dx = ops.train_row_grad_ragged(d_idx_sel, d_counts, table, step, g_recon, None, lin.weight.detach(), True)
    off, ent = ops.train_csr_ragged(d_idx_sel, d_counts, H_)
    g_pol = torch.full((), CONFIG["polarize_lambda"], dtype=F32, device=DEV) if sae_type == "b_sae" else None
    dW, db, ddec = model._batch_unit_grad(off, ent, dev(w_val_sel), gv, rows, g_recon, g_pol, True, True)
    same(got["encoder.0.weight"], dW, "dW_enc"), same(got["encoder.0.bias"], db, "db_enc"), same(got["decoder.weight"], ddec, "d decoder")
    same(got["decoder.bias"], ops.train_col_sum(g_recon), "db_dec"), same(x.grad, dx, "dx")
    # the thresholds: the restatement on the band lists, times theta (torch's own exp backward)
    gv_band, _ = ops.train_row_grad_ragged(dev(w_idx_band), dev(w_counts_band), table, step, g_recon, None, None, False)
    w_gv_band, _ = BU.row_grad_ragged(w_idx_band, w_counts_band, host(table), step, host(g_recon), None, None)
    same(gv_band, w_gv_band, "gv over the band lists")
    offsets, entries = BU.csr_ragged(w_idx_band, w_counts_band, H_)
    dtheta = U.threshold_grad(offsets, entries, w_gv_band, host(theta), np.float32(L0_COEF), B_, EPS)
    assert np.count_nonzero(dtheta) > 10
    same(jr.log_threshold.grad, dev(dtheta) * jr.log_threshold.detach().exp(), "log_threshold.grad")
    # without a gradient for the thresholds nothing of the band is computed, and the other gradients are the same bits
    model.zero_grad(set_to_none=True)
    jr.log_threshold.requires_grad_(False)
    out2 = model.forward_train_jumprelu(rows, jr, dense_latent=False)
    assert out2[0] is None
    trainer_loss(sae_type, out2[:-1], rows, CONFIG)
    for k, g in _grads(model).items():
        same(g, got[k], k)


def test_with_the_cap_at_hidden_dim_it_is_the_dense_mask(rows):
    model = _model("baseline")
    jr = _controller(model, rows, cap=H_)
    idx_sel, val_sel, counts, _ = model.forward_jumprelu(rows, jr)
    assert int(jr.report[4]) == 0                              # K == H: no row is uncertified
    dense = model.encoder(rows.clone())                        # the model's own dense latent (pre-activations, no ReLU)
    mask = dense > jr.thresholds()[None, :]
    got = torch.zeros_like(mask)
    hi, hc = host(idx_sel), host(counts)
    for r in range(B_):
        got[r, hi[r, :hc[r]].tolist()] = True
    assert torch.equal(got, mask) and int(mask.sum()) == int(jr.report[0])
    same(ops.densify(idx_sel, val_sel, H_), torch.where(mask, dense, torch.zeros_like(dense)), "the dense latent")


class _JumpSTE(torch.autograd.Function):
    """z * H(z - theta) with the paper's pseudo-derivative: d/dtheta = -(theta / eps) * rect((z - theta) / eps)"""
    @staticmethod
    def forward(ctx, z, theta, eps):
        ctx.save_for_backward(z, theta)
        ctx.eps = eps
        return z * (z > theta)

    @staticmethod
    def backward(ctx, g):
        z, theta = ctx.saved_tensors
        rect = ((z - theta).abs() < ctx.eps / 2).double()
        return g * (z > theta), (-(theta / ctx.eps) * rect * g).sum(0), None


class _StepSTE(torch.autograd.Function):
    """H(z - theta) with the paper's pseudo-derivative: d/dtheta = -(1 / eps) * rect((z - theta) / eps), none for z"""
    @staticmethod
    def forward(ctx, z, theta, eps):
        ctx.save_for_backward(z, theta)
        ctx.eps = eps
        return (z > theta).double()

    @staticmethod
    def backward(ctx, g):
        z, theta = ctx.saved_tensors
        rect = ((z - theta).abs() < ctx.eps / 2).double()
        return None, (-(1.0 / ctx.eps) * rect * g).sum(0), None


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_gradients_against_a_dense_fp64_jumprelu(sae_type, rows):
    """The whole objective written densely over [B, H] in fp64 with the paper's STE.  Every gradient element is a nested sum of
    products; an fp32 evaluation of such a sum differs from the exact one by at most (number of roundings on the longest path)
    x 2^-24 x (the same sum over the absolute values of its terms), first order -- the bound of tests/evaluation_util.py's
    fp32_sum_bound, applied to the whole expression.  The absolute sums come from running the same formulas on absolute values;
    the count N_TERMS adds up the lengths of the chained sums.  No constant is picked by eye."""
    cap = 128                                                 # the 128th of 256 pre-activations is far below every threshold
    model = _model(KIND[sae_type])
    jr = _controller(model, rows, cap=cap)
    out = model.forward_train_jumprelu(rows, jr)
    assert int(jr.report[4]) == 0                              # every row certified: the capped selection is the dense one
    trainer_loss(sae_type, out[:-1], rows, CONFIG, extra=[(out[-1], torch.full((), L0_COEF, dtype=F32, device=DEV))])
    got = {k: g.cpu().double() for k, g in _grads(model).items()}
    got["log_threshold"] = jr.log_threshold.grad.cpu().double()

    lin, dec = model.encoder.linear, model.decoder
    coef = 0.5 if sae_type == "b_sae" else 1.0
    _, step, _ = model._nested_train_decoder()
    W = lin.weight.detach().cpu().double().requires_grad_()
    b = lin.bias.detach().cpu().double().requires_grad_()
    dp = dec.weight.detach().cpu().double().requires_grad_()
    bd = dec.bias.detach().cpu().double().requires_grad_()
    theta = jr.thresholds().cpu().double().requires_grad_()    # the fp32 thresholds as the leaf: d log = d theta * theta
    x64 = rows.cpu().double()
    lam = CONFIG["polarize_lambda"]
    if sae_type == "baseline_sae":
        t64, pol = dp.t(), 0.0
    else:
        bw = 2.0 ** torch.arange(4, dtype=torch.float64)
        pw = bw.clone()
        bw[-1] = -bw[-1]
        p = torch.sigmoid(dp).view(H_, D_, 4)
        t64, pol = (p * bw).sum(-1), lam * (p * (1 - p) * pw).mean()
    z = x64 @ W.t() + b
    a = _JumpSTE.apply(z, theta, EPS)
    r64 = step * (a @ t64) + bd
    l0 = _StepSTE.apply(z, theta, EPS).sum(1).mean()
    (coef * ((r64 - x64) ** 2).mean() + pol + L0_COEF * l0).backward()
    want = {"encoder.0.weight": W.grad, "encoder.0.bias": b.grad, "decoder.weight": dp.grad, "decoder.bias": bd.grad,
            "log_threshold": theta.grad * theta.detach()}
    # the fp64 masks are the GPU's: no pre-activation lies within rounding of its threshold or of the band's edge
    sel = (z.detach() > theta.detach())
    assert torch.equal(sel.sum(1).int(), jr.counts.cpu()) and int(sel.sum()) == int(jr.report[0])
    band = ((z.detach() - theta.detach()).abs() < EPS / 2)
    assert int(band.sum()) == int(jr.report[1]) > 50

    # the same formulas on absolute values
    with torch.no_grad():
        xa, Wa, ba, ta_, bda, th = x64.abs(), W.abs(), b.abs(), t64.abs(), bd.abs(), theta.detach()
        if sae_type == "b_sae":
            ta_ = (p * bw.abs()).sum(-1)
        za = xa @ Wa.t() + ba
        aa = za * sel
        ea = step * (aa @ ta_) + bda + xa                      # |reconstruction| + |target|
        ga = 2 * coef * ea / (B_ * D_)
        gva = step * (ga @ ta_.t())                            # [B, H]: |dL/dz| of a unit, selected or not
        dTa = step * (aa.t() @ ga)                             # [H, D]
        bound_abs = {"encoder.0.weight": (gva * sel).t() @ xa, "encoder.0.bias": (gva * sel).sum(0), "decoder.bias": ga.sum(0),
                     "log_threshold": th * ((th / EPS) * (gva * band).sum(0) + L0_COEF * band.sum(0) / (B_ * EPS))}
        if sae_type == "baseline_sae":
            bound_abs["decoder.weight"] = dTa.t()
        else:
            # a difference counts with the sum of its operands' magnitudes, like the residual above: 1 - p as 1 + p and
            # 1 - 2 p as 1 + 2 p (a saturated bit has p next to 1 in fp32, and 1 - p carries p's rounding in full)
            s = (p * (1 + p))
            bound_abs["decoder.weight"] = (dTa[:, :, None] * bw.abs() * s + lam * pw * (1 + 2 * p) * s / p.numel()).reshape(H_, D_ * 4)
    # roundings on the longest path: the encoder's dot product and bias (D + 1), the decode over a row's selected entries and
    # the bias (cap + 1), residual, its two scalings, gv's dot product and step (D + 1), the sum over the batch's rows (B), and
    # for the binary decoder the sigmoid, its table of four bit planes and the logit's chain (4 + 6)
    n_terms = (D_ + 1) + (cap + 1) + 3 + (D_ + 1) + B_ + 10
    figures = {}
    for k in want:
        err = (got[k] - want[k]).abs()
        bound = n_terms * 2.0 ** -24 * bound_abs[k]
        figures[k] = (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    print(sae_type, n_terms, figures)
    assert sorted(got) == sorted(want)
    for k in want:
        assert bool(((got[k] - want[k]).abs() <= n_terms * 2.0 ** -24 * bound_abs[k]).all()), (k, figures[k])
        assert float(want[k].abs().max()) > 0


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_three_steps_through_the_trainer(sae_type, rows, tmp_path):
    logs = []
    model = _model(KIND[sae_type])
    if sae_type == "baseline_sae":
        model.normalize_decoder_weights()
    t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path), log_fn=logs.append,
                log_every=1, jumprelu=True, jumprelu_l0_coef=L0_COEF, jumprelu_cap=CAP_, jumprelu_bandwidth=EPS,
                jumprelu_init="calibrate", activity_window=B_, aux_k=4, resample_every=1)
    assert (t.jumprelu.cap, t.jumprelu.bandwidth) == (CAP_, EPS) and t._jumprelu_calibrate
    start = t.jumprelu.log_threshold.detach().clone()
    t.one_epoch(rows)                                         # one batch per call: the chunk is one batch of B_ rows
    assert not t._jumprelu_calibrate
    calibrated_then_stepped = t.jumprelu.log_threshold.detach().clone()
    assert not torch.equal(calibrated_then_stepped, start) and len(set(host(calibrated_then_stepped).tolist())) > 1
    for _ in range(2):
        t.one_epoch(rows)
    assert [len(b) for b in t.trained_batches] == [1, 1, 1]
    assert not torch.equal(t.jumprelu.log_threshold.detach(), calibrated_then_stepped)       # log_threshold moves
    keys = ("jumprelu/l0", "jumprelu/band_entries", "jumprelu/uncertified_rows", "jumprelu/saturated_rows", "jumprelu/theta_min")
    print(sae_type, [[m[k] for k in keys] for m in logs])
    assert len(logs) == 3 and all(k in m for m in logs for k in keys)
    assert all(m["jumprelu/l0"] > 0 and m["jumprelu/band_entries"] > 0 and m["jumprelu/theta_min"] > 0 for m in logs)
    assert "aux_loss" in logs[0] and "dead_features" in logs[0] and "resampled_features" in logs[0]
    sd = t.jumprelu.state_dict()
    other = JumpReLU(model, cap=CAP_, bandwidth=EPS)
    other.load_state_dict(sd)
    same(other.log_threshold, t.jumprelu.log_threshold)
    default = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path))
    assert default.jumprelu is None
