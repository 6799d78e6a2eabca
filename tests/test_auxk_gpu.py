"""AuxK on the GPU (csrc/auxk.hip, quantizedsae_amd.training.auxk): the subset top-k and the loss bit for bit against the numpy
restatements of tests/auxk_util.py -- both sides perform the same IEEE operations in the same order, the library is built
without contracted multiply-adds, so the tolerance is zero -- and the subset top-k also against the composition of existing
ops it replaces; both entry points between guard words; ``forward_aux`` and ``aux_k_loss`` on the two top-k model classes
against an fp64 evaluation on the same selection at the project's training tolerance (1e-5 of the largest gradient entry,
DESIGN.md section 2); and the Trainer's ``aux_k``.

What is tested is the arithmetic and the plumbing.  Whether AuxK keeps units alive on real data is not: no real activations
exist offline."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import auxk_util as U  # noqa: E402
import guard_util as GU  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call  # noqa: E402
from quantizedsae_amd import _lib, ops  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402,F401
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import FeatureActivity, Trainer, aux_k_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, F32, F64 = torch.int32, torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _grad_mode_on():
    with torch.enable_grad():
        yield


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def same(got, want, what=""):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)              # (0-d stays 0-d)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gb, wb = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
    assert np.array_equal(gb, wb), f"{what}: {int((gb != wb).sum())} bytes differ"


# ---- subset top-k -----------------------------------------------------------------------------------------------------
def composed(x, W, bias, units, k):
    """What the kernel replaces, from existing ops: gather the listed rows, pad their number to a multiple of 4 with rows
    that cannot win (zero weights, bias -inf), ops.encode_topk, and the positions mapped back through the list."""
    n, D = units.numel(), W.shape[1]
    pad = (-n) % 4
    Wg, bg, up = W.index_select(0, units.long()), bias.index_select(0, units.long()), units
    if pad:
        Wg = torch.cat([Wg, torch.zeros((pad, D), dtype=F32, device=W.device)])
        bg = torch.cat([bg, torch.full((pad,), float("-inf"), dtype=F32, device=W.device)])
        up = torch.cat([units, torch.full((pad,), -1, dtype=I32, device=W.device)])
    pos, val = ops.encode_topk(x, Wg.contiguous(), bg.contiguous(), k)
    return up[pos.long()], val


def check_topk(x, W, bias, units, k, compose=True):
    want = U.subset_topk(x, W, bias, units, k)
    xd, Wd, bd, ud = dev(x), dev(W), dev(bias), dev(np.asarray(units, dtype=np.int32))
    for mod in (ops, torch_ops):
        idx, val = mod.encode_topk_units(xd, Wd, bd, ud, k)
        same(idx, want[0], "idx")
        same(val, want[1], "val")
    if compose:
        cidx, cval = composed(xd, Wd, bd, ud, k)
        same(idx, host(cidx), "idx against the composition")
        same(val, host(cval), "val against the composition")
    return want


@pytest.mark.parametrize("name", sorted(U.TOPK_SHAPES))
def test_subset_topk_equals_the_restatement_and_the_composition(name):
    x, W, bias, units, k = U.topk_case(name)
    H = W.shape[0]
    assert H - 1 in units and (0 in units or len(units) < 2)
    check_topk(x, W, bias, units, k)


def test_subset_topk_ties_between_duplicated_rows_go_to_the_lower_unit():
    x, W, bias, units, k = U.topk_case("two_panels_k_tail_split_2")
    W, bias = W.copy(), bias.copy()
    twins = [int(units[2]), int(units[40]), int(units[-1])]          # three list entries in two candidate tiles
    W[twins] = 3 * W[twins[0]]
    bias[twins] = 1.0
    idx, val = check_topk(x, W, bias, units, k)
    seen = 0
    for r in range(x.shape[0]):
        at = [int(np.where(idx[r] == t)[0][0]) for t in twins if t in idx[r]]
        if len(at) == 3:
            assert at[1] == at[0] + 1 and at[2] == at[1] + 1 and len(set(val[r, at].tolist())) == 1
            seen += 1
    assert seen > 0


def test_subset_topk_of_a_row_whose_values_are_all_negative():
    x, W, bias, units, k = U.topk_case("k_equals_n")
    idx, val = check_topk(x, W, bias - 50.0, units, k)
    assert (val < 0).all()


def test_a_selected_minus_zero_comes_back_as_plus_zero():
    """The header's statement: val is decoded from the key, which holds -0 as +0.  Every chain here is
    fmaf(-0, 1, ... fmaf(-0, 1, -0)) = -0.0 (D = 32: one whole K slice, no zero padding joins the chain); the subset top-k
    returns +0.0 and, all values tying, the lowest units."""
    B, D, H = 2, 32, 12
    x, W, bias = np.full((B, D), -0.0, np.float32), np.ones((H, D), np.float32), np.full((H,), -0.0, np.float32)
    units = np.array([1, 4, 5, 7, 11], dtype=np.int32)
    assert (U.preacts(x, W, bias, units).view(np.uint32) == 0x80000000).all()
    idx, val = check_topk(x, W, bias, units, 3, compose=False)
    assert idx.tolist() == [[1, 4, 5]] * B and (val.view(np.uint32) == 0).all()


def test_forward_aux_limits_and_the_empty_list():
    model = _model("baseline")
    x = dev(U.gaussian(1, 5, D_))
    units = torch.tensor(DEAD, dtype=I32, device=DEV)
    with pytest.raises(ValueError, match="limit of 64"):
        model.forward_aux(x, units, 65)
    with pytest.raises(ValueError, match="exceeds the 8 listed units"):
        model.forward_aux(x, units, 9)
    with pytest.raises(ValueError, match="limit of 64"):
        aux_k_loss(model, x, x, units, 65)
    with pytest.raises(ValueError, match="1 .. 64"):
        ops.encode_topk_units(x, model.encoder.linear.weight.detach(), None, units, 65)
    with pytest.raises(ValueError, match="listed units"):
        ops.encode_topk_units(x, model.encoder.linear.weight.detach(), None, units, 9)
    empty = torch.zeros((0,), dtype=I32, device=DEV)
    out = model.forward_aux(x, empty, 4)
    assert out.grad_fn is None and tuple(out.shape) == (5, D_) and not out.any()
    zero = aux_k_loss(model, x, x, empty, 4)
    assert zero.grad_fn is None and zero.item() == 0.0
    # k_aux is clamped to the list by aux_k_loss, not by forward_aux
    assert aux_k_loss(model, x, torch.zeros_like(x), units, 64).grad_fn is not None


# ---- the loss ---------------------------------------------------------------------------------------------------------
def _off_alignment(a: np.ndarray) -> torch.Tensor:
    """a contiguous device view of ``a`` that starts 4 bytes past a 16-byte boundary"""
    flat = torch.empty((a.size + 1,), dtype=F32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def loss_inputs(B, D, zero_denominator=False):
    x, recon, aux = U.gaussian(21, B, D), U.gaussian(22, B, D), U.gaussian(23, B, D)
    if zero_denominator:
        x = np.round(x * 8) / np.float32(8)                  # multiples of 1/8: x - 0.25 and the way back are exact
        recon = x - np.float32(0.25)                         # e = 0.25 in every row: it equals its own mean
        assert (x - recon == np.float32(0.25)).all()
    return x, recon, aux


@pytest.mark.parametrize("B,D,off,zero", [(1, 1, False, False), (3, 5, True, False), (257, 36, False, False), (6, 8, False, True)],
                         ids=["1x1", "3x5_off_alignment", "257x36", "zero_denominator"])
def test_loss_equals_the_restatement(B, D, off, zero):
    x, recon, aux = loss_inputs(B, D, zero)
    coef = 1 / 32
    wl, wg, ws = U.auxk_loss(x, recon, aux, coef)
    put = _off_alignment if off else dev
    xd, rd, ad = put(x), put(recon), put(aux)
    sums = torch.empty((2,), dtype=F64, device=DEV)
    loss, grad = ops.auxk_loss(xd, rd, ad, coef, sums=sums)
    same(loss, np.asarray(wl, dtype=np.float32), "loss")
    same(grad, wg, "grad")
    same(sums, ws, "sums")
    if zero or B == 1:
        assert ws[1] == 0.0 and loss.item() == 0.0 and not grad.any()
    loss2, grad2 = torch_ops.auxk_loss(xd, rd, ad, coef)                     # a second run: the same bits
    same(loss2, host(loss), "loss, second run")
    same(grad2, host(grad), "grad, second run")


# ---- both entry points between guard words ----------------------------------------------------------------------------------
def _guard_topk(name):
    def build():
        x, W, bias, units, k = U.topk_case(name)
        B, D = x.shape
        H, n = W.shape[0], len(units)
        widx, wval = U.subset_topk(x, W, bias, units, k)

        def front(t):
            idx, val = ops.encode_topk_units(t["x"], t["W"], t["bias"], t["units"], k)
            return {"idx": idx, "val": val}
        return Call(name, "qsaex_encode_topk_units",
                    [Buf("x", "in", dev(x)), D, Buf("W", "in", dev(W)), D, Buf("bias", "in", dev(bias)), B, D, H,
                     Buf("units", "in", dev(units)), n, k, Buf("idx", "out", shape=(B, k), dtype=I32),
                     Buf("val", "out", shape=(B, k), dtype=F32), WS, WS_BYTES, STREAM],
                    front, sizer=("qsaex_encode_topk_units_workspace_bytes", (B, D, n, k)),
                    expect={"idx": torch.from_numpy(widx), "val": torch.from_numpy(wval)})
    return build


def _guard_loss(B, D, offset_bytes):
    def build():
        x, recon, aux = loss_inputs(B, D)
        coef = 1 / 32
        wl, wg, ws = U.auxk_loss(x, recon, aux, coef)

        def front(t):
            sums = torch.empty((2,), dtype=F64, device=DEV)
            loss, grad = ops.auxk_loss(t["x"], t["recon"], t["aux"], coef, sums=sums)
            return {"loss": loss, "grad": grad, "sums": sums}
        return Call(f"{B}x{D}", "qsaex_auxk_loss",
                    [Buf("x", "in", dev(x), offset_bytes=offset_bytes), Buf("recon", "in", dev(recon), offset_bytes=offset_bytes),
                     Buf("aux", "in", dev(aux), offset_bytes=offset_bytes), B, D, coef, Buf("loss", "out", shape=(), dtype=F32),
                     Buf("grad", "out", shape=(B, D), dtype=F32, offset_bytes=offset_bytes), Buf("sums", "out", shape=(2,), dtype=F64),
                     WS, WS_BYTES, STREAM],
                    front, sizer=("qsaex_auxk_loss_workspace_bytes", (B, D)),
                    expect={"loss": torch.from_numpy(np.asarray(wl, dtype=np.float32)), "grad": torch.from_numpy(wg),
                            "sums": torch.from_numpy(ws)})
    return build


#: label -> (entry point, builder of its guard_util.Call); tests/test_auxk_host.py reads the entry points for its ledger.
#: Building a case touches the GPU; importing this table does not.
GUARD_CASES = {
    "topk_minimal": ("qsaex_encode_topk_units", _guard_topk("minimal")),
    "topk_tile_tails": ("qsaex_encode_topk_units", _guard_topk("two_panels_k_tail_split_2")),
    "loss_minimal": ("qsaex_auxk_loss", _guard_loss(1, 1, 0)),
    "loss_tails_off_alignment": ("qsaex_auxk_loss", _guard_loss(257, 36, 4)),
}


@pytest.mark.parametrize("label", sorted(GUARD_CASES))
def test_entry_point_between_guard_words(label):
    entry, build = GUARD_CASES[label]
    call = build()
    assert call.entry == entry
    GU.run_call(call, _lib.load(), DEV)


# ---- forward_aux and aux_k_loss on the models ------------------------------------------------------------------------------
D_, H_, K_, B_ = 16, 64, 4, 32
DEAD = [3, 9, 17, 20, 33, 41, 50, 63]                        # made dead by an encoder bias of -100
COEF = 1 / 32


def _model(kind: str, seed: int = 5):
    torch.manual_seed(seed)
    if kind == "baseline":
        model = BaselineSparseAutoencoder(D_, H_)
        model.topk = K_
    else:
        model = BinarySAE(D_, H_, n_bits=4)
        model.k = K_ / H_
        assert model.top_k == K_
    with torch.no_grad():
        model.encoder.linear.bias[DEAD] = -100.0
    return model.to(DEV)


def _decoder(model):
    return model.decoder.weight


def _atoms(model, g):
    """the rows of a decoder gradient, one per unit"""
    return g.t() if isinstance(model, BaselineSparseAutoencoder) else g


def _reference64(model, x, idx, recon=None, cotangent=None):
    """fp64 torch on the selection ``idx``: the auxiliary reconstruction, and the gradients of <aux, cotangent> or, with
    ``recon``, of the AuxK loss -> (aux, {parameter name: gradient})"""
    lin = model.encoder.linear
    W = lin.weight.detach().cpu().double().requires_grad_()
    b = lin.bias.detach().cpu().double().requires_grad_()
    dec = _decoder(model).detach().cpu().double().requires_grad_()
    x64, idx = x.detach().cpu().double(), idx.cpu().long()
    if isinstance(model, BaselineSparseAutoencoder):
        table, step = dec.t(), 1.0
    else:
        n = model.decoder.n_bits
        bw = 2.0 ** torch.arange(n, dtype=F64)
        bw[-1] = -bw[-1]
        table, step = (torch.sigmoid(dec).view(H_, D_, n) * bw).sum(-1), model.decoder.quantization_step
    pre = (x64[:, None, :] * W[idx]).sum(-1) + b[idx]
    aux = step * (pre[:, :, None] * table[idx]).sum(1)
    if recon is None:
        out = (aux * cotangent.detach().cpu().double()).sum()
    else:
        e = (x.detach() - recon.detach()).cpu().double()                     # fl32(x - recon), widened
        out = COEF * ((aux - e) ** 2).sum() / ((e - e.mean(0)) ** 2).sum()
    out.backward()
    return aux.detach(), out.detach(), {"encoder.weight": W.grad, "encoder.bias": b.grad, "decoder.weight": dec.grad}


def _param_grads(model):
    lin = model.encoder.linear
    return {"encoder.weight": lin.weight.grad, "encoder.bias": lin.bias.grad, "decoder.weight": _decoder(model).grad,
            "decoder.bias": model.decoder.bias.grad}


def _close(got, want, what):
    scale = want.abs().max().item()
    assert scale > 0, what
    err = (got.detach().cpu().double() - want).abs().max().item()
    assert err <= 1e-5 * scale, f"{what}: {err:.3e} against 1e-5 x {scale:.3e}"


@pytest.mark.parametrize("kind", ["baseline", "binary"])
def test_forward_aux_and_its_gradient_against_fp64(kind):
    model = _model(kind)
    lin = model.encoder.linear
    x = dev(U.gaussian(31, B_, D_)).requires_grad_()
    units = torch.tensor(DEAD, dtype=I32, device=DEV)
    cot = dev(U.gaussian(32, B_, D_))
    idx, _ = ops.encode_topk_units(x.detach(), lin.weight.detach(), lin.bias.detach(), units, K_)
    assert set(idx.unique().tolist()) <= set(DEAD)
    aux = model.forward_aux(x, units, K_)
    assert aux.grad_fn is not None and tuple(aux.shape) == (B_, D_) and aux.dtype == F32
    torch.autograd.backward([aux], [cot])
    aux64, _, want = _reference64(model, x, idx, cotangent=cot)
    _close(aux, aux64, "aux")
    got = _param_grads(model)
    for name in want:
        _close(got[name], want[name], name)
    assert got["decoder.bias"] is None and x.grad is None                    # no decoder bias term, nothing for x


@pytest.mark.parametrize("kind", ["baseline", "binary"])
def test_aux_k_loss_and_its_gradient_against_fp64(kind):
    model = _model(kind)
    lin = model.encoder.linear
    x = dev(U.gaussian(33, B_, D_))
    units = torch.tensor(DEAD, dtype=I32, device=DEV)
    recon = model.forward_train(x)[1]
    idx, _ = ops.encode_topk_units(x, lin.weight.detach(), lin.bias.detach(), units, K_)
    loss = aux_k_loss(model, x, recon, units, K_, COEF)
    assert loss.grad_fn is not None and loss.dim() == 0 and loss.dtype == F32
    loss.backward()
    _, loss64, want = _reference64(model, x, idx, recon=recon)
    assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item())
    got = _param_grads(model)
    for name in want:
        _close(got[name], want[name], name)
    assert got["decoder.bias"] is None                                       # recon is detached inside: nothing reaches the main path


def _step_grads(model, x, units):
    """the gradients of mse(recon, x) (+ the AuxK loss over ``units``) -> name -> tensor"""
    model.zero_grad(set_to_none=True)
    recon = model.forward_train(x)[1]
    total = ((recon - x) ** 2).mean()
    if units is not None:
        total = total + aux_k_loss(model, x, recon, units, K_, COEF)
    total.backward()
    return {k: v.detach().clone() for k, v in _param_grads(model).items()}


@pytest.mark.parametrize("kind", ["baseline", "binary"])
def test_dead_units_get_a_gradient_from_the_auxiliary_loss_and_only_they(kind):
    model = _model(kind)
    lin = model.encoder.linear
    model.activity = FeatureActivity.for_model(model)
    x = dev(U.gaussian(34, B_, D_))
    units = torch.tensor(DEAD, dtype=I32, device=DEV)
    alive = torch.tensor([h for h in range(H_) if h not in DEAD], device=DEV)
    dead = units.long()
    idx, _ = ops.encode_topk_units(x, lin.weight.detach(), lin.bias.detach(), units, K_)
    chosen = idx.unique().long()
    assert 0 < chosen.numel() <= len(DEAD)

    plain = _step_grads(model, x, None)
    before = (model.activity.fired.clone(), model.activity.last.clone(), model.activity.rows_seen)
    assert before[2] == B_ and not model.activity.fired[dead].any()          # the main top-k never selects them
    both = _step_grads(model, x, units)
    again = _step_grads(model, x, units)
    # the tracker saw two more batches from forward_train and nothing from forward_aux: the dead stay dead for it
    assert model.activity.rows_seen == 3 * B_ and not model.activity.fired[dead].any()
    assert torch.equal(model.activity.fired, 3 * before[0])

    for name in ("encoder.weight", "encoder.bias", "decoder.weight"):
        atoms = (lambda g: _atoms(model, g)) if name == "decoder.weight" else (lambda g: g)
        assert not atoms(plain[name])[dead].any(), name                      # without the term: exactly zero
        rows = atoms(both[name])[chosen]
        assert bool((rows.reshape(chosen.numel(), -1) != 0).any(dim=1).all()), name   # with it: every selected dead unit moves
        assert bool((atoms(both[name])[alive] == atoms(plain[name])[alive]).all()), name
    assert bool((both["decoder.bias"] == plain["decoder.bias"]).all())
    for name in both:
        same(again[name], host(both[name]), f"{name}, second run")


def test_forward_aux_leaves_the_tracker_alone_and_reuses_the_steps_table(monkeypatch):
    from quantizedsae_amd.sae import binary as binary_module
    model = _model("binary")
    model.activity = FeatureActivity.for_model(model)
    x = dev(U.gaussian(35, B_, D_))
    units = torch.tensor(DEAD, dtype=I32, device=DEV)
    calls = []
    real = binary_module.ops.binary_soft_table
    monkeypatch.setattr(binary_module.ops, "binary_soft_table", lambda *a, **k: calls.append(1) or real(*a, **k))
    model.forward_train(x)
    state = (model.activity.fired.clone(), model.activity.last.clone(), model.activity.rows_seen)
    a = model.forward_aux(x, units, K_)
    assert not calls                                                         # the table forward_train built
    assert torch.equal(model.activity.fired, state[0]) and torch.equal(model.activity.last, state[1])
    assert model.activity.rows_seen == state[2]
    with torch.no_grad():
        model.decoder.weight.mul_(1.5)                                       # moves the logits' version counter
    b = model.forward_aux(x, units, K_)
    assert len(calls) == 1 and not torch.equal(a, b)                         # on its own: one fresh table
    model.forward_aux(x, units, K_)
    assert len(calls) == 1


# ---- the Trainer ------------------------------------------------------------------------------------------------------
CONFIG = {"input_dim": D_, "n_bits": 4, "hidden_dim": H_, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": K_,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": B_}
KIND = {"baseline_sae": "baseline", "b_sae": "binary"}


def _run_trainer(sae_type, tmp_path, **options):
    logs, dead_list_calls = [], []
    t = Trainer(CONFIG, sae_type, False, True, model=_model(KIND[sae_type]), dataset_dir=str(tmp_path), save_dir=str(tmp_path),
                log_fn=logs.append, log_every=1, **options)
    if t.activity is not None:
        summary = t.activity.summary

        def spying_summary(window, **kw):
            if kw.get("dead_list"):
                dead_list_calls.append(kw)
            return summary(window, **kw)
        t.activity.summary = spying_summary
    torch.manual_seed(9)
    t.one_epoch(dev(U.gaussian(36, 3 * B_, D_)))
    assert len(t.trained_batches[-1]) == 3
    return t, logs, dead_list_calls


def _state(t):
    return {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()}


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_trainer_with_aux_k(sae_type, tmp_path):
    first = {k: v.detach().cpu().clone() for k, v in _model(KIND[sae_type]).state_dict().items()}
    plain, logs0, _ = _run_trainer(sae_type, tmp_path, activity_window=B_)
    none, logs1, _ = _run_trainer(sae_type, tmp_path, activity_window=B_, aux_k=None)
    t, logs, refreshes = _run_trainer(sae_type, tmp_path, activity_window=B_, aux_k=K_, aux_refresh=2)
    # aux_k=None: the weights of a Trainer built without the argument, bit for bit, and no aux key in the metrics
    for k, v in _state(plain).items():
        same(_state(none)[k], v.numpy(), k)
    assert not [k for m in logs0 + logs1 for k in m if k.startswith("aux_")]
    # three steps, a refresh every two: the dead list is read at the first and the third step and at no other time
    assert len(refreshes) == 2 and all(kw == {"dead_list": True, "advance": False} for kw in refreshes)
    assert len(logs) == 3
    for m in logs:
        assert m["aux_units"] >= len(DEAD) and np.isfinite(m["aux_loss"]) and m["aux_loss"] > 0
    assert logs[0]["aux_units"] == logs[1]["aux_units"]                      # the second step ran over the first step's list
    # without the term no gradient ever reaches the units with the bias of -100; with it the run trains other weights
    assert torch.equal(first["encoder.0.weight"][DEAD], _state(plain)["encoder.0.weight"][DEAD])
    assert not torch.equal(_state(plain)["encoder.0.weight"], _state(t)["encoder.0.weight"])


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_trainer_with_aux_k_and_resampling(sae_type, tmp_path):
    t, logs, refreshes = _run_trainer(sae_type, tmp_path, activity_window=B_, aux_k=K_, resample_every=2, resample_seed=3)
    assert len(logs) == 3 and all("aux_loss" in m and "aux_units" in m for m in logs)
    resampling = [b % 2 == 0 for b in t.trained_batches[-1]]
    assert 0 < sum(resampling) < 3 and [("resampled_features" in m) for m in logs] == resampling
    # aux_refresh defaults to log_every = 1: one list per step for the loss, and one per resampling step
    assert len(refreshes) == 3 + sum(resampling)
    assert all(torch.isfinite(v).all() for v in _state(t).values() if v.is_floating_point())
