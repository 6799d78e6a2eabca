"""The dense JumpReLU encoder on the GPU (csrc/jump_dense.hip, include/qsae_jump_dense.h): the entry point between guard words,
twice on one poisoned workspace of exactly the sizer's bytes, bit for bit against the numpy restatement of
tests/jump_dense_util.py; both front ends and the dispatcher op; and the two top-k model classes: the dense path against the
capped one on a batch the capped path certifies, against the restatement on a batch it does not, and three steps of the Trainer."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard_util as GU  # noqa: E402
import jump_dense_util as U  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import FeatureActivity, JumpReLU, Trainer, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64, F32 = torch.int32, torch.int64, torch.float32
NAMES = U.NAMES


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


# ---- the entry point between guard words ----------------------------------------------------------------------------------
#: (B, D, H, K, band lists, bias): a thinned cross product in which every B of {1, 3, 70, 130} (the panel's tail at 128), every
#: H of {8, 300, 1100} (one tile; three splits with a tile tail; more tiles than splits, so uneven splits), every D of {4, 36,
#: 512} (below BK; a K tail; the workload's) and every K of {1, 5, 64, 65, 256} appears, with and without the band lists and the
#: bias; each shape runs with every kind of thresholds.
SHAPES = ((1, 4, 8, 1, True, True), (3, 36, 300, 5, True, False), (70, 36, 300, 5, False, True), (70, 512, 1100, 64, True, True),
          (130, 36, 300, 65, True, True), (130, 4, 1100, 256, True, False), (3, 512, 300, 256, False, False))
#: thresholds at the 0.2 quantile of the pre-activations where K = 5 and H = 300: about 240 of a row's 300 units fire, more than
#: K and more than a (split, row) region of the workspace holds, so these rows go through the kernel that recomputes a row
LOW_QUANTILE = 0.2


def _quantile(H, K):
    return LOW_QUANTILE if (H, K) == (300, 5) else 0.9


def _expected(want, band):
    out = {n: torch.from_numpy(np.ascontiguousarray(w)) for n, w in zip(NAMES, want) if n != "l0"}
    out["l0"] = torch.tensor([want[5]], dtype=F32)
    if not band:
        del out["idx_band"], out["counts_band"]
    return out


def _guard_encode(kind, B, D, H, K, band, with_bias, off=0):
    """``off``: every 4-byte operand starts that many bytes past a 16-byte boundary (x and W stay 16-byte aligned, the report
    8-byte aligned, as the header asks)"""
    def build():
        x, W, bias, theta, eps = U.case(kind, B, D, H, seed=3, with_bias=with_bias, quantile=_quantile(H, K))
        want = U.encode_jump(x, W, bias, theta, K, eps)
        if (H, K) == (300, 5) and kind in ("all", "mixed"):                  # the low thresholds ("special" has its own)
            assert int(want[6][2]) > B / 2, (kind, want[6].tolist())         # most rows hold more than K firing units

        def front(t):
            got = dict(zip(NAMES, ops.encode_jump(t["x"], t["W"], t.get("bias"), t["theta"], K, float(eps), want_band=band)))
            return {n: v for n, v in got.items() if v is not None}
        return Call(f"{kind}_{B}x{D}_H{H}_K{K}_band{int(band)}_bias{int(with_bias)}_off{off}", "qsaed_encode_jump",
                    [Buf("x", "in", dev(x)), D, Buf("W", "in", dev(W)), D,
                     Buf("bias", "in", dev(bias), offset_bytes=off) if with_bias else None,
                     Buf("theta", "in", dev(theta), offset_bytes=off), B, D, H, K, float(eps), float(U.half_eps(eps)),
                     Buf("idx_sel", "out", shape=(B, K), dtype=I32, offset_bytes=off),
                     Buf("val_sel", "out", shape=(B, K), dtype=F32, offset_bytes=off),
                     Buf("counts", "out", shape=(B,), dtype=I32, offset_bytes=off),
                     Buf("idx_band", "out", shape=(B, K), dtype=I32, offset_bytes=off) if band else None,
                     Buf("counts_band", "out", shape=(B,), dtype=I32, offset_bytes=off) if band else None,
                     Buf("l0", "out", shape=(1,), dtype=F32, offset_bytes=off), Buf("report", "out", shape=(6,), dtype=I64),
                     WS, WS_BYTES, STREAM], front, sizer=("qsaed_encode_jump_workspace_bytes", (B, D, H, K)),
                    expect=_expected(want, band))
    return build


def _guard_cases():
    cases = {}
    for kind in U.KINDS:
        for B, D, H, K, band, with_bias in SHAPES:
            cases[f"{kind}_{B}x{D}_H{H}_K{K}"] = ("qsaed_encode_jump", _guard_encode(kind, B, D, H, K, band, with_bias))
    cases["special_70x36_H300_K64_off4"] = ("qsaed_encode_jump", _guard_encode("special", 70, 36, 300, 64, True, True, off=4))
    return cases


#: label -> (entry point, builder of its guard_util.Call); tests/test_jump_dense_host.py reads the entry points for its ledger.
#: Building a case touches the GPU; importing this table does not.
GUARD_CASES = _guard_cases()


def test_the_shapes_cover_every_value():
    for i, values in enumerate(((1, 3, 70, 130), (4, 36, 512), (8, 300, 1100), (1, 5, 64, 65, 256), (True, False), (True, False))):
        assert {s[i] for s in SHAPES} == set(values)
    assert all(K <= H for _, _, H, K, _, _ in SHAPES)


@pytest.mark.parametrize("kind", U.KINDS + ("off4",))
def test_entry_point_between_guard_words(kind):
    labels = [label for label in sorted(GUARD_CASES) if (label.endswith("_off4") if kind == "off4" else
                                                          label.startswith(kind + "_") and not label.endswith("_off4"))]
    assert len(labels) == (1 if kind == "off4" else len(SHAPES))
    for label in labels:
        entry, build = GUARD_CASES[label]
        call = build()
        assert call.entry == entry
        GU.run_call(call, _lib.load(), DEV)


def test_both_front_ends_and_the_dispatcher_op():
    x, W, bias, theta, eps = U.case("mixed", 70, 36, 300, seed=5)
    want = U.encode_jump(x, W, bias, theta, 64, eps)
    for mod in (ops, torch_ops):
        got = mod.encode_jump(dev(x), dev(W), dev(bias), dev(theta), 64, float(eps))
        for g, w, name in zip(got, want, NAMES):
            same(g, np.array([w], np.float32) if name == "l0" else w, name)
        got = mod.encode_jump(dev(x), dev(W), None, dev(theta), 64, float(eps), want_band=False)
        assert got[3] is None and got[4] is None
        same(got[2], U.encode_jump(x, W, None, theta, 64, eps)[2], "counts without a bias")
    empty = ops.encode_jump(dev(x[:0]), dev(W), dev(bias), dev(theta), 64, float(eps))
    assert tuple(empty[0].shape) == (0, 64) and host(empty[6]).tolist() == [0] * 6
    assert ops.JUMP_DENSE_MAX_K == torch_ops.JUMP_DENSE_MAX_K == 256
    with pytest.raises(ValueError, match="bandwidth"):
        ops.encode_jump(dev(x), dev(W), dev(bias), dev(theta), 64, 0.0)
    with pytest.raises(ValueError, match="K = 301"):
        ops.encode_jump(dev(x), dev(W), dev(bias), dev(theta), 301, 0.25)
    with pytest.raises(ValueError, match="theta"):
        ops.encode_jump(dev(x), dev(W), dev(bias), dev(theta[:8]), 8, 0.25)
    Q = torch.ops.qsae
    torch.library.opcheck(Q.encode_jump.default, (dev(x), dev(W), dev(bias), dev(theta), 64, float(eps), True))
    torch.library.opcheck(Q.encode_jump.default, (dev(x), dev(W), None, dev(theta), 5, float(eps), False))


# ---- the two top-k model classes ----------------------------------------------------------------------------------------
D_, H_, K_, B_ = 32, 300, 8, 70
CAP = 64
EPS = 0.05
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


@pytest.fixture(scope="module")
def rows_np():
    return S.activations(91, B_, D_)


@pytest.fixture(scope="module")
def rows(rows_np):
    return dev(rows_np)


def _preact(kind, rows_np):
    st = _state(kind)
    return U.preact(rows_np, st["encoder.0.weight"], st["encoder.0.bias"])


def _certified_thresholds(z, cap=CAP, margin=EPS):
    """One threshold per unit, every one above every row's cap-th largest pre-activation by ``margin``, at least the bandwidth
    (so the capped path certifies every row: the cap-th value lies below theta_min - eps / 2), spread upwards per unit.  On
    these shapes the smallest lies near the 0.9 quantile of the pre-activations; at the bandwidth between 5 and 40 units of a
    row fire."""
    base = np.sort(z, axis=1)[:, -cap].max() + margin
    jitter = np.abs(np.random.default_rng(5).standard_normal(z.shape[1]))
    return (base * (1 + 0.5 * jitter)).astype(np.float32)


def _uncertified_thresholds(H):
    """Thresholds spread over a factor of about four around 1.8: at K = 5 a row's five largest pre-activations include units
    that do not fire while smaller ones do, which a top-5 list cannot show"""
    return (np.float32(1.8) * np.exp(0.7 * np.random.default_rng(5).standard_normal(H))).astype(np.float32)


def _controller(model, theta, cap=CAP, eps=EPS):
    jr = JumpReLU(model, cap=cap, bandwidth=eps)
    with torch.no_grad():
        jr.log_threshold.copy_(dev(theta).log())
    return jr


def _grads(model, jr):
    out = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    out["log_threshold"] = jr.log_threshold.grad.detach().clone()
    return out


def _prefix_equal(a, b, counts, what):
    a, b = host(a), host(b)
    for r, c in enumerate(host(counts).tolist()):
        assert np.array_equal(a[r, :c].view(np.uint32), b[r, :c].view(np.uint32)), (what, r)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_dense_equals_capped_where_the_capped_path_certifies_every_row(sae_type, rows, rows_np):
    kind = KIND[sae_type]
    theta = _certified_thresholds(_preact(kind, rows_np))
    outs, grads, reports, lists = {}, {}, {}, {}
    for path in ("capped", "dense"):
        model = _model(kind)
        model.activity = FeatureActivity.for_model(model)
        jr = _controller(model, theta)
        fwd = model.forward_jumprelu_dense if path == "dense" else model.forward_jumprelu
        lists[path] = fwd(rows, jr)
        reports[path + "_eval"] = host(jr.report).tolist()
        x = rows.clone().requires_grad_()
        train = model.forward_train_jumprelu_dense if path == "dense" else model.forward_train_jumprelu
        out = train(x, jr)
        reports[path] = host(jr.report).tolist()
        assert len(out) == (4 if sae_type == "b_sae" else 3) and all(o.grad_fn is not None for o in out) and out[-1].dim() == 0
        trainer_loss(sae_type, out[:-1], rows, CONFIG, extra=[(out[-1], torch.full((), L0_COEF, dtype=F32, device=DEV))])
        outs[path] = (out[0].detach(), out[1].detach(), out[-1].detach(), jr.counts.clone(), host(model.activity.fired).copy())
        grads[path] = dict(_grads(model, jr), x=x.grad.detach().clone())
        assert jr.report_names is (JumpReLU.REPORT_NAMES_DENSE if path == "dense" else JumpReLU.REPORT_NAMES)
    # the precondition, from the capped path's own report: no uncertified row, no saturated row, something selected and a band
    for rep in (reports["capped"], reports["capped_eval"]):
        assert rep[4] == 0 and rep[2] == 0 and rep[0] > B_ and rep[1] > 50, rep
    assert reports["dense"][:2] == reports["capped"][:2] and reports["dense"][2] == 0 and reports["dense"][5] == reports["dense"][0]
    assert reports["dense"][3] == reports["capped"][3]
    c_idx, c_val, c_counts, c_recon = lists["capped"]
    d_idx, d_val, d_counts, d_recon = lists["dense"]
    same(d_counts, c_counts, "counts"), same(d_recon, c_recon, "the evaluation's reconstruction")
    _prefix_equal(d_idx, c_idx, c_counts, "idx_sel"), _prefix_equal(d_val, c_val, c_counts, "val_sel")
    hd, hc = host(d_idx), host(d_counts)
    assert all((hd[r, c:] == -1).all() and not host(d_val)[r, c:].view(np.uint32).any() for r, c in enumerate(hc.tolist()))
    for i, name in enumerate(("latent", "reconstruction", "l0", "counts")):
        same(outs["dense"][i], outs["capped"][i], name)
    assert np.array_equal(outs["dense"][4], outs["capped"][4]) and outs["dense"][4].sum() == reports["dense"][0]
    assert sorted(grads["dense"]) == sorted(grads["capped"])
    for k in grads["capped"]:
        same(grads["dense"][k], grads["capped"][k], k + ".grad")
        assert float(grads["capped"][k].abs().max()) > 0, k
    # the band lists, which the models do not return: the two selections at the level of the ops
    model = _model(kind)
    lin = model.encoder.linear
    th = dev(theta).log().exp()
    idx, val = model._select_cap(rows, CAP, "test")
    c = ops.jump_select(idx, val, th, EPS)
    d = ops.encode_jump(rows, lin.weight.detach(), lin.bias.detach(), th, CAP, EPS)
    same(d[4], c[4], "counts_band"), _prefix_equal(d[3], c[3], c[4], "idx_band"), same(d[5], c[5], "l0")


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_dense_equals_the_restatement_where_the_capped_path_is_uncertified(sae_type, rows, rows_np):
    kind, K, eps = KIND[sae_type], 5, 0.25
    model = _model(kind)
    jr = _controller(model, _uncertified_thresholds(H_), cap=K, eps=eps)
    theta = host(jr.thresholds())
    z = _preact(kind, rows_np)
    same(model.encoder(rows.clone()), z, "the model's pre-activations are the restatement's")
    want = U.encode_jump_from_z(z, theta, K, eps)
    idx_sel, val_sel, counts, recon = model.forward_jumprelu_dense(rows, jr)
    same(idx_sel, want[0], "idx_sel"), same(val_sel, want[1], "val_sel"), same(counts, want[2], "counts"), same(jr.report, want[6], "report")
    s = jr.summary()
    assert s["truncated_rows"] == int(want[6][2]) and s["firing"] == int(want[6][5]) and s["l0"] == int(want[6][5]) / B_
    # the dense mask: every firing unit of a row that is not truncated, the K largest of one that is
    sel, _ = U.predicates(z, theta, eps)
    n_sel = sel.sum(axis=1)
    whole = n_sel <= K
    assert 10 < int(whole.sum()) < B_ - 10 and int((~whole).sum()) == int(want[6][2])
    latent = host(ops.densify(idx_sel, val_sel, H_))
    same(latent[whole], U.dense_latent(z, theta)[whole], "where(z > theta, z, 0) on the rows that are not truncated")
    got_mask = latent != 0
    assert np.array_equal(got_mask[whole], sel[whole]) and (got_mask[~whole].sum(axis=1) == K).all() and not (got_mask & ~sel).any()
    # the capped path at the same K is not JumpReLU here: it reports every row uncertified and differs from the dense mask
    c_idx, c_val, c_counts, _ = model.forward_jumprelu(rows, jr)
    assert int(jr.report[4]) == B_
    capped = host(ops.densify(c_idx, c_val, H_))
    differing = int((capped != latent).any(axis=1).sum())
    print(sae_type, "rows on which the capped path differs from JumpReLU:", differing, "of", B_)
    assert differing >= 1
    # training on this batch: l0 counts every firing unit, also beyond the K-th of a truncated row
    out = model.forward_train_jumprelu_dense(rows, jr)
    same(out[-1], np.float32(want[5]), "l0"), same(out[0], latent, "latent")
    assert int(want[6][5]) == int(n_sel.sum()) > int(want[2].sum()) and want[5] == np.float32(int(n_sel.sum()) / B_)
    with pytest.raises(ValueError, match="expected \\[batch"):
        model.forward_jumprelu_dense(rows[:, :8], jr)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_three_steps_of_the_dense_trainer_equal_the_capped_trainer(sae_type, rows, rows_np, tmp_path):
    # three bandwidths above the lists' last values: three Adam steps move weights and thresholds, the certificate must hold
    theta = _certified_thresholds(_preact(KIND[sae_type], rows_np), margin=3 * EPS)
    final, logs = {}, {}
    for dense in (False, True):
        logs[dense] = []
        model = _model(KIND[sae_type])
        if sae_type == "baseline_sae":
            model.normalize_decoder_weights()
        t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path),
                    log_fn=logs[dense].append, log_every=1, jumprelu=True, jumprelu_l0_coef=L0_COEF, jumprelu_cap=CAP,
                    jumprelu_bandwidth=EPS, jumprelu_dense=dense)
        assert t.jumprelu_dense is dense
        with torch.no_grad():
            t.jumprelu.log_threshold.copy_(dev(theta).log())
        torch.manual_seed(29)                                 # the loader shuffles the chunk's rows with the default generator:
        for _ in range(3):                                    # both trainers see the same orders (sums run over rows in order)
            t.one_epoch(rows)                                 # one batch per call: the chunk is one batch of B_ rows
        final[dense] = dict({k: v.detach().clone() for k, v in model.state_dict().items()},
                            log_threshold=t.jumprelu.log_threshold.detach().clone())
    assert len(logs[False]) == len(logs[True]) == 3
    # the precondition at every step, from the capped trainer's own log
    assert all(m["jumprelu/uncertified_rows"] == 0 and m["jumprelu/saturated_rows"] == 0 and m["jumprelu/band_entries"] > 0
               for m in logs[False]), logs[False]
    assert all("jumprelu/truncated_rows" in m and "jumprelu/uncertified_rows" not in m for m in logs[True])
    assert all(m["jumprelu/truncated_rows"] == 0 for m in logs[True])
    for a, b in zip(logs[False], logs[True]):
        assert a["jumprelu/l0"] == b["jumprelu/l0"] > 0 and a["jumprelu/band_entries"] == b["jumprelu/band_entries"]
    assert sorted(final[False]) == sorted(final[True])
    for k in final[False]:
        same(final[True][k], final[False][k], k)
    assert not torch.equal(final[True]["log_threshold"], dev(theta).log())                   # the thresholds moved
