"""The dense BatchTopK encoder on the GPU (csrc/batch_dense.hip, include/qsae_batch_dense.h): the entry point between guard
words, twice on one poisoned workspace of exactly the sizer's bytes, bit for bit against the numpy restatement of
tests/batch_dense_util.py; one batch under five floors (the result must not depend on the floor; the second attempt must run
exactly where the floor is too high); both front ends and the dispatcher op; the two top-k model classes, plain and nested,
against the capped path (lists within the prefix, counts, reconstruction, latent, every .grad); and three steps of the Trainer."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import batch_dense_util as U  # noqa: E402
import guard_util as GU  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import BatchTopK, Trainer, nested_loss, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64, F32 = torch.int32, torch.int64, torch.float32
INF, NAN = float("inf"), float("nan")


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
#: (B, D, H, K, bias): a thinned cross product in which every B of {1, 3, 70, 130} (the panel's tail at 128), every H of {8,
#: 300, 1100} (one tile; three splits with a tile tail; more tiles than splits), every D of {4, 36, 512} (below BK; a K tail;
#: the workload's) and every K of {1, 5, 64, 65, 256} appears, with and without the bias; each shape runs under every floor.
SHAPES = ((1, 4, 8, 1, True), (3, 36, 300, 5, False), (70, 36, 300, 5, True), (70, 512, 1100, 64, True), (130, 36, 300, 65, True),
          (130, 4, 1100, 256, False), (3, 512, 300, 256, False))
#: the floor of a case, from the batch's smallest selected value m: "certified" is what a training step leaves (0.9 m, on the
#: device, with the threshold state), "zero" admits about half of a row's units (at H = 1100 more than a row's 512 records, at
#: H = 300 more than a region's 64: the resolve kernel), "too_high" (2 m) fails the certificate so that the second attempt runs,
#: "special" is a batch with a row of NaN and a row of zeros under a floor of -inf
KINDS = ("certified", "zero", "too_high", "special")
STATE = (0.5, 3, 0.25)                                        # theta, batches, lr of the cases that carry the threshold state


def k_of(K):
    """the k of n_select = B k at the cap K: a quarter of it, as the front end's default cap = 4 k"""
    return max(1, K // 4)


def case(kind, B, D, H, K, with_bias, seed=3):
    """-> (x, W, bias, n_select, floor, on the device?, with state?)"""
    x, W, bias = U.operands(B, D, H, seed + 31 * B + 7 * D + H, with_bias)
    n_select = B * k_of(K)
    if kind == "special":
        x = x.copy()
        if B >= 2:
            x[B - 1, :] = 0.0                                  # z = bias (or +0)
        if B >= 3:
            x[1, D // 2] = np.nan                              # the whole row is NaN: never a candidate
        if bias is not None:
            bias = bias.copy()
            bias[H - 1] = -0.0
        return x, W, bias, n_select, -INF, False, True
    m = U.smallest_selected(U.preact(x, W, bias), K, n_select)
    if kind == "certified":
        return x, W, bias, n_select, float(np.float32(0.9) * m), True, True
    if kind == "zero":
        return x, W, bias, n_select, 0.0, False, False
    assert kind == "too_high"
    return x, W, bias, n_select, float(np.float32(2.0) * m), True, False


def _guard_encode(kind, B, D, H, K, with_bias, off=0):
    """``off``: every 4-byte operand starts that many bytes past a 16-byte boundary (x and W stay 16-byte aligned, the report
    and batches 8-byte aligned, as the header asks)"""
    def build():
        x, W, bias, n_select, floor, on_device, with_state = case(kind, B, D, H, K, with_bias)
        theta, batches, lr = STATE if with_state else (None, 0, 0.0)
        z = U.preact(x, W, bias)
        want = U.encode_batch_topk_from_z(z, K, n_select, floor, floor_ratio=0.75, floor_dev=on_device, theta=theta, batches=batches,
                                          lr=lr)
        report = want[3]
        if kind == "zero" and H == 1100:                       # the path this case exists for
            assert U.rows_resolved(z, floor).mean() > 0.5
        if kind == "too_high":
            assert report[5] == 1, report.tolist()
        if kind == "certified":
            assert report[5] == 0 and report[0] == n_select, report.tolist()
        expect = {"idx_sel": torch.from_numpy(want[0]), "val_sel": torch.from_numpy(want[1]), "counts": torch.from_numpy(want[2]),
                  "report": torch.from_numpy(report)}
        if with_state:
            expect["theta"] = torch.tensor([want[4][0]], dtype=F32)
            expect["batches"] = torch.tensor([want[4][1]], dtype=I64)
        if on_device:
            expect["floor"] = torch.tensor([want[4][2]], dtype=F32)

        def front(t):
            state = (t["theta"], t["batches"], lr) if with_state else None
            got = dict(zip(U.NAMES, ops.encode_batch_topk(t["x"], t["W"], t.get("bias"), n_select, K, t["floor"] if on_device else floor,
                                                          0.75, state)))
            for name in ("theta", "batches", "floor"):
                if name in t:
                    got[name] = t[name]
            return got
        return Call(f"{kind}_{B}x{D}_H{H}_K{K}_bias{int(with_bias)}_off{off}", "qsaebd_encode_batch_topk",
                    [Buf("x", "in", dev(x)), D, Buf("W", "in", dev(W)), D,
                     Buf("bias", "in", dev(bias), offset_bytes=off) if with_bias else None, B, D, H, K, n_select,
                     Buf("floor", "inout", dev(np.array([floor], np.float32)), offset_bytes=off) if on_device else None,
                     0.0 if on_device else floor, 0.75,
                     Buf("idx_sel", "out", shape=(B, K), dtype=I32, offset_bytes=off),
                     Buf("val_sel", "out", shape=(B, K), dtype=F32, offset_bytes=off),
                     Buf("counts", "out", shape=(B,), dtype=I32, offset_bytes=off), Buf("report", "out", shape=(8,), dtype=I64),
                     Buf("theta", "inout", dev(np.array([theta], np.float32)), offset_bytes=off) if with_state else None,
                     Buf("batches", "inout", dev(np.array([batches], np.int64))) if with_state else None, lr,
                     WS, WS_BYTES, STREAM], front, sizer=("qsaebd_encode_batch_topk_workspace_bytes", (B, D, H, K)), expect=expect)
    return build


def _guard_cases():
    cases = {}
    for kind in KINDS:
        for B, D, H, K, with_bias in SHAPES:
            cases[f"{kind}_{B}x{D}_H{H}_K{K}"] = ("qsaebd_encode_batch_topk", _guard_encode(kind, B, D, H, K, with_bias))
    cases["certified_70x36_H300_K64_off4"] = ("qsaebd_encode_batch_topk", _guard_encode("certified", 70, 36, 300, 64, True, off=4))
    return cases


#: label -> (entry point, builder of its guard_util.Call); tests/test_batch_dense_host.py reads the entry points for its ledger.
#: Building a case touches the GPU; importing this table does not.
GUARD_CASES = _guard_cases()


def test_the_shapes_cover_every_value():
    for i, values in enumerate(((1, 3, 70, 130), (4, 36, 512), (8, 300, 1100), (1, 5, 64, 65, 256), (True, False))):
        assert {s[i] for s in SHAPES} == set(values)
    assert all(K <= H for _, _, H, K, _ in SHAPES)


@pytest.mark.parametrize("kind", KINDS + ("off4",))
def test_entry_point_between_guard_words(kind):
    labels = [label for label in sorted(GUARD_CASES) if (label.endswith("_off4") if kind == "off4" else
                                                          label.startswith(kind + "_") and not label.endswith("_off4"))]
    assert len(labels) == (1 if kind == "off4" else len(SHAPES))
    for label in labels:
        entry, build = GUARD_CASES[label]
        call = build()
        assert call.entry == entry
        GU.run_call(call, _lib.load(), DEV)


# ---- one batch, five floors -----------------------------------------------------------------------------------------------
FLOOR_SHAPES = ((70, 36, 300, 64, True), (130, 4, 1100, 256, False))


@pytest.mark.parametrize("shape", FLOOR_SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_the_result_does_not_depend_on_the_floor(shape):
    B, D, H, K, with_bias = shape
    x, W, bias = U.operands(B, D, H, 17, with_bias)
    z = U.preact(x, W, bias)
    n_select = B * k_of(K)
    ref = U.capped_reference_from_z(z, K, n_select)
    m = U.bits_f32(ref[3][3])
    assert m > 0 and ref[3][0] == n_select
    floors = {"-inf": -INF, "+0": 0.0, "0.9 m": float(np.float32(0.9) * m), "m": float(m), "2 m": float(np.float32(2.0) * m)}
    if H == 1100:                                              # the path coverage this shape exists for
        assert U.rows_resolved(z, 0.0).mean() > 0.5
    t_ref, b_ref = U.BT.threshold_update(np.float32(0.5), 3, ref[3], np.float32(0.25))
    dx, dW, db = dev(x), dev(W), None if bias is None else dev(bias)
    for name, floor in floors.items():
        theta, batches = torch.full((), 0.5, dtype=F32, device=DEV), torch.full((), 3, dtype=I64, device=DEV)
        idx_sel, val_sel, counts, report = ops.encode_batch_topk(dx, dW, db, n_select, K, floor, 1.0, (theta, batches, 0.25))
        rep = host(report)
        same(counts, ref[2], f"{name}: counts"), same(val_sel, ref[1], f"{name}: val_sel"), same(idx_sel, ref[0], f"{name}: idx_sel")
        assert rep[:4].tolist() == ref[3].tolist(), (name, rep.tolist(), ref[3].tolist())
        same(theta, np.float32(t_ref), f"{name}: theta")
        assert int(batches) == b_ref == 4
        assert rep[5] == (1 if name in ("m", "2 m") else 0), (name, rep.tolist())
        assert rep[7] == U.f32_bits(floor) and rep[4] <= B * K
        print(shape, name, "candidates per row", rep[4] / B, "rows over the cap", rep[6], "second attempt", rep[5])


def test_a_nan_floor_runs_the_second_attempt_and_the_device_floor_follows_the_batch():
    B, D, H, K, n_select = 70, 36, 300, 64, 70 * 16
    x, W, bias = U.operands(B, D, H, 17)
    ref = U.capped_reference_from_z(U.preact(x, W, bias), K, n_select)
    m = U.bits_f32(ref[3][3])
    floor = torch.full((), NAN, dtype=F32, device=DEV)
    for step, second in ((0, 1), (1, 0)):                      # the first call seeds the floor word, the second is certified by it
        idx_sel, val_sel, counts, report = ops.encode_batch_topk(dev(x), dev(W), dev(bias), n_select, K, floor, 0.75)
        same(counts, ref[2], "counts"), same(val_sel, ref[1], "val_sel"), same(idx_sel, ref[0], "idx_sel")
        assert int(report[5]) == second and host(report)[:4].tolist() == ref[3].tolist()
        same(floor, np.float32(np.float32(0.75) * m), "the floor word")
    # nothing selected: neither the floor nor the threshold state is written, and any floor certifies
    floor.fill_(NAN)
    theta, batches = torch.full((), 0.5, dtype=F32, device=DEV), torch.zeros((), dtype=I64, device=DEV)
    idx_sel, val_sel, counts, report = ops.encode_batch_topk(dev(x), dev(W), dev(bias), 0, K, floor, 0.75, (theta, batches, 0.25))
    assert host(report)[:6].tolist() == [0, 0, B, 0, 0, 0] and bool(torch.isnan(floor)) and float(theta) == 0.5 and int(batches) == 0
    assert (host(idx_sel) == -1).all() and not host(val_sel).view(np.uint32).any() and not host(counts).any()


def test_both_front_ends_and_the_dispatcher_op():
    B, D, H, K, n_select = 70, 36, 300, 64, 70 * 16
    x, W, bias = U.operands(B, D, H, 5)
    want = U.encode_batch_topk(x, W, bias, K, n_select, 0.25)
    for mod in (ops, torch_ops):
        got = mod.encode_batch_topk(dev(x), dev(W), dev(bias), n_select, K, 0.25)
        for g, w, name in zip(got, want, U.NAMES):
            same(g, w, name)
        got = mod.encode_batch_topk(dev(x), dev(W), None, n_select, K, 0.25, 0.5)
        same(got[2], U.encode_batch_topk(x, W, None, K, n_select, 0.25)[2], "counts without a bias")
    empty = ops.encode_batch_topk(dev(x[:0]), dev(W), dev(bias), 0, K, 0.25)
    assert tuple(empty[0].shape) == (0, K) and host(empty[3]).tolist() == [0] * 8
    assert ops.BATCH_DENSE_MAX_K == torch_ops.BATCH_DENSE_MAX_K == 256
    with pytest.raises(ValueError, match="floor_ratio"):
        ops.encode_batch_topk(dev(x), dev(W), dev(bias), n_select, K, 0.25, 1.5)
    with pytest.raises(ValueError, match="K = 301"):
        ops.encode_batch_topk(dev(x), dev(W), dev(bias), n_select, 301, 0.25)
    with pytest.raises(ValueError, match="n_select"):
        ops.encode_batch_topk(dev(x), dev(W), dev(bias), B * K + 1, K, 0.25)
    Q = torch.ops.qsae
    floor, theta, batches = torch.full((), 0.25, dtype=F32, device=DEV), torch.zeros((), dtype=F32, device=DEV), \
        torch.zeros((), dtype=I64, device=DEV)
    torch.library.opcheck(Q.encode_batch_topk.default, (dev(x), dev(W), dev(bias), n_select, K, floor, 0.0, 0.75, theta, batches, 0.25))
    torch.library.opcheck(Q.encode_batch_topk.default, (dev(x), dev(W), None, B, 5, None, 0.25, 1.0, None, None, 0.0))


# ---- the two top-k model classes ----------------------------------------------------------------------------------------
D_, H_, K_, CAP_, B_ = 64, 512, 8, 32, 64
CONFIG = {"input_dim": D_, "n_bits": 4, "hidden_dim": H_, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": K_,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": B_}
KIND = {"baseline_sae": "baseline", "b_sae": "binary"}
BOUNDS = [64, 128, 256, 512]
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
def rows():
    return dev(S.activations(91, B_, D_))


def _prefix_equal(a, b, counts, what):
    a, b = host(a), host(b)
    for r, c in enumerate(host(counts).tolist()):
        assert np.array_equal(a[r, :c].view(np.uint32), b[r, :c].view(np.uint32)), (what, r)


def _run(sae_type, rows, nested, floor):
    """-> (eval tuple, train outputs, grads, counts, report, threshold state) of one model under ``floor`` (None: capped)"""
    model = _model(KIND[sae_type])
    ctl = BatchTopK(model, cap=CAP_, dense=floor is not None)
    if floor is not None:
        ctl.floor.fill_(floor)
        ctl.floor_seeded = True
    if floor is None:
        lists = model.forward_nested_batch_topk(rows, ctl, BOUNDS) if nested else model.forward_batch_topk(rows, ctl)
    else:
        lists = model.forward_nested_batch_topk_dense(rows, ctl, BOUNDS) if nested else model.forward_batch_topk_dense(rows, ctl)
        assert float(ctl.floor) == np.float32(floor) and int(ctl.batches) == 0      # evaluation moves neither
    x = rows.clone().requires_grad_()
    if nested:
        train = model.forward_train_nested_batch_topk if floor is None else model.forward_train_nested_batch_topk_dense
        out = train(x, ctl, BOUNDS)
        nested_loss(sae_type, out, rows, CONFIG)
        flat = [out[0]] + list(out[1]) + list(out[2:])
    else:
        train = model.forward_train_batch_topk if floor is None else model.forward_train_batch_topk_dense
        out = train(x, ctl)
        trainer_loss(sae_type, out, rows, CONFIG)
        flat = list(out)
    assert all(o.grad_fn is not None for o in flat)
    grads = dict({k: p.grad.detach().clone() for k, p in model.named_parameters()}, x=x.grad.detach().clone())
    return lists, [o.detach() for o in flat], grads, ctl.counts.clone(), host(ctl.report).copy(), (float(ctl.theta), int(ctl.batches)), ctl


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_dense_models_equal_the_capped_ones(sae_type, nested, rows):
    c_lists, c_out, c_grads, c_counts, c_report, c_state, _ = _run(sae_type, rows, nested, None)
    m = U.bits_f32(c_report[3])
    assert m > 0 and c_report[0] == B_ * K_ and c_report[1] == 0
    for name, floor, second in (("0.9 m", float(np.float32(0.9) * m), 0), ("2 m", float(np.float32(2.0) * m), 1)):
        d_lists, d_out, d_grads, d_counts, d_report, d_state, ctl = _run(sae_type, rows, nested, floor)
        assert int(ctl.report_dense[5]) == second and ctl.dense_summary()["second_attempts"] == 2 * second, name
        same(d_counts, c_counts, "counts")
        assert d_report.tolist() == c_report.tolist() and d_state == c_state
        same(ctl.floor, np.float32(np.float32(ctl.floor_ratio) * m), "the floor after the training step")
        _prefix_equal(d_lists[0], c_lists[0], c_counts, "idx"), _prefix_equal(d_lists[1], c_lists[1], c_counts, "val_sel")
        same(d_lists[2], c_lists[2], "counts of the evaluation"), same(d_lists[3], c_lists[3], "the evaluation's reconstruction")
        hi, hc = host(d_lists[0]), host(d_counts)
        assert all((hi[r, c:] == -1).all() for r, c in enumerate(hc.tolist()))
        assert len(d_out) == len(c_out)
        for i, (g, w) in enumerate(zip(d_out, c_out)):
            same(g, w, f"{name}: output {i}")
        assert sorted(d_grads) == sorted(c_grads)
        for k in c_grads:
            same(d_grads[k], c_grads[k], f"{name}: {k}.grad")
            assert float(c_grads[k].abs().max()) > 0, k


def test_an_unseeded_controller_runs_capped_once_and_seeds_the_floor(rows):
    model = _model("baseline")
    ctl = BatchTopK(model, cap=CAP_, dense=True, floor_ratio=0.75)
    assert not ctl.floor_seeded and bool(torch.isnan(ctl.floor))
    model.forward_train_batch_topk_dense(rows, ctl)
    assert ctl.floor_seeded and ctl.report_dense is None and ctl.dense_selections == 0
    m = U.bits_f32(host(ctl.report)[3])
    same(ctl.floor, np.float32(np.float32(0.75) * m), "the seeded floor")
    model.forward_train_batch_topk_dense(rows, ctl)
    assert ctl.dense_selections == 1 and int(ctl.report_dense[5]) == 0 and int(ctl.batches) == 2
    sd = ctl.state_dict()
    other = BatchTopK(model, cap=CAP_, dense=True, floor_ratio=0.75)
    other.load_state_dict(sd)
    assert other.floor_seeded and float(other.floor) == float(ctl.floor)
    old = {k: v for k, v in sd.items() if k != "dense_floor"}     # a state saved before the floor existed
    other = BatchTopK(model, cap=CAP_, dense=True)
    other.load_state_dict(old)
    assert not other.floor_seeded and other.threshold() == ctl.threshold()
    with pytest.raises(ValueError, match="dense=True"):
        model.forward_train_batch_topk_dense(rows, BatchTopK(model, cap=CAP_))


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_three_steps_of_the_dense_trainer_equal_the_capped_trainer(sae_type, nested, tmp_path, monkeypatch):
    import quantizedsae_amd.training.trainer as TR
    made, real = [], TR.optim.Adam

    def recording(*args, **kw):                               # the epoch's optimizer, for its state
        made.append(real(*args, **kw))
        return made[-1]
    monkeypatch.setattr(TR.optim, "Adam", recording)
    rows = dev(S.activations(91, 3 * B_, D_))                 # one epoch of three batches under one Adam
    final, logs = {}, {}
    for dense in (False, True):
        logs[dense] = []
        model = _model(KIND[sae_type])
        if sae_type == "baseline_sae":
            model.normalize_decoder_weights()
        t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path),
                    log_fn=logs[dense].append, log_every=1, batch_topk=True, batch_topk_cap=CAP_, batch_topk_dense=dense,
                    batch_topk_nested_bounds=BOUNDS if nested else None, **({"batch_topk_floor_ratio": 0.9} if dense else {}))
        assert t.batch_topk_dense is dense and t.batch_topk.dense is dense
        torch.manual_seed(29)                                 # the loader shuffles the chunk's rows with the default generator
        t.one_epoch(rows)
        assert int(t.batch_topk.batches) == 3
        final[dense] = dict({k: v.detach().clone() for k, v in model.state_dict().items()}, theta=t.batch_topk.theta.clone(),
                            batches=t.batch_topk.batches.clone())
        n_adam = 0
        for i, st in enumerate(made[-1].state.values()):
            for k, v in st.items():
                if isinstance(v, torch.Tensor):
                    final[dense][f"adam_{i}_{k}"] = v.detach().clone()
                    n_adam += 1
        assert n_adam > 0
    assert len(logs[False]) == len(logs[True]) == 3
    assert all("batch_topk/second_attempts" in m and "batch_topk/candidates_per_row" in m for m in logs[True])
    assert all("batch_topk/second_attempts" not in m for m in logs[False])
    print(sae_type, nested, [(m["batch_topk/second_attempts"], m["batch_topk/candidates_per_row"]) for m in logs[True]])
    assert logs[True][0]["batch_topk/candidates_per_row"] == CAP_ and 0 < logs[True][2]["batch_topk/candidates_per_row"] <= CAP_
    for a, b in zip(logs[False], logs[True]):
        for key in a:
            if "loss" in key or key.startswith("batch_topk/") or key.startswith("l0_level"):
                assert a[key] == b[key], (key, a[key], b[key])
    assert sorted(final[False]) == sorted(final[True])
    for k in final[False]:
        same(final[True][k], final[False][k], k)
