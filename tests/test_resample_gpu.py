"""Resampling dead units on the GPU (csrc/resample.hip, quantizedsae_amd.training.resample): the five entry points bit for
bit against the numpy restatement of tests/resample_util.py -- both sides perform the same IEEE operations in the same order,
the library is built without contracted multiply-adds, so the tolerance is zero --, every entry point between guard words,
``resample_dead`` on the two top-k model classes, and the Trainer's ``resample_every``.

What is tested is the arithmetic and the plumbing.  Whether revived units stay alive on real data is not: no trained
checkpoint and no real activations exist offline."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard_util as GU  # noqa: E402
import resample_util as U  # noqa: E402
import trainer_util as TU  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call  # noqa: E402
from quantizedsae_amd import _lib, ops, optim  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402,F401
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import FeatureActivity, Trainer, resample_dead, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I64, I32, F32, F64 = torch.int64, torch.int32, torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _grad_mode_on():
    with torch.enable_grad():
        yield


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def same(got, want, what=""):
    got = host(got) if isinstance(got, torch.Tensor) else np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got.view(np.uint8) != want.view(np.uint8)).sum())} bytes differ"


# ---- row weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", U.ROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_weights_equal_the_restatement(shape):
    N, D, ld = shape
    x, recon = U.rows_case(N, D, ld)
    xd, rd = dev(x), dev(recon)
    w = ops.resample_row_weights(xd[:, :D], rd[:, :D])         # a row stride above D is read in place
    want = U.row_weights(x[:, :D], recon[:, :D])
    same(w, want, "w")
    same(torch.ops.qsae.resample_row_weights(xd[:, :D], rd[:, :D]), want, "w through the dispatcher")
    if N >= 8:                                                  # NaN, +-inf and the fp32 overflow: weight 0; 3e38: the finite value
        w = host(w)
        assert (w[[1, 2, 3, 4, 6]] == 0).all() and np.isfinite(w[5]) and w[5] > 1e150 and (w[7:] > 0).all()


# ---- draw ------------------------------------------------------------------------------------------------------------------------
def _draw(w, u):
    rows, report = ops.resample_draw(dev(w), dev(u))
    want_rows, want_report = U.draw(w, u)
    same(rows, want_rows, "rows")
    same(report, want_report, "report")
    return host(rows), host(report)


@pytest.mark.parametrize("case", [(1, 1), (1029, 67), (70001, 1000)], ids=lambda c: f"N{c[0]}_n{c[1]}")
def test_draw_equals_the_restatement(case):
    N, n = case
    w = U.weights_case(N, zeros=N > 1)
    if N == 1:
        w[0] = 2.5
    u = U.uniforms(n)                                           # holds 0 and nextafter(1, 0)
    rows, report = _draw(w, u)
    drawn = rows[rows >= 0]
    assert (w[drawn] > 0).all() and np.unique(drawn).size == drawn.size        # never a zero-weight row, never a row twice
    assert rows[0] == np.flatnonzero(w > 0)[0] and report[U.DEAD] == n
    again, _ = _draw(w, u)
    assert again.tobytes() == rows.tobytes()


def test_draw_without_weight_and_with_three_rows():
    rows, report = _draw(np.zeros(1029), U.uniforms(67))
    assert (rows == U.NO_ROW).all() and report.tolist() == [67, 0, 0, 0, 67, 0, 0, 0]
    w = np.zeros(1029)
    w[[5, 500, 1028]] = 1.0, 2.0, 3.0
    u = U.uniforms(67, seed=3)
    rows, report = _draw(w, u)
    kept = np.flatnonzero(rows >= 0)
    assert 1 <= kept.size <= 3 and report[U.DUPLICATE] == 67 - kept.size and rows[0] == 5 and rows[66] == U.LOST_ROW
    raw = np.array([int(np.argmax(U.prefix_sum(w) > t)) for t in u * 6.0])
    for j in kept:                                              # the owner of a row is the lowest j that drew it
        assert j == np.flatnonzero(raw == rows[j])[0]


# ---- alive statistics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 1000])
def test_alive_stats_equal_the_restatement(H):
    D, nb = 36, 4
    W, _, logits, _ = U.model_case(H, D, nb)
    Wd, Ld = dev(W), dev(logits)
    for dead in (np.zeros(0, np.int32), np.array([0, H - 1], np.int32), np.arange(H, dtype=np.int32)):
        same(ops.resample_alive_stats(Wd, Ld, dev(dead), nb), U.alive_stats(W, logits, dead), f"stats, {dead.size} dead")
        same(ops.resample_alive_stats(Wd, None, dev(dead)), U.alive_stats(W, None, dead), f"stats without logits, {dead.size} dead")


# ---- the two writes ----------------------------------------------------------------------------------------------------------------
def _write(c, *, moments=True, last=True, logit_scale=None, rows_seen=4242, through=ops):
    t = {k: dev(c[k]) for k in ("dead", "rows", "x", "dec_bias", "stats", "W_enc", "b_enc", "dec", "report", "last")}
    m = [dev(a) for a in c["moments"]]
    args = (t["W_enc"], t["b_enc"], t["dec"], t["dead"], t["rows"], t["x"], t["dec_bias"], t["stats"], t["report"])
    kw = dict(moments=m if moments else None, last=t["last"] if last else None, rows_seen=rows_seen, encoder_scale=0.2)
    if c["n_bits"] is None:
        through.resample_write_table(*args, **kw)
    else:
        through.resample_write_binary(*args, c["n_bits"], logit_scale=logit_scale, **kw)
    want = U.write(c["dead"], c["rows"], c["x"], c["dec_bias"], c["stats"], c["W_enc"], c["b_enc"], c["dec"], c["report"],
                   n_bits=c["n_bits"], moments=c["moments"] if moments else None, last=c["last"] if last else None,
                   rows_seen=rows_seen, logit_scale=logit_scale)
    for name in ("W_enc", "b_enc", "dec", "report"):
        same(t[name], want[name], name)
    for i in range(6):                                          # zero at exactly the written positions, unchanged elsewhere
        same(m[i], want["moments"][i] if moments else c["moments"][i], f"moment {i}")
    same(t["last"], want["last"] if last else c["last"], "last")
    for name in ("dead", "rows", "x", "dec_bias", "stats"):
        same(t[name], c[name], name)
    return want, {**{k: host(v) for k, v in t.items()}, "moments": [host(a) for a in m]}


@pytest.mark.parametrize("n_bits", [None, 1, 4, 8], ids=lambda b: f"bits{b}")
@pytest.mark.parametrize("shape", U.WRITE_SHAPES, ids=lambda s: f"H{s[0]}_D{s[1]}")
def test_writes_equal_the_restatement(shape, n_bits):
    H, D = shape
    c = U.write_case(H, D, n_bits)
    n = c["dead"].size
    assert c["dead"][0] == 0 and c["dead"][-1] == H - 1 and (c["rows"] == U.NO_ROW).sum() == 1
    want, got = _write(c)
    assert want["report"].tolist()[:6] == [n, n - 3, 1, 1, 1, 0]                # one degenerate, one -1, one -2 are left alone
    revived = [int(h) for j, h in enumerate(c["dead"]) if j not in (1, 2, 3)]
    others = np.setdiff1d(np.arange(H), revived)
    # every position not written is the snapshot's bits (the comparison above says so through the restatement; here directly)
    assert got["W_enc"][others].tobytes() == c["W_enc"][others].tobytes() and (got["b_enc"][revived] == 0).all()
    assert got["b_enc"][others].tobytes() == c["b_enc"][others].tobytes()
    dec_rows = got["dec"] if n_bits else got["dec"].T
    assert np.ascontiguousarray(dec_rows[others]).tobytes() == np.ascontiguousarray((c["dec"] if n_bits else c["dec"].T)[others]).tobytes()
    assert (got["moments"][0][revived] == 0).all() and (got["moments"][3][revived] == 0).all()
    assert (got["last"][revived] == 4242).all() and (got["last"][others] == c["last"][others]).all()
    _, again = _write(c)                                        # a second run: the same bits
    assert all(again[k].tobytes() == got[k].tobytes() for k in ("W_enc", "b_enc", "dec", "report", "last"))
    _write(c, moments=False, last=False, logit_scale=2.5 if n_bits else None, through=torch_ops)     # null optimizer and tracker


@pytest.mark.parametrize("n_bits", [None, 8], ids=lambda b: f"bits{b}")
def test_writes_at_the_largest_row(n_bits):
    _write(U.write_case(4, 4096, n_bits, n=2))


def test_out_of_order_and_out_of_range_entries_are_skipped_never_written():
    c = U.write_case(1000, 36, 4)
    c["dead"] = np.array([5, 5, 1000, -1, 7, 6, 999], np.int32)
    c["rows"] = np.array([0, 1, 2, 3, 4, 5, c["N"]], np.int32)
    c["x"] = np.random.default_rng(9).standard_normal(c["x"].shape).astype(np.float32)
    want, _ = _write(c)
    assert want["report"][U.SKIPPED] == 5 and want["report"][U.REVIVED] == 2


# ---- guards --------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = {"qsae_resample_row_weights", "qsae_resample_draw", "qsae_resample_draw_workspace_bytes", "qsae_resample_alive_stats",
                "qsae_resample_write_table", "qsae_resample_write_binary"}


def guard_calls(shape):
    tails = shape == "tails"
    calls = []
    N, D, ld = (1029, 516, 520) if tails else (1, 4, 4)
    x, recon = U.rows_case(N, D, ld)
    calls.append(Call(f"row weights {N}x{D} ld={ld}", "qsae_resample_row_weights",
                      [Buf("x", "in", data=dev(x)), ld, Buf("recon", "in", data=dev(recon)), ld, N, D,
                       Buf("w", "out", shape=(N,), dtype=F64), STREAM],
                      lambda t, D=D: {"w": dev(U.row_weights(host(t["x"])[:, :D], host(t["recon"])[:, :D]))}))
    N, n = (1029, 67) if tails else (1, 1)
    w = U.weights_case(N, zeros=tails) if tails else np.array([2.5])

    def draw_front(t):
        rows, report = U.draw(host(t["w"]), host(t["u"]))
        return {"rows": dev(rows), "report": dev(report)}
    calls.append(Call(f"draw N={N} n={n}", "qsae_resample_draw",
                      [Buf("w", "in", data=dev(w)), N, Buf("u", "in", data=dev(U.uniforms(n))), n,
                       Buf("rows", "out", shape=(n,), dtype=I32), Buf("report", "out", shape=(U.REPORT_WORDS,), dtype=I64),
                       WS, WS_BYTES, STREAM], draw_front, sizer=("qsae_resample_draw_workspace_bytes", (N,))))
    H, D, nb = (1000, 36, 4) if tails else (4, 4, 1)
    W, _, logits, _ = U.model_case(H, D, nb)
    dead = np.array([0, H - 1], np.int32)

    def alive_front(t):
        Wh, Lh = host(t["W_enc"]).astype(np.float64), host(t["logits"]).astype(np.float64)
        return {"unit_norm": dev(np.sqrt(U.block_sum(Wh * Wh))), "unit_abs": dev(U.block_sum(np.abs(Lh))),
                "stats": dev(U.alive_stats(host(t["W_enc"]), host(t["logits"]), host(t["dead"])))}
    calls.append(Call(f"alive stats H={H} D={D}", "qsae_resample_alive_stats",
                      [Buf("W_enc", "in", data=dev(W)), H, D, Buf("logits", "in", data=dev(logits)), nb, Buf("dead", "in", data=dev(dead)),
                       2, Buf("unit_norm", "out", shape=(H,), dtype=F64), Buf("unit_abs", "out", shape=(H,), dtype=F64),
                       Buf("stats", "out", shape=(2,), dtype=F64), STREAM], alive_front))
    for nb in (None, 4):
        H, D = (1000, 260) if tails else (4, 4)
        c = U.write_case(H, D, nb)
        names = ("m_We", "v_We", "m_be", "v_be", "m_dec", "v_dec")

        def write_front(t, c=c, nb=nb, names=names):
            out = U.write(c["dead"], c["rows"], c["x"], c["dec_bias"], c["stats"], host(t["W_enc"]), host(t["b_enc"]), host(t["dec"]),
                          host(t["report"]), n_bits=nb, moments=[host(t[k]) for k in names], last=host(t["last"]), rows_seen=77)
            res = {k: dev(out[k]) for k in ("W_enc", "b_enc", "dec", "report", "last")}
            res.update({k: dev(m) for k, m in zip(names, out["moments"])})
            return res
        args = [Buf("dead", "in", data=dev(c["dead"])), Buf("rows", "in", data=dev(c["rows"])), c["dead"].size,
                Buf("x", "in", data=dev(c["x"])), D, c["N"], D, H] + ([nb] if nb else []) + \
               [Buf("dec_bias", "in", data=dev(c["dec_bias"])), Buf("stats", "in", data=dev(c["stats"])), 0.2] + ([0, 0.0] if nb else []) + \
               [Buf("W_enc", "inout", data=dev(c["W_enc"])), Buf("b_enc", "inout", data=dev(c["b_enc"])), Buf("dec", "inout", data=dev(c["dec"]))] + \
               [Buf(k, "inout", data=dev(m)) for k, m in zip(names, c["moments"])] + \
               [Buf("last", "inout", data=dev(c["last"])), 77, Buf("report", "inout", data=dev(c["report"])), STREAM]
        calls.append(Call(f"write {'binary' if nb else 'table'} H={H} D={D}", f"qsae_resample_write_{'binary' if nb else 'table'}",
                          args, write_front))
    return calls


@pytest.mark.parametrize("shape", ["minimal", "tails"])
def test_entry_points_between_guards(shape):
    lib = _lib.load()
    calls = guard_calls(shape)
    assert {c.entry for c in calls} | {c.sizer[0] for c in calls if c.sizer} == ENTRY_POINTS
    for call in calls:
        GU.run_call(call, lib, DEV)


# ---- the two model classes -------------------------------------------------------------------------------------------------------
MODEL_B, MODEL_D, MODEL_H = 48, 64, 1000


def _model(kind, seed=31):
    if kind == "b_sae":
        model = BinarySAE(MODEL_D, MODEL_H, 4.0, 8)
        sd = TU.S.binary_sae_params(seed, MODEL_D, MODEL_H, 8, dec_bias_std=0.05, logit_std=2.0)
    else:
        model = BaselineSparseAutoencoder(MODEL_D, MODEL_H)
        sd = TU.S.baseline_sae_params(seed, MODEL_D, MODEL_H, bias_std=0.05)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return model.to(DEV)


@pytest.mark.parametrize("kind,opt", [("baseline_sae", "torch"), ("b_sae", "qsae"), ("b_sae", None)])
def test_resample_dead_rewrites_the_model_as_the_restatement_says(kind, opt):
    model = _model(kind)
    x = dev(TU.S.activations(77, MODEL_B, MODEL_D))
    tracker = model.activity = FeatureActivity.for_model(model)
    optimizer = None
    if opt is not None:
        optimizer = (torch.optim.Adam if opt == "torch" else optim.Adam)(model.parameters(), lr=1e-3)
    cfg = dict(TU.epoch_config(), input_dim=MODEL_D, hidden_dim=MODEL_H)
    outputs = model.forward_train(x)                            # one training step: the tracker is fed, the moments exist
    trainer_loss(kind, outputs, x, cfg)
    if optimizer is not None:
        optimizer.step()
    with torch.no_grad():
        model(x)                                                # the derived copies of the weights exist now
    s = tracker.summary(MODEL_B, dead_list=True, advance=False)
    n = s.dead
    assert 0 < n < MODEL_H and tracker.rows_seen == MODEL_B
    lin, dec = model.encoder.linear, model.decoder
    params = (lin.weight, lin.bias, dec.weight)
    before = {k: host(v) for k, v in model.state_dict().items()}
    moments = None
    if optimizer is not None:
        moments = [host(optimizer.state[p][k]) for p in params for k in ("exp_avg", "exp_avg_sq")]
        steps = [float(optimizer.state[p]["step"]) for p in params]
    last0 = host(tracker.last)
    u = np.random.default_rng(5).random(n)
    recon = host(model.forward_compact(x)[2])
    report = resample_dead(model, s.dead_indices, x, optimizer=optimizer, activity=tracker, u=dev(u))
    # the restatement of the whole step
    dead = host(s.dead_indices)
    rows, rep = U.draw(U.row_weights(host(x), recon), u)
    nb = dec.n_bits if kind == "b_sae" else None
    W0, b0, d0, bias0 = (before[k] for k in ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.bias"))
    stats = U.alive_stats(W0, d0 if nb else None, dead)
    want = U.write(dead, rows, host(x), bias0, stats, W0, b0, d0, rep, n_bits=nb, moments=moments, last=last0, rows_seen=MODEL_B)
    same(report.rows, rows, "rows")
    same(report.block, want["report"], "report")
    assert report.revived == want["report"][U.REVIVED] > 0 and report.dead == n and report.duplicate == want["report"][U.DUPLICATE]
    after = model.state_dict()
    same(after["encoder.0.weight"], want["W_enc"], "W_enc")
    same(after["encoder.0.bias"], want["b_enc"], "b_enc")
    same(after["decoder.weight"], want["dec"], "decoder.weight")
    same(after["decoder.bias"], bias0, "decoder.bias")
    revived = dead[rows >= 0]
    revived = np.array([h for h in revived if want["b_enc"][h] == 0 and (want["W_enc"][h] != W0[h]).any()])
    assert revived.size == report.revived
    same(tracker.last, want["last"], "last")
    assert (host(tracker.last)[revived] == tracker.rows_seen).all()
    if optimizer is not None:
        got = [optimizer.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq")]
        for i in range(6):
            same(got[i], want["moments"][i], f"moment {i}")
        assert (host(got[0])[revived] == 0).all() and (host(got[3])[revived] == 0).all()
        assert [float(optimizer.state[p]["step"]) for p in params] == steps           # step is untouched
    # the derived copies were dropped: forward() equals the forward of a fresh model loaded from the state dict
    fresh = _model(kind, seed=99)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        got, ref = model(x), fresh(x)
    assert len(got) == len(ref) and all(GU.same_bits(a, b) for a, b in zip(got, ref))
    if kind == "b_sae":
        q = host(dec.quantized_int_weights())
        for h in revived:
            assert (q[h] == want["q"][int(h)]).all(), h


# ---- the Trainer -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def epoch_fixture():
    return TU.load_epoch_fixture()


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory, epoch_fixture):
    d = tmp_path_factory.mktemp("resample_dataset")
    torch.save(TU.epoch_chunk(epoch_fixture[0]["seed"]), d / TU.CHUNK_NAME)
    return d


PLANTED = [0, 1, 2]                                            # units made dead by an encoder bias of -1e30
RESAMPLE_KEYS = {"resample_dead", "resampled_features", "resample_duplicates", "resample_degenerate", "resample_no_weight",
                 "resample_skipped"}


def _epoch_model(sae_type, seed):
    from quantizedsae_amd.training.trainer import _build_model
    model = _build_model(sae_type, TU.epoch_config())
    sd = {k: torch.from_numpy(v) for k, v in TU.epoch_params(sae_type, seed).items()}
    sd["encoder.0.bias"] = sd["encoder.0.bias"].clone()
    sd["encoder.0.bias"][PLANTED] = -1e30
    model.load_state_dict(sd, strict=False)
    return model.to(DEV)


def _run_epoch(sae_type, meta, dataset_dir, tmp_path, **options):
    logs, entries = [], []
    t = Trainer(TU.epoch_config(), sae_type, False, True, model=_epoch_model(sae_type, meta["seed"]), dataset_dir=str(dataset_dir),
                save_dir=str(tmp_path), log_fn=logs.append, log_every=1, **options)
    step = t._step

    def spying_step(optimizer, batch, log_step):
        entries.append((batch.detach().clone(), {k: v.detach().clone() for k, v in t.model.state_dict().items()}))
        return step(optimizer, batch, log_step)
    t._step = spying_step
    torch.manual_seed(meta["seed"])
    t.one_epoch(str(dataset_dir / TU.CHUNK_NAME))
    return t, logs, entries


def _same_state(a, b):
    return list(a) == list(b) and all(GU.same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_trainer_resamples_on_its_steps_and_only_there(sae_type, epoch_fixture, dataset_dir, tmp_path, capsys):
    meta, _ = epoch_fixture
    W, R = 100, 2
    plain, logs0, entries0 = _run_epoch(sae_type, meta, dataset_dir, tmp_path)
    tracked, logs1, entries1 = _run_epoch(sae_type, meta, dataset_dir, tmp_path, activity_window=W)
    t, logs, entries = _run_epoch(sae_type, meta, dataset_dir, tmp_path, activity_window=W, resample_every=R, resample_seed=11)
    batches = t.trained_batches[-1]
    # resample_every=None: a whole epoch is the same bits with and without the tracker, and no resample key is logged
    assert _same_state(plain.model.state_dict(), tracked.model.state_dict())
    assert not any(RESAMPLE_KEYS & set(m) for m in logs0 + logs1) and tracked.resample_every is None
    # the loader's order is untouched: the same batches, bit for bit
    assert batches == plain.trained_batches[-1] == tracked.trained_batches[-1] and len(batches) == len(entries) == len(logs) >= 3
    assert all(torch.equal(a[0], b[0]) for a, b in zip(entries0, entries))
    # the resample metrics appear on exactly the steps with batch_idx % R == 0
    for b, m in zip(batches, logs):
        assert (RESAMPLE_KEYS <= set(m)) == (b % R == 0) and (not (RESAMPLE_KEYS & set(m)) or b % R == 0), b
    firsts = [i for i, (b, m) in enumerate(zip(batches, logs)) if b % R == 0 and m["resample_dead"] > 0]
    assert firsts, "no resampling step found a dead unit"
    first = firsts[0]
    m = logs[first]
    assert m["resample_dead"] >= len(PLANTED) and m["resampled_features"] >= 1
    assert (m["resampled_features"] + m["resample_duplicates"] + m["resample_degenerate"] + m["resample_no_weight"]
            + m["resample_skipped"]) == m["resample_dead"]
    # before the window has passed nothing is dead: the step reports zeros and launches nothing
    if batches[0] % R == 0:
        assert logs[0]["resample_dead"] == 0 and logs[0]["resampled_features"] == 0 and first > 0
    # up to the first resampling step that found something, the parameters are the bits of a run without the option
    for i in range(first + 1):
        assert _same_state(entries1[i][1], entries[i][1]), i
    final, final1 = t.model.state_dict(), tracked.model.state_dict()
    assert not GU.same_bits(final["encoder.0.weight"], final1["encoder.0.weight"])
    # unit 0 is the first drawer: it owns its row, and its bias left -1e30 behind
    assert float(final1["encoder.0.bias"][0]) < -1e29 and float(final["encoder.0.bias"][0]) > -1.0
    # under no_log: one printed line per resampling step
    capsys.readouterr()
    t.log_fn = None
    torch.manual_seed(meta["seed"])
    t.one_epoch(str(dataset_dir / TU.CHUNK_NAME))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "resample: revived=" in ln]
    assert len(lines) == sum(1 for b in t.trained_batches[-1] if b % R == 0)
