"""BatchTopK on the GPU (csrc/batch_topk.hip, csrc/batch_topk_decode.hip, include/qsae_batch.h): the batch-wide selection, the
threshold state and the threshold selection bit for bit against the numpy restatement of tests/batch_topk_util.py, on both front
ends; the ragged decode, row gradient and per-unit lists bit for bit against the restatement and against the existing ops
called per group of rows of equal count; all six entry points between guard words, twice on one workspace of exactly the sizer's
bytes; the dispatcher ops; and the two top-k model classes: forward_batch_topk, forward_train_batch_topk, forward_threshold and
the Trainer's ``batch_topk``."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import batch_topk_util as U  # noqa: E402
import guard_util as GU  # noqa: E402
import oracle  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call  # noqa: E402
from sparsity_curve_util import gaussian  # noqa: E402
from train_util import max_rel_err  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import BatchTopK, FeatureActivity, Trainer, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64, F32 = torch.int32, torch.int64, torch.float32
TOL = 1e-5                                                   # the project's bound on a gradient against fp64 (max_rel_err)


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


def straddling_n(val: np.ndarray) -> int:
    """an n_select whose tie class -- the most frequent value -- is cut in the middle (with heavy ties: across several rows)"""
    key = U.mono_key(val).reshape(-1)
    uniq, cnt = np.unique(key, return_counts=True)
    t = uniq[np.argmax(cnt)]
    return int((key > t).sum()) + max(1, int(cnt.max()) // 2)


# ---- the selection ------------------------------------------------------------------------------------------------------
def test_key_order_is_the_top_k_kernels():
    """mono_key of common.h as topk.hip applies it: NaN first, then +inf .. -inf, -0 == +0 (ties to the lower index)"""
    row = U.special_rows(16)[None, :].copy()
    idx, _ = ops.topk_rows(dev(row).clone(), 16, zero_rest=False)
    assert host(idx)[0].tolist() == U._key_order(row).tolist()
    counts, _, _ = ops.batch_select(dev(row[:, U._key_order(row)]), 5)
    assert host(counts).tolist() == [5]


@pytest.mark.parametrize("kind", U.SELECT_KINDS)
@pytest.mark.parametrize("shape", U.SELECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_selection_equals_the_restatement(shape, kind):
    B, K = shape
    val = U.select_values(kind, B, K, seed=B)
    dval = dev(val)
    for n in sorted({0, 1, B * max(1, K // 4), B * K, straddling_n(val)}):
        want = U.batch_select(val, n)
        for mod in (ops, torch_ops):
            counts, val_sel, report = mod.batch_select(dval, n)
            same(counts, want[0], f"counts n={n}")
            same(val_sel, want[1], f"val_sel n={n}")
            same(report, want[2], f"report n={n}")
        assert int(counts.sum()) == n == int(report[0])
        assert int(report[1]) == int((want[0] == K).sum()) and int(report[2]) == int((want[0] == 0).sum())
        counts2, none, _ = ops.batch_select(dval, n, want_val=False)
        assert none is None
        same(counts2, want[0], "the same bits on a second run")


def test_a_tie_class_that_straddles_rows():
    val = np.full((9, 7), 0.5, dtype=np.float32)
    val[:, 0] = 2.0
    counts, val_sel, report = ops.batch_select(dev(val), 9 + 6 * 3 + 2)      # the nine 2s, rows 0 .. 2 in full, two of row 3
    assert host(counts).tolist() == [7, 7, 7, 3, 1, 1, 1, 1, 1]
    same(report, U.batch_select(val, 29)[2])


def test_unsorted_rows_are_safe_and_exact():
    val = gaussian(41, 37, 21)
    val[3, 5], val[9, 0] = np.nan, -np.inf
    for n in (0, 1, 300, 37 * 21):
        counts, val_sel, report = ops.batch_select(dev(val), n)
        want = U.batch_select(val, n)
        assert int(counts.sum()) == n
        same(counts, want[0])
        same(val_sel, want[1])
        same(report, want[2])


def test_threshold_state_over_consecutive_batches():
    val = U.select_values("gaussian", 70, 64, seed=3)
    theta = torch.zeros((), dtype=F32, device=DEV)
    batches = torch.zeros((), dtype=I64, device=DEV)
    state = (np.float32(0.0), 0)
    for n, scale in ((70 * 16, 1.0), (70 * 16, 2.0), (70 * 60, 1.0), (70 * 8, 0.5)):     # the third batch has m <= 0
        v = (val * np.float32(scale)).astype(np.float32)
        mod = torch_ops if scale == 2.0 else ops
        _, _, report = mod.batch_select(dev(v), n, True, theta, batches, 0.01)
        want = U.batch_select(v, n)
        same(report, want[2])
        new = U.threshold_update(state[0], state[1], want[2], 0.01)
        assert (state[1] == new[1]) == (scale == 1.0 and n == 70 * 60)
        state = new
        same(theta, np.float32(state[0]), "theta")
        assert int(batches) == state[1]
    assert state[1] == 3


@pytest.mark.parametrize("kind", ["gaussian", "eight_levels", "special"])
def test_threshold_selection_equals_the_restatement(kind):
    for B, K in ((1, 1), (3, 5), (70, 64), (257, 33), (5, 256)):
        val = U.select_values(kind, B, K, seed=B + 1)
        dval = dev(val)
        present = val[B // 2, K // 2]
        for theta in (present, np.nan, np.inf, -np.inf, 0.0, -0.0):
            want = U.threshold_select(val, theta)
            for mod, arg in ((ops, float(theta)), (torch_ops, torch.tensor(theta, dtype=F32, device=DEV))):
                got = mod.threshold_select(dval, arg)
                for g, w, what in zip(got, want, ("counts", "val_sel", "report")):
                    same(g, w, f"{what} theta={theta}")


# ---- ragged rows --------------------------------------------------------------------------------------------------------
def _dev_decoder(decoder):
    return (decoder[0], dev(decoder[1])) + tuple(decoder[2:])


def decode_ragged(mod, idx, val, counts, dd, bias):
    if dd[0] == "packed":
        return mod.decode_ragged_binary(idx, val, counts, dd[1], dd[2], dd[3], dd[4], bias)
    return mod.decode_ragged_table(idx, val, counts, dd[1], dd[2], bias)


def decode_plain(idx, val, dd, bias):
    if dd[0] == "packed":
        return ops.decode_binary_sparse(idx, val, dd[1], dd[2], dd[3], dd[4], bias)
    return ops.decode_table_sparse(idx, val, dd[1], dd[2], bias)


@pytest.mark.parametrize("name", sorted(U.RAGGED_CASES))
def test_ragged_decode(name):
    idx, val, decoder, bias, H = U.ragged_case(name)
    B, K = idx.shape
    dd, di, dv, db = _dev_decoder(decoder), dev(idx), dev(val), None if bias is None else dev(bias)
    D = decoder[2] if decoder[0] == "packed" else decoder[1].shape[1]
    for pattern, counts in U.count_patterns(B, K).items():
        want = U.decode_ragged(idx, val, counts, decoder, bias)
        for mod in (ops, torch_ops):
            got = decode_ragged(mod, di, dv, dev(counts), dd, db)
            same(got, want, f"{pattern} against the restatement")
        c = U.clamp_counts(counts, K)
        for n in np.unique(c):                               # the plain op per group of rows of equal count
            rows = np.nonzero(c == n)[0]
            if n == 0:
                zero = np.float32(0) + (bias if bias is not None else np.zeros(D, np.float32))
                same(got[dev(rows)], np.broadcast_to(zero, (len(rows), D)).copy(), "count 0 gives the bias")
                continue
            same(got[dev(rows)], decode_plain(dev(idx[rows, :n]), dev(val[rows, :n]), dd, db), f"{pattern}: plain op, count {n}")
        # the plain decode of (idx, val_sel): zeros behind the prefix change nothing on a finite dictionary
        val_sel = np.where(np.arange(K)[None, :] < c[:, None], val, np.float32(0)).astype(np.float32)
        same(got, decode_plain(di, dev(val_sel), dd, db), f"{pattern}: plain decode of (idx, val_sel)")


def test_an_inf_dictionary_row_behind_a_prefix_does_not_show():
    idx, val, decoder, bias, H = U.ragged_case("table_D48")
    B, K = idx.shape
    idx = idx.copy()
    idx[0, 1], idx[0, 2] = [h for h in range(H) if h not in set(idx[0].tolist())][:2]      # every id inside, distinct per row
    counts = np.full(B, 3, np.int32)
    front = np.zeros(H, dtype=bool)
    front[idx[:, :3].reshape(-1)] = True
    table = decoder[1].copy()
    table[~front] = np.inf                                   # every unit that no prefix holds -- the units behind them among these
    assert np.isinf(table[idx[:, 3:]]).any(axis=(1, 2)).all()
    got = ops.decode_ragged_table(dev(idx), dev(val), dev(counts), dev(table), 1.0, dev(bias))
    assert bool(torch.isfinite(got).all())
    same(got, U.decode_ragged(idx, val, counts, ("table", table, 1.0), bias))
    gv, dx = ops.train_row_grad_ragged(dev(idx), dev(counts), dev(table), 1.0, dev(gaussian(7, B, 48)), None, dev(table), True)
    assert bool(torch.isfinite(gv).all()) and bool(torch.isfinite(dx).all()) and not host(gv)[:, 3:].view(np.uint32).any()


@pytest.mark.parametrize("name", [n for n in sorted(U.RAGGED_CASES) if n.startswith("table")])
def test_ragged_row_gradient_and_lists(name):
    idx, val, decoder, _, H = U.ragged_case(name)
    B, K = idx.shape
    table, D = decoder[1], decoder[1].shape[1]
    g, gl, W = gaussian(81, B, D), gaussian(82, B, H), gaussian(83, H, D)
    di, dt, dg, dgl, dW = dev(idx), dev(table), dev(g), dev(gl), dev(W)
    for pattern, counts in U.count_patterns(B, K).items():
        dc, c = dev(counts), U.clamp_counts(counts, K)
        off, ent = U.csr_ragged(idx, counts, H)
        for mod in (ops, torch_ops):
            o, e = mod.train_csr_ragged(di, dc, H)
            same(o, off, f"{pattern}: offsets")
            same(e, ent, f"{pattern}: entries")
        for use_g, use_gl, want_dx in ((True, True, True), (True, False, False), (False, True, True)):
            if K > 64 and (pattern != "mixed" or not use_g or not use_gl):
                continue                                      # the long lists once: the restatement walks them on the host
            gv, dx = ops.train_row_grad_ragged(di, dc, dt, 0.25, dg if use_g else None, dgl if use_gl else None, dW, want_dx)
            wgv, wdx = U.row_grad_ragged(idx, counts, table, 0.25, g if use_g else None, gl if use_gl else None, W if want_dx else None)
            same(gv, wgv, f"{pattern}: gv")
            if want_dx:
                same(dx, wdx, f"{pattern}: dx")
            for n in np.unique(c):                           # qsae_train_row_grad per group of rows of equal count
                rows = np.nonzero(c == n)[0]
                if n == 0:
                    continue
                r = dev(rows)
                pgv, pdx = ops.train_row_grad(dev(idx[rows, :n]), dt, 0.25, dg[r] if use_g else None, dgl[r] if use_gl else None,
                                              dW, want_dx)
                same(gv[r][:, :n], pgv, f"{pattern}: plain gv, count {n}")
                if want_dx:
                    same(dx[r], pdx, f"{pattern}: plain dx, count {n}")
    if K <= H:                                               # all counts == K, every id in range and distinct: qsae_train_csr
        inside = idx.copy()
        out = (inside[0] < 0) | (inside[0] >= H)
        inside[0, out] = [h for h in range(H) if h not in set(inside[0].tolist())][:int(out.sum())]
        o, e = ops.train_csr_ragged(dev(inside), dev(np.full(B, K, np.int32)), H)
        po, pe = ops.train_csr(dev(inside), H)
        same(o, po, "offsets of the plain lists")
        same(e, pe, "entries of the plain lists")


# ---- all six entry points between guard words ---------------------------------------------------------------------------
def _guard_select(kind, B, K, n, with_state):
    def build():
        val = U.select_values(kind, B, K, seed=B)
        want = U.batch_select(val, n)
        theta0, batches0 = np.float32(0.5), 4
        th, nb = U.threshold_update(theta0, batches0, want[2], 0.01)

        def front(t):
            theta, batches = (t["theta"].clone(), t["batches"].clone()) if with_state else (None, None)
            counts, val_sel, report = ops.batch_select(t["val"], n, True, theta, batches, 0.01)
            out = {"counts": counts, "val_sel": val_sel, "report": report}
            if with_state:
                out.update(theta=theta, batches=batches)
            return out
        expect = {"counts": torch.from_numpy(want[0]), "val_sel": torch.from_numpy(want[1]), "report": torch.from_numpy(want[2])}
        state = [None, None]
        if with_state:
            state = [Buf("theta", "inout", torch.full((1,), float(theta0), dtype=F32, device=DEV)),
                     Buf("batches", "inout", torch.full((1,), batches0, dtype=I64, device=DEV))]
            expect.update(theta=torch.tensor([th], dtype=F32), batches=torch.tensor([nb], dtype=I64))
        return Call(f"{kind}_{B}x{K}", "qsaeb_batch_select",
                    [Buf("val", "in", dev(val)), B, K, n, Buf("counts", "out", shape=(B,), dtype=I32),
                     Buf("val_sel", "out", shape=(B, K), dtype=F32), Buf("report", "out", shape=(4,), dtype=I64), *state, 0.01,
                     WS, WS_BYTES, STREAM], front, sizer=("qsaeb_batch_select_workspace_bytes", (B, K)), expect=expect)
    return build


def _guard_threshold(kind, B, K, on_device):
    def build():
        val = U.select_values(kind, B, K, seed=B)
        theta = val[B // 2, K // 2]
        want = U.threshold_select(val, theta)

        def front(t):
            counts, val_sel, report = ops.threshold_select(t["val"], t["theta"] if on_device else float(theta))
            return {"counts": counts, "val_sel": val_sel, "report": report}
        return Call(f"{kind}_{B}x{K}", "qsaeb_threshold_select",
                    [Buf("val", "in", dev(val)), B, K,
                     Buf("theta", "in", torch.full((1,), float(theta), dtype=F32, device=DEV)) if on_device else None,
                     0.0 if on_device else float(theta), Buf("counts", "out", shape=(B,), dtype=I32),
                     Buf("val_sel", "out", shape=(B, K), dtype=F32), Buf("report", "out", shape=(4,), dtype=I64),
                     WS, WS_BYTES, STREAM], front, sizer=("qsaeb_threshold_select_workspace_bytes", (B, K)),
                    expect={"counts": torch.from_numpy(want[0]), "val_sel": torch.from_numpy(want[1]),
                            "report": torch.from_numpy(want[2])})
    return build


def _guard_decode(name, pattern):
    def build():
        idx, val, decoder, bias, H = U.ragged_case(name)
        B, K = idx.shape
        counts = U.count_patterns(B, K)[pattern]
        packed = decoder[0] == "packed"
        D = decoder[2] if packed else decoder[1].shape[1]
        want = U.decode_ragged(idx, val, counts, decoder, bias)

        def front(t):
            dd = (decoder[0], t["dict"]) + tuple(decoder[2:])
            return {"recon": decode_ragged(ops, t["idx"], t["val"], t["counts"], dd, t.get("bias"))}
        dict_args = [Buf("dict", "in", dev(decoder[1])), H, D] + ([decoder[3], decoder[4]] if packed else [decoder[2]])
        entry = "qsaeb_decode_ragged_binary" if packed else "qsaeb_decode_ragged_table"
        return Call(f"{name}_{pattern}", entry,
                    [Buf("idx", "in", dev(idx)), Buf("val", "in", dev(val)), Buf("counts", "in", dev(counts)), B, K, *dict_args,
                     Buf("bias", "in", dev(bias)) if bias is not None else None, Buf("recon", "out", shape=(B, D), dtype=F32),
                     STREAM], front, expect={"recon": torch.from_numpy(want)})
    return build


def _guard_row(name, pattern):
    def build():
        idx, val, decoder, _, H = U.ragged_case(name)
        B, K = idx.shape
        counts = U.count_patterns(B, K)[pattern]
        table, D = decoder[1], decoder[1].shape[1]
        g, gl, W = gaussian(81, B, D), gaussian(82, B, H), gaussian(83, H, D)

        def front(t):
            gv, dx = ops.train_row_grad_ragged(t["idx"], t["counts"], t["table"], 0.25, t["g"], t["g_latent"], t["W"], True)
            return {"gv": gv, "dx": dx}
        return Call(f"{name}_{pattern}", "qsaeb_row_grad_ragged",
                    [Buf("idx", "in", dev(idx)), Buf("counts", "in", dev(counts)), B, K, Buf("table", "in", dev(table)), H, D, 0.25,
                     Buf("g", "in", dev(g)), Buf("g_latent", "in", dev(gl)), H, Buf("W", "in", dev(W)),
                     Buf("gv", "out", shape=(B, K), dtype=F32), Buf("dx", "out", shape=(B, D), dtype=F32), STREAM], front)
    return build


def _guard_csr(name, pattern):
    def build():
        idx, _, _, _, H = U.ragged_case(name)
        B, K = idx.shape
        counts = U.count_patterns(B, K)[pattern]
        off, ent = U.csr_ragged(idx, counts, H)

        def front(t):
            o, e = ops.train_csr_ragged(t["idx"], t["counts"], H)
            return {"offsets": o, "entries": e}
        return Call(f"{name}_{pattern}", "qsaeb_csr_ragged",
                    [Buf("idx", "in", dev(idx)), Buf("counts", "in", dev(counts)), B, K, H,
                     Buf("offsets", "out", shape=(H + 1,), dtype=I32), Buf("entries", "out", shape=(B * K,), dtype=I32),
                     WS, WS_BYTES, STREAM], front, sizer=("qsaeb_csr_ragged_workspace_bytes", (B, K, H)),
                    expect={"offsets": torch.from_numpy(off), "entries": torch.from_numpy(ent)})
    return build


#: label -> (entry point, builder of its guard_util.Call); tests/test_batch_topk_host.py reads the entry points for its ledger.
#: Building a case touches the GPU; importing this table does not.
GUARD_CASES = {
    "select_minimal": ("qsaeb_batch_select", _guard_select("gaussian", 1, 1, 1, False)),
    "select_odd_with_state": ("qsaeb_batch_select", _guard_select("eight_levels", 257, 33, 257 * 8, True)),
    "select_many_workgroups": ("qsaeb_batch_select", _guard_select("shared_high_bits", 1024, 256, 1024 * 64, True)),
    "threshold_minimal": ("qsaeb_threshold_select", _guard_threshold("gaussian", 1, 1, False)),
    "threshold_odd_on_device": ("qsaeb_threshold_select", _guard_threshold("special", 257, 33, True)),
    "decode_binary_minimal": ("qsaeb_decode_ragged_binary", _guard_decode("packed_D4_n1", "mixed")),
    "decode_binary_row_tail": ("qsaeb_decode_ragged_binary", _guard_decode("packed_D516_n4", "outside")),
    "decode_binary_long_list": ("qsaeb_decode_ragged_binary", _guard_decode("packed_D48_n4_K256", "mixed")),
    "decode_table_minimal": ("qsaeb_decode_ragged_table", _guard_decode("table_D4", "mixed")),
    "decode_table_row_tail": ("qsaeb_decode_ragged_table", _guard_decode("table_D516", "outside")),
    "decode_table_long_list": ("qsaeb_decode_ragged_table", _guard_decode("table_D48_K256", "all")),
    "row_grad_minimal": ("qsaeb_row_grad_ragged", _guard_row("table_D4", "mixed")),
    "row_grad_row_tail": ("qsaeb_row_grad_ragged", _guard_row("table_D516", "outside")),
    "row_grad_long_list": ("qsaeb_row_grad_ragged", _guard_row("table_D48_K256", "mixed")),
    "csr_small_dictionary": ("qsaeb_csr_ragged", _guard_csr("table_D48_s0.5_nobias_H8", "mixed")),
    "csr_clamped_counts": ("qsaeb_csr_ragged", _guard_csr("table_D516", "outside")),
    "csr_long_list": ("qsaeb_csr_ragged", _guard_csr("table_D48_K256", "all")),
}


@pytest.mark.parametrize("label", sorted(GUARD_CASES))
def test_entry_point_between_guard_words(label):
    entry, build = GUARD_CASES[label]
    call = build()
    assert call.entry == entry
    GU.run_call(call, _lib.load(), DEV)


# ---- the dispatcher ops ---------------------------------------------------------------------------------------------------
def test_dispatcher_ops():
    idx, val, decoder, bias, H = U.ragged_case("table_D48")
    B, K = idx.shape
    counts = dev(U.count_patterns(B, K)["mixed"])
    di, dv, dt = dev(idx), dev(val), dev(decoder[1])
    Q = torch.ops.qsae
    theta, batches = torch.zeros((), dtype=F32, device=DEV), torch.zeros((), dtype=I64, device=DEV)
    torch.library.opcheck(Q.batch_select.default, (dv, 3 * B, True, theta, batches, 0.01))
    torch.library.opcheck(Q.batch_select.default, (dv, 3 * B, False, None, None, 0.01))
    torch.library.opcheck(Q.threshold_select.default, (dv, theta, 0.0, True))
    torch.library.opcheck(Q.decode_ragged_table.default, (di, dv, counts, dt, 1.0, dev(bias)))
    torch.library.opcheck(Q.train_row_grad_ragged.default, (di, counts, dt, 0.5, dev(gaussian(1, B, 48)), None, dt, True))
    torch.library.opcheck(Q.train_csr_ragged.default, (di, counts, H))


# ---- the two top-k model classes ----------------------------------------------------------------------------------------
D_, H_, K_, CAP_, B_ = 64, 512, 8, 32, 64
CONFIG = {"input_dim": D_, "n_bits": 4, "hidden_dim": H_, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": K_,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": B_}
KIND = {"baseline_sae": "baseline", "b_sae": "binary"}
SEED = 11


def _state(kind: str, seed: int = SEED):
    if kind == "baseline":
        return S.baseline_sae_params(seed, D_, H_, bias_std=0.1)
    return S.binary_sae_params(seed, D_, H_, 4, dec_bias_std=0.1, logit_std=0.5)


def _model(kind: str, seed: int = SEED):
    if kind == "baseline":
        model = BaselineSparseAutoencoder(D_, H_)
        model.topk = K_
    else:
        model = BinarySAE(D_, H_, gamma=4.0, n_bits=4)
        model.k = (K_ + 0.5) / H_
        assert model.top_k == K_
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _state(kind, seed).items()})
    return model.to(DEV)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.fixture(scope="module")
def rows():
    return dev(S.activations(91, B_, D_))


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_with_cap_equal_to_k_it_is_forward_train(sae_type, rows):
    """n_select = B K: every entry is selected -- outputs and every .grad of forward_train, bit for bit"""
    model = _model(KIND[sae_type])
    x = rows.clone().requires_grad_()
    out = model.forward_train(x)
    trainer_loss(sae_type, out, rows, CONFIG)
    want, want_x = _grads(model), x.grad.clone()
    model.zero_grad(set_to_none=True)
    x.grad = None
    ctl = BatchTopK(model, cap=K_)
    got = model.forward_train_batch_topk(x, ctl)
    assert len(got) == len(out) and host(ctl.counts).tolist() == [K_] * B_ and host(ctl.report)[:3].tolist() == [B_ * K_, B_, 0]
    for g, w, what in zip(got, out, ("latent", "reconstruction", "polarize")):
        same(g, w, what)
    trainer_loss(sae_type, got, rows, CONFIG)
    for k, g in _grads(model).items():
        same(g, want[k], k)
    same(x.grad, want_x, "x.grad")


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_train_batch_topk_outputs_and_gradients(sae_type, rows):
    model = _model(KIND[sae_type])
    ctl = BatchTopK(model, cap=CAP_)
    assert (ctl.k, ctl.cap) == (K_, CAP_) == (K_, min(256, H_, 4 * K_))
    x = rows.clone().requires_grad_()
    latent, recon, *rest = model.forward_train_batch_topk(x, ctl)
    counts, report = ctl.counts, host(ctl.report)
    assert int(counts.sum()) == B_ * K_ == report[0] and len(set(host(counts).tolist())) > 1
    # the selection and the forward are the ops' composition, and forward_batch_topk's
    lin, dec = model.encoder.linear, model.decoder
    idx, val = model._select_cap(rows, CAP_, "test")
    wc, wv, wr = U.batch_select(host(val), B_ * K_)
    same(counts, wc, "counts")
    same(ctl.report, wr, "report")
    same(latent, ops.densify(idx, dev(wv), H_), "latent")
    m = np.array([report[3]], dtype=np.uint32).view(np.float32)[0]
    assert m > 0 and ctl.threshold() == float(m) and int(ctl.batches) == 1
    table, step, _ = model._nested_train_decoder()
    same(recon, ops.decode_ragged_table(idx, val, counts, table, step, dec.bias.detach()), "reconstruction")
    same(recon, U.decode_ragged(host(idx), host(val), wc, ("table", host(table), step), host(dec.bias)), "against the oracle")
    if sae_type == "baseline_sae":                           # forward_batch_topk decodes what forward() decodes from
        i2, v2, c2, r2 = model.forward_batch_topk(rows, ctl)
        same(i2, idx), same(v2, wv), same(c2, wc), same(r2, recon)
        assert ctl.threshold() == float(m) and int(ctl.batches) == 1          # not moved by the evaluation forward
    trainer_loss(sae_type, (latent, recon, *rest), rows, CONFIG)
    got = _grads(model)
    # bit for bit the composition of the ragged ops on the loss' own gradient
    coef = 0.5 if sae_type == "b_sae" else 1.0
    _, g_recon = ops.trainer_loss(rows, [recon.detach()], 0, coef)
    g_recon = g_recon[0]
    gv, dx = ops.train_row_grad_ragged(idx, counts, table, step, g_recon, None, lin.weight.detach(), True)
    off, ent = ops.train_csr_ragged(idx, counts, H_)
    g_pol = torch.full((), CONFIG["polarize_lambda"], dtype=F32, device=DEV) if sae_type == "b_sae" else None
    dW, db, ddec = model._batch_unit_grad(off, ent, dev(wv), gv, rows, g_recon, g_pol, True, True)
    same(got["encoder.0.weight"], dW, "dW_enc"), same(got["encoder.0.bias"], db, "db_enc"), same(got["decoder.weight"], ddec, "d decoder")
    same(got["decoder.bias"], ops.train_col_sum(g_recon), "db_dec"), same(x.grad, dx, "dx")
    wgv, wdx = U.row_grad_ragged(host(idx), wc, host(table), step, host(g_recon), None, host(lin.weight))
    same(gv, wgv, "gv against the restatement"), same(dx, wdx, "dx against the restatement")
    # ... and within the project's bound of fp64 autograd on the same selection
    W = lin.weight.detach().cpu().double().requires_grad_()
    b = lin.bias.detach().cpu().double().requires_grad_()
    dp = dec.weight.detach().cpu().double().requires_grad_()
    bd = dec.bias.detach().cpu().double().requires_grad_()
    x64, ii = rows.cpu().double().requires_grad_(), idx.cpu().long()
    if sae_type == "baseline_sae":
        t64, pol = dp.t(), 0.0
    else:
        bw = 2.0 ** torch.arange(4, dtype=torch.float64)
        pw = bw.clone()
        bw[-1] = -bw[-1]
        p = torch.sigmoid(dp).view(H_, D_, 4)
        t64, pol = (p * bw).sum(-1), CONFIG["polarize_lambda"] * (p * (1 - p) * pw).mean()
    keep = (torch.arange(CAP_)[None, :] < torch.from_numpy(wc.astype(np.int64))[:, None]).double()
    pre = (x64[:, None, :] * W[ii]).sum(-1) + b[ii]
    r64 = step * ((pre * keep)[:, :, None] * t64[ii]).sum(1) + bd
    (coef * ((r64 - x64.detach()) ** 2).mean() + pol).backward()
    want = {"encoder.0.weight": W.grad, "encoder.0.bias": b.grad, "decoder.weight": dp.grad, "decoder.bias": bd.grad}
    figures = {k: max_rel_err(got[k], want[k]) for k in want}
    # x64 also enters the loss as the target; only its path through the model is dx
    print(sae_type, figures)
    assert sorted(got) == sorted(want) and all(v <= TOL for v in figures.values()), figures


def test_without_a_saturated_row_it_is_uncapped_batch_topk(rows):
    """The CPU oracle's dense pre-activations: no row reaches the cap and the threshold value is unique, so the B k largest
    of the flattened [B, H] matrix are exactly the selected set."""
    sd = _state("baseline")
    pre = oracle.encode(host(rows), sd["encoder.0.weight"], sd["encoder.0.bias"])
    flat = torch.from_numpy(pre).reshape(-1)
    top = torch.topk(flat, B_ * K_ + 1)
    assert float(top.values[B_ * K_ - 1]) > float(top.values[B_ * K_])          # a unique threshold value
    chosen = np.zeros(B_ * H_, dtype=bool)
    chosen[top.indices[:B_ * K_].numpy()] = True
    chosen = chosen.reshape(B_, H_)
    assert chosen.sum(axis=1).max() < CAP_                    # no saturated row on the CPU
    model = _model("baseline")
    ctl = BatchTopK(model, cap=CAP_)
    idx, val_sel, counts, _ = model.forward_batch_topk(rows, ctl)
    assert int(ctl.report[1]) == 0                            # ... and none on the GPU
    got = np.zeros((B_, H_), dtype=bool)
    hi, hc = host(idx), host(counts)
    for r in range(B_):
        got[r, hi[r, :hc[r]]] = True
    assert np.array_equal(got, chosen)
    same(ops.densify(idx, val_sel, H_), np.where(chosen, pre, np.float32(0)).astype(np.float32), "the dense latent")


def test_activity_counts_only_selected_entries(rows):
    model = _model("baseline")
    model.activity = FeatureActivity.for_model(model)
    ctl = BatchTopK(model, cap=CAP_)
    model.forward_train_batch_topk(rows, ctl, dense_latent=False)
    idx, val = model._select_cap(rows, CAP_, "test")
    _, val_sel, _ = U.batch_select(host(val), B_ * K_)
    want = np.bincount(host(idx)[val_sel > 0], minlength=H_)
    assert np.array_equal(host(model.activity.fired), want) and want.sum() <= B_ * K_ < (host(val) > 0).sum()


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_threshold(sae_type, rows):
    model = _model(KIND[sae_type])
    ctl = BatchTopK(model, cap=CAP_)
    model.forward_train_batch_topk(rows, ctl, dense_latent=False)
    theta = ctl.threshold()
    assert theta > 0
    idx, val_sel, counts, recon = model.forward_threshold(rows, ctl)
    i2, v2, c2, r2 = model.forward_threshold(rows, theta, cap=CAP_)
    same(idx, i2), same(val_sel, v2), same(counts, c2), same(recon, r2)
    _, val = model._select_cap(rows, CAP_, "test")
    wc, wv, wr = U.threshold_select(host(val), np.float32(theta))
    same(counts, wc), same(val_sel, wv), same(ctl.report, wr)
    assert int(counts.sum()) == B_ * K_                       # the batch the threshold came from: its own selection
    decoder, bias = model._nested_decoder()
    hd = (decoder[0], host(decoder[1])) + ((D_,) if decoder[0] == "packed" else ()) + tuple(decoder[2:])
    same(recon, U.decode_ragged(host(idx), host(val), wc, hd, host(bias)), "decoded from what forward() decodes from")
    with pytest.raises(ValueError, match="cap"):
        model.forward_threshold(rows, 0.5, cap=257)
    with pytest.raises(ValueError, match="expected \\[batch"):
        model.forward_threshold(rows[:, :8], ctl)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_three_steps_through_the_trainer(sae_type, rows, tmp_path):
    logs = []
    model = _model(KIND[sae_type])
    if sae_type == "baseline_sae":
        model.normalize_decoder_weights()
    t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path), log_fn=logs.append,
                log_every=1, batch_topk=True, batch_topk_cap=CAP_, activity_window=B_, aux_k=4)
    assert (t.batch_topk.k, t.batch_topk.cap) == (K_, CAP_)
    for _ in range(3):                                        # one batch per call: the chunk is one batch of B_ rows
        t.one_epoch(rows)
    assert [len(b) for b in t.trained_batches] == [1, 1, 1] and int(t.batch_topk.batches) == 3
    key = "recon_loss" if sae_type == "b_sae" else "loss"
    print(sae_type, [m[key] for m in logs], [m["batch_topk/threshold"] for m in logs])
    assert logs[2][key] < logs[0][key]
    assert all(m["batch_topk/threshold"] > 0 and m["batch_topk/saturated_rows"] == 0 and m["batch_topk/empty_rows"] >= 0
               for m in logs) and "aux_loss" in logs[0] and "dead_features" in logs[0]
    assert logs[2]["batch_topk/threshold"] == t.batch_topk.threshold()
    sd = t.batch_topk.state_dict()
    other = BatchTopK(model, cap=CAP_)
    other.load_state_dict(sd)
    assert other.threshold() == t.batch_topk.threshold() and int(other.batches) == 3
    with pytest.raises(ValueError, match="nested"):
        Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path), batch_topk=True,
                nested_bounds="default")
    default = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path))
    assert default.batch_topk is None
