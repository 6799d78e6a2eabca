"""The nested levels over ragged rows on the GPU (csrc/nested_ragged.hip, include/qsae_nested_batch.h): the decode and its
per-level counts bit for bit against the numpy restatement of tests/nested_ragged_util.py and anchored to the existing ops (the
last level is decode_ragged_*, full prefixes give decode_nested_*, one level gives decode_ragged_*); the row gradient bit for bit
against the restatement, train_row_grad_nested and train_row_grad_ragged; the existing nested unit sums over the ragged lists
against the composition of the plain ops and fp64; special values behind a prefix and behind a bound; all three entry points
between guard words; the two top-k model classes (forward_nested_batch_topk, forward_nested_threshold,
forward_train_nested_batch_topk), the Trainer's ``batch_topk_nested_bounds``, ``nested_errors(threshold=)`` and the dispatcher
ops."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard_util as GU  # noqa: E402
import nested_ragged_util as R  # noqa: E402
import nested_util as N  # noqa: E402
from batch_topk_util import batch_select, clamp_counts, threshold_select  # noqa: E402
from guard_util import STREAM, Buf, Call, HostArray, HostPointers  # noqa: E402
from sparsity_curve_util import gaussian, packed_dictionary  # noqa: E402
from train_util import max_rel_err  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.inference import DatasetMoments, nested_errors  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import BatchTopK, Trainer, nested_loss, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, F32 = torch.int32, torch.float32
TOL = 1e-5                                                   # the project's bound on a gradient against fp64 (max_rel_err)
H = R.H


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


def _dev_decoder(decoder):
    return (decoder[0], dev(decoder[1])) + tuple(decoder[2:])


def decode(mod, idx, val, counts, dd, bias, bounds):
    if dd[0] == "packed":
        return mod.decode_nested_ragged_binary(idx, val, counts, dd[1], dd[2], dd[3], dd[4], bias, bounds)
    return mod.decode_nested_ragged_table(idx, val, counts, dd[1], dd[2], bias, bounds)


def decode_ragged(idx, val, counts, dd, bias):
    if dd[0] == "packed":
        return ops.decode_ragged_binary(idx, val, counts, dd[1], dd[2], dd[3], dd[4], bias)
    return ops.decode_ragged_table(idx, val, counts, dd[1], dd[2], bias)


def decode_nested(idx, val, dd, bias, bounds):
    if dd[0] == "packed":
        return ops.decode_nested_binary(idx, val, dd[1], dd[2], dd[3], dd[4], bias, bounds)
    return ops.decode_nested_table(idx, val, dd[1], dd[2], bias, bounds)


# ---- 1, 2: the decode and its counts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_decode_equals_the_restatement_and_the_existing_ops(name):
    idx, val, bounds, decoder, bias = R.build_case(name)
    B, K = idx.shape
    dd, di, dv, db = _dev_decoder(decoder), dev(idx), dev(val), None if bias is None else dev(bias)
    anchored = 0                                             # rows compared with the ragged decode, over all patterns
    for pattern, counts in R.patterns(B, K).items():
        dc, c = dev(counts), clamp_counts(counts, K)
        want = R.nested_recons(idx, val, counts, bounds, decoder, bias)
        below = R.counts_below(idx, counts, bounds, H)
        for mod in (ops, torch_ops):
            got, got_below = decode(mod, di, dv, dc, dd, db, bounds)
            same(got, want, f"{pattern}: levels ({mod.__name__})")
            same(got_below, below, f"{pattern}: counts_below ({mod.__name__})")
        # (a) the last level is the ragged decode, on the rows whose prefix ids lie in the dictionary (it clamps, this drops)
        inside = np.array([((idx[r, :c[r]] >= 0) & (idx[r, :c[r]] < H)).all() for r in range(B)])
        rows = dev(np.nonzero(inside)[0])
        anchored += int(inside.sum())
        assert torch.equal(got[-1][rows], decode_ragged(di, dv, dc, dd, db)[rows]), pattern
        # (b) full prefixes: every level is the nested decode at k = K
        if pattern == "all":
            assert torch.equal(got, decode_nested(di, dv, dd, db, bounds))
        # (c) one level over the whole dictionary is the ragged decode
        one, one_below = decode(ops, di, dv, dc, dd, db, [H])
        assert torch.equal(one[0][rows], decode_ragged(di, dv, dc, dd, db)[rows]) and torch.equal(one[0], got[-1])
        assert torch.equal(one_below[0], got_below[-1])
    assert anchored >= B


def test_front_end_validation():
    idx, val, bounds, decoder, bias = R.build_case("table_D48")
    di, dv, table, dc = dev(idx), dev(val), dev(decoder[1]), dev(R.patterns(9, 12)["mixed"])
    for bad in ([], [0, 512], [64, 64, 512], [64, 33, 512], [1, 33, 64], [1, 33, 64, 513], list(range(1, 9)) + [512], [1.5, 512]):
        with pytest.raises(ValueError, match="bounds|levels"):
            ops.decode_nested_ragged_table(di, dv, dc, table, 1.0, None, bad)
        with pytest.raises(ValueError, match="bounds|levels"):
            ops.train_row_grad_nested_ragged(di, dc, table, 1.0, [None] * len(bad), bad, None, None)
    with pytest.raises(ValueError, match="idx is"):
        ops.decode_nested_ragged_table(di, dv[:, :3], dc, table, 1.0, None, bounds)
    with pytest.raises(ValueError, match="counts is"):
        ops.decode_nested_ragged_table(di, dv, dc[:4], table, 1.0, None, bounds)
    with pytest.raises(ValueError, match="bias"):
        ops.decode_nested_ragged_table(di, dv, dc, table, 1.0, dev(bias)[:4], bounds)
    with pytest.raises(ValueError, match="level gradients"):
        ops.train_row_grad_nested_ragged(di, dc, table, 1.0, [None], bounds, None, None)
    levels, below = ops.decode_nested_ragged_table(di[:0], dv[:0], dc[:0], table, 1.0, None, bounds)      # no rows: nothing happens
    assert levels.shape == (4, 0, 48) and below.shape == (4, 0)


# ---- 3: the row gradient --------------------------------------------------------------------------------------------------
ROW_CASES = ["table_D4", "table_D48", "table_D516", "table_D48_K256", "table_D520_s0.5_nobias_B5_K65", "table_D516_s0.5_B5_K7",
             "table_D48_B1_K1_eight_levels", "table_D4_s0.5_B5_K7_one_level"]


class RowCase:
    def __init__(self, name: str):
        idx, val, bounds, decoder, _ = R.build_case(name)
        self.idx, self.val, self.bounds, self.table = idx, val, bounds, decoder[1]
        self.B, self.K = idx.shape
        self.D = self.table.shape[1]
        seed = 9000 + sorted(R.CASES).index(name)
        self.g = [gaussian(seed + l, self.B, self.D) for l in range(len(bounds))]
        self.gl, self.W = gaussian(seed + 10, self.B, H), gaussian(seed + 11, H, self.D)
        self.di, self.dt, self.dg, self.dgl, self.dW = dev(idx), dev(self.table), [dev(t) for t in self.g], dev(self.gl), dev(self.W)

    def run(self, counts, present=None, mod=ops, bounds=None, use_gl=True, want_dx=True):
        bounds = self.bounds if bounds is None else bounds
        g = [t if (present is None or present[l]) else None for l, t in enumerate(self.dg[:len(bounds)])]
        return mod.train_row_grad_nested_ragged(self.di, dev(counts), self.dt, 0.25, g, bounds, self.dgl if use_gl else None,
                                                self.dW, want_dx=want_dx)


@pytest.mark.parametrize("name", ROW_CASES)
def test_row_gradient(name):
    c = RowCase(name)
    L = len(c.bounds)
    full, fgv, _ = ops.train_row_grad_nested(c.di, c.dt, 0.25, c.dg, c.bounds, c.dgl, c.dW, want_dx=False)     # at width K
    for pattern, counts in R.patterns(c.B, c.K).items():
        n = clamp_counts(counts, c.K)
        behind = dev(np.arange(c.K)[None, :] >= n[:, None])
        for mod in (ops, torch_ops):
            G, gv, dx = c.run(counts, mod=mod)
            same(G, full, f"{pattern}: G is train_row_grad_nested's, whatever the counts are")
            assert torch.equal(gv[~behind], fgv[~behind]), f"{pattern}: gv inside the prefixes"
            assert not host(gv[behind]).view(np.uint32).any(), f"{pattern}: +0 behind the prefixes"
        if c.K <= 64 or pattern == "around_64":              # the long lists once: the restatement walks them on the host
            wG, wgv, wdx = R.row_grad(c.idx, counts, c.table, 0.25, c.g, c.bounds, c.gl, c.W)
            same(G, wG, f"{pattern}: G"), same(gv, wgv, f"{pattern}: gv"), same(dx, wdx, f"{pattern}: dx")
        if pattern == "all":                                  # full prefixes: train_row_grad_nested, dx included
            for got, want in zip((G, gv, dx), ops.train_row_grad_nested(c.di, c.dt, 0.25, c.dg, c.bounds, c.dgl, c.dW, want_dx=True)):
                same(got, want, "all")
        # one level: train_row_grad_ragged with g_recon = g[0]
        G1, gv1, dx1 = c.run(counts, bounds=[H])
        rgv, rdx = ops.train_row_grad_ragged(c.di, dev(counts), c.dt, 0.25, c.dg[0], c.dgl, c.dW, want_dx=True)
        same(G1[0], c.dg[0], "one level: G"), same(gv1, rgv, "one level: gv"), same(dx1, rdx, "one level: dx")
        # without a latent gradient, without dx
        G2, gv2, dx2 = c.run(counts, use_gl=False, want_dx=False)
        assert dx2 is None and torch.equal(G2, G)
        assert torch.equal(gv2[~behind], ops.train_row_grad_nested(c.di, c.dt, 0.25, c.dg, c.bounds, None, None)[1][~behind])
    if L == 4:
        counts = R.patterns(c.B, c.K)["mixed"]
        for present in ((1, 0, 1, 0), (0, 1, 1, 1), (0, 0, 0, 0)):                            # an absent level is skipped
            G, gv, dx = c.run(counts, present=present)
            g = [t if p else None for t, p in zip(c.g, present)]
            same(G, N.suffix_sums(g, c.B, c.D), f"{present}: G")
            if c.K <= 64:
                _, wgv, wdx = R.row_grad(c.idx, counts, c.table, 0.25, g, c.bounds, c.gl, c.W)
                same(gv, wgv, f"{present}: gv"), same(dx, wdx, f"{present}: dx")


# ---- 4: the existing nested unit sums over the ragged lists -----------------------------------------------------------------
class UnitCase:
    """The operands of one backward at the op level over ragged lists: what tests/test_nested_gpu.py::TrainCase holds, with
    counts, val_sel and the ragged lists; ``levels`` and ``unit_levels`` as check_composition reads them."""

    def __init__(self, name: str, pattern: str, n_bits: int = 4, gamma: float = 4.0):
        idx, val, bounds, _, _ = R.build_case(name)
        self.B, self.K = idx.shape
        _, self.D = R.CASES[name][:2]
        counts = R.patterns(self.B, self.K)[pattern]
        c = clamp_counts(counts, self.K)
        seed = 9500 + sorted(R.CASES).index(name)
        self.n_bits, self.bounds, self.step = n_bits, bounds, gamma / 2 ** (n_bits - 1)
        self.sel = np.arange(self.K)[None, :] < c[:, None]
        self.h_idx, self.h_val = idx, np.where(self.sel, val, np.float32(0)).astype(np.float32)
        self.idx, self.val, self.counts = dev(idx), dev(self.h_val), dev(counts)
        self.x, self.W = dev(gaussian(seed, self.B, self.D)), dev(gaussian(seed + 1, H, self.D))
        self.logits = dev(gaussian(seed + 2, H, self.D * n_bits))
        self.table = ops.binary_soft_table(self.logits, self.D, n_bits)
        self.g = [dev(gaussian(seed + 10 + l, self.B, self.D) * np.float32(1.0 / (self.B * self.D))) for l in range(len(bounds))]
        self.g_latent = dev(gaussian(seed + 3, self.B, H) * np.float32(1e-3))
        self.g_pol = torch.tensor(1e-2, dtype=F32, device=DEV)
        self.offsets, self.entries = ops.train_csr_ragged(self.idx, self.counts, H)
        self.unit_levels = dev(N.levels_of(np.arange(H), bounds))

    def nested(self, mod=ops):
        G, gv, dx = mod.train_row_grad_nested_ragged(self.idx, self.counts, self.table, self.step, self.g, self.bounds,
                                                     self.g_latent, self.W, want_dx=True)
        dW, db, dl = mod.train_unit_grad_nested(self.offsets, self.entries, self.val, gv, self.x, G, self.bounds, self.logits,
                                                self.n_bits, self.step, self.g_pol)
        tW, tb, tWd = mod.train_table_unit_grad_nested(self.offsets, self.entries, self.val, gv, self.x, G, self.bounds)
        return dict(G=G, gv=gv, dx=dx, dW=dW, db=db, dl=dl, tW=tW, tb=tb, tWd=tWd)


@pytest.mark.parametrize("name,pattern,n_bits", [("table_D48", "mixed", 4), ("table_D48", "outside", 8), ("table_D516", "mixed", 1),
                                                 ("table_D48_K256", "around_64", 4), ("table_D4", "none", 4),
                                                 ("table_D520_s0.5_nobias_B5_K65", "mixed", 4)])
def test_unit_sums_over_ragged_lists(name, pattern, n_bits):
    """The existing nested unit-gradient ops on the lists of train_csr_ragged never reach an entry behind a prefix: they are
    the composition of the plain unit-gradient ops, once per level with g_recon = G[level] and restricted to that level's units
    (check_composition of tests/test_nested_gpu.py, rebuilt on the ragged lists), and within TOL of fp64 over the prefixes."""
    c = UnitCase(name, pattern, n_bits)
    n = c.nested()
    G = n["G"]
    want = {k: torch.full_like(n[k], float("nan")) for k in ("dW", "db", "dl", "tW", "tb", "tWd")}
    for l in range(len(c.bounds)):
        mine = c.unit_levels == l
        dW, db, dl = ops.train_unit_grad(c.offsets, c.entries, c.val, n["gv"], c.x, G[l], c.logits, c.n_bits, c.step, c.g_pol)
        tW, tb, tWd = ops.train_table_unit_grad(c.offsets, c.entries, c.val, n["gv"], c.x, G[l])
        for key, t in (("dW", dW), ("db", db), ("dl", dl), ("tW", tW), ("tb", tb)):
            want[key][mine] = t[mine]
        want["tWd"][:, mine] = tWd[:, mine]
    for key, t in want.items():
        same(n[key], t, key)
    again = c.nested(torch_ops)
    for key in n:                                            # the other front end, and a second run: the same bits
        same(again[key], n[key], key)
    # fp64 over the entries the lists hold: in a prefix, id inside the dictionary
    keep = c.sel & (c.h_idx >= 0) & (c.h_idx < H)
    hh = np.clip(c.h_idx, 0, H - 1)
    lev = np.minimum(N.levels_of(hh, c.bounds), len(c.bounds) - 1)
    G64 = torch.from_numpy(N.suffix_sums([host(t) for t in c.g], c.B, c.D)).double()
    T, x64 = host(c.table).astype(np.float64), host(c.x).astype(np.float64)
    gv64 = np.zeros((c.B, c.K))
    dWe, dbe, rows = np.zeros((H, c.D)), np.zeros(H), np.zeros((H, c.D))
    for r, j in zip(*np.nonzero(c.sel)):
        h, Gr = hh[r, j], G64[lev[r, j], r].numpy()
        gv64[r, j] = float(host(c.g_latent)[r, h]) + c.step * float(Gr @ T[h])
        if keep[r, j]:
            dWe[h] += gv64[r, j] * x64[r]
            dbe[h] += gv64[r, j]
            rows[h] += float(c.h_val[r, j]) * Gr
    dl64 = N.logit_grads64(torch.from_numpy(rows), host(c.logits), c.D, c.n_bits, c.step, float(c.g_pol))
    figures = {"gv": max_rel_err(n["gv"], torch.from_numpy(gv64)) if c.sel.any() else 0.0,
               "dlogits": max_rel_err(n["dl"], dl64)}
    if keep.any():
        figures.update({"dW_enc": max_rel_err(n["dW"], torch.from_numpy(dWe)), "db_enc": max_rel_err(n["db"], torch.from_numpy(dbe)),
                        "tW_enc": max_rel_err(n["tW"], torch.from_numpy(dWe)), "dW_dec": max_rel_err(n["tWd"], torch.from_numpy(rows).t())})
    else:
        assert not any(host(n[k]).view(np.uint32).any() for k in ("dW", "db", "tW", "tb", "tWd"))
    print(name, pattern, figures)
    assert all(v <= TOL for v in figures.values()), figures


# ---- 5: special values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SPECIAL_CASES))
def test_special_values_do_not_show(name):
    idx, val, counts, bounds, decoder, bias, check = R.special_case(name)
    got, below = ops.decode_nested_ragged_table(dev(idx), dev(val), dev(counts), dev(decoder[1]), decoder[2],
                                                None if bias is None else dev(bias), bounds)
    same(got, R.nested_recons(idx, val, counts, bounds, decoder, bias), "levels")
    same(below, R.counts_below(idx, counts, bounds, decoder[1].shape[0]), "counts_below")
    check(host(got))
    if name == "behind_a_prefix":                             # ... nor in the row gradient
        B, D = idx.shape[0], decoder[1].shape[1]
        g = [dev(gaussian(7 + l, B, D)) for l in range(3)]
        G, gv, dx = ops.train_row_grad_nested_ragged(dev(idx), dev(counts), dev(decoder[1]), 0.5, g, bounds, None, dev(decoder[1]), True)
        c = clamp_counts(counts, idx.shape[1])
        assert bool(torch.isfinite(gv).all()) and bool(torch.isfinite(dx).all())
        assert not host(gv)[np.arange(idx.shape[1])[None, :] >= c[:, None]].view(np.uint32).any()


# ---- 6: all three entry points between guard words -----------------------------------------------------------------------------
def _minimal():
    """B = 1, K = 1, D = 4, H = 1, bounds = [1]"""
    return (np.zeros((1, 1), np.int32), np.array([[1.5]], np.float32), [1], gaussian(1, 1, 4), gaussian(2, 1, 4)[0])


def _guard_decode(name, packed_bits=None):
    def build():
        if name == "minimal":
            idx, val, bounds, table, bias = _minimal()
            decoder = ("table", table, 0.5) if packed_bits is None else \
                ("packed", packed_dictionary(6, 1, 4, packed_bits), 4, packed_bits, 0.25)
        else:
            idx, val, bounds, decoder, bias = R.build_case(name)
        B, K = idx.shape
        counts = R.patterns(B, K)["outside"]
        Hc, L = decoder[1].shape[0], len(bounds)
        packed = decoder[0] == "packed"
        D = decoder[2] if packed else decoder[1].shape[1]
        want = R.nested_recons(idx, val, counts, bounds, decoder, bias)
        below = R.counts_below(idx, counts, bounds, Hc)

        def front(t):
            dd = (decoder[0], t["dict"]) + tuple(decoder[2:])
            recon, cb = decode(ops, t["idx"], t["val"], t["counts"], dd, t.get("bias"), bounds)
            return {"recon": recon, "below": cb}
        dict_args = [Buf("dict", "in", dev(decoder[1])), Hc, D] + ([decoder[3], decoder[4]] if packed else [decoder[2]])
        entry = "qsaem_decode_nested_ragged_binary" if packed else "qsaem_decode_nested_ragged_table"
        return Call(name, entry,
                    [Buf("idx", "in", dev(idx)), Buf("val", "in", dev(val)), Buf("counts", "in", dev(counts)), B, K, *dict_args,
                     Buf("bias", "in", dev(bias)) if bias is not None else None, HostArray(bounds), L,
                     Buf("recon", "out", shape=(L, B, D), dtype=F32), Buf("below", "out", shape=(L, B), dtype=I32), STREAM],
                    front, expect={"recon": torch.from_numpy(want), "below": torch.from_numpy(below)})
    return build


def _guard_row(name, absent=()):
    def build():
        if name == "minimal":
            idx, _, bounds, table, _ = _minimal()
            B, K, D, Hc = 1, 1, 4, 1
            g, gl, W = [gaussian(3, 1, 4)], gaussian(4, 1, 1), gaussian(5, 1, 4)
        else:
            c = RowCase(name)
            idx, bounds, table, B, K, D, Hc, g, gl, W = c.idx, c.bounds, c.table, c.B, c.K, c.D, H, c.g, c.gl, c.W
        counts = R.patterns(B, K)["outside"]
        L = len(bounds)
        gbufs = [None if l in absent else Buf(f"g{l}", "in", dev(g[l])) for l in range(L)]
        wG, wgv, wdx = R.row_grad(idx, counts, table, 0.25, [None if l in absent else g[l] for l in range(L)], bounds, gl, W) \
            if K <= 64 else (None, None, None)

        def front(t):
            gs = [t.get(f"g{l}") for l in range(L)]
            G, gv, dx = ops.train_row_grad_nested_ragged(t["idx"], t["counts"], t["table"], 0.25, gs, bounds, t["g_latent"], t["W"],
                                                         want_dx=True)
            return {"G": G, "gv": gv, "dx": dx}
        expect = None if wG is None else {"G": torch.from_numpy(wG), "gv": torch.from_numpy(wgv), "dx": torch.from_numpy(wdx)}
        return Call(name, "qsaem_row_grad_nested_ragged",
                    [Buf("idx", "in", dev(idx)), Buf("counts", "in", dev(counts)), B, K, Buf("table", "in", dev(table)), Hc, D, 0.25,
                     HostPointers(gbufs), HostArray(bounds), L, Buf("g_latent", "in", dev(gl)), Hc, Buf("W", "in", dev(W)),
                     Buf("G", "out", shape=(L, B, D), dtype=F32), Buf("gv", "out", shape=(B, K), dtype=F32),
                     Buf("dx", "out", shape=(B, D), dtype=F32), STREAM], front, expect=expect)
    return build


#: label -> (entry point, builder of its guard_util.Call); tests/test_nested_ragged_host.py reads the entry points for its
#: ledger.  Building a case touches the GPU; importing this table does not.  Every case runs with the counts pattern "outside".
GUARD_CASES = {
    "decode_binary_minimal": ("qsaem_decode_nested_ragged_binary", _guard_decode("minimal", packed_bits=4)),
    "decode_binary_row_tail": ("qsaem_decode_nested_ragged_binary", _guard_decode("packed_D516_n1_B5_K65_eight_levels")),
    "decode_binary_long_list": ("qsaem_decode_nested_ragged_binary", _guard_decode("packed_D48_n4_K256")),
    "decode_table_minimal": ("qsaem_decode_nested_ragged_table", _guard_decode("minimal")),
    "decode_table_row_tail": ("qsaem_decode_nested_ragged_table", _guard_decode("table_D516_s0.5_B5_K7")),
    "decode_table_long_list": ("qsaem_decode_nested_ragged_table", _guard_decode("table_D48_K256")),
    "row_grad_minimal": ("qsaem_row_grad_nested_ragged", _guard_row("minimal")),
    "row_grad_row_tail_absent_levels": ("qsaem_row_grad_nested_ragged", _guard_row("table_D516_s0.5_B5_K7", absent=(1, 3))),
    "row_grad_long_list": ("qsaem_row_grad_nested_ragged", _guard_row("table_D48_K256")),
}


@pytest.mark.parametrize("label", sorted(GUARD_CASES))
def test_entry_point_between_guard_words(label):
    entry, build = GUARD_CASES[label]
    call = build()
    assert call.entry == entry
    GU.run_call(call, _lib.load(), DEV)


# ---- 10: the dispatcher ops -----------------------------------------------------------------------------------------------------
def test_dispatcher_ops():
    c = RowCase("table_D48")
    counts = dev(R.patterns(c.B, c.K)["mixed"])
    Q = torch.ops.qsae
    dv, bias = dev(c.val), dev(gaussian(5, 1, c.D)[0])
    torch.library.opcheck(Q.decode_nested_ragged_table.default, (c.di, dv, counts, c.dt, 0.5, bias, c.bounds))
    idx, val, bounds, decoder, pb = R.build_case("packed_D48_n4")
    torch.library.opcheck(Q.decode_nested_ragged_binary.default, (dev(idx), dev(val), counts, dev(decoder[1]), 48, 4, 0.25, None, bounds))
    g = [c.dg[0], None, c.dg[2], c.dg[3]]
    torch.library.opcheck(Q.train_row_grad_nested_ragged.default, (c.di, counts, c.dt, 0.5, g, c.bounds, c.dgl, c.dW, True))
    torch.library.opcheck(Q.train_row_grad_nested_ragged.default, (c.di, counts, c.dt, 0.5, g, c.bounds, None, None, False))
    for got, want in zip(torch_ops.decode_nested_ragged_table(c.di, dv, counts, c.dt, 0.5, bias, c.bounds),
                         ops.decode_nested_ragged_table(c.di, dv, counts, c.dt, 0.5, bias, c.bounds)):
        same(got, want)
    for got, want in zip(torch_ops.train_row_grad_nested_ragged(c.di, counts, c.dt, 0.5, g, c.bounds, c.dgl, c.dW, True),
                         ops.train_row_grad_nested_ragged(c.di, counts, c.dt, 0.5, g, c.bounds, c.dgl, c.dW, True)):
        same(got, want)


# ---- 7: the two top-k model classes -----------------------------------------------------------------------------------------
D_, H_, K_, CAP_, B_ = 64, 512, 8, 32, 40
M_BOUNDS = [64, 128, 256, 512]
CONFIG = {"input_dim": D_, "n_bits": 4, "hidden_dim": H_, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": K_,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": B_}
KIND = {"baseline_sae": "baseline", "b_sae": "binary"}


def _model(kind: str, seed: int = 11):
    if kind == "baseline":
        sd = S.baseline_sae_params(seed, D_, H_, bias_std=0.1)
        model = BaselineSparseAutoencoder(D_, H_)
        model.topk = K_
    else:
        sd = S.binary_sae_params(seed, D_, H_, 4, dec_bias_std=0.1, logit_std=0.5)
        model = BinarySAE(D_, H_, gamma=4.0, n_bits=4)
        model.k = (K_ + 0.5) / H_
        assert model.top_k == K_
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(DEV)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.fixture(scope="module")
def rows():
    return dev(S.activations(91, B_, D_))


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_with_cap_equal_to_k_it_is_forward_train_nested(sae_type, rows):
    """n_select = B K: every entry is selected -- outputs and every .grad of forward_train_nested, bit for bit"""
    model = _model(KIND[sae_type])
    x = rows.clone().requires_grad_()
    out = model.forward_train_nested(x, M_BOUNDS)
    nested_loss(sae_type, out, rows, CONFIG)
    want, want_x = _grads(model), x.grad.clone()
    model.zero_grad(set_to_none=True)
    x.grad = None
    ctl = BatchTopK(model, cap=K_)
    got = model.forward_train_nested_batch_topk(x, ctl, M_BOUNDS)
    assert len(got) == len(out) and isinstance(got[1], tuple) and len(got[1]) == 4
    assert host(ctl.counts).tolist() == [K_] * B_ and host(ctl.level_counts[-1]).tolist() == [K_] * B_
    same(got[0], out[0], "latent")
    for l in range(4):
        same(got[1][l], out[1][l], f"level {l}")
    if sae_type == "b_sae":
        same(got[2], out[2], "polarize")
    nested_loss(sae_type, got, rows, CONFIG)
    for k, g in _grads(model).items():
        same(g, want[k], k)
    same(x.grad, want_x, "x.grad")


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_with_one_level_it_is_forward_train_batch_topk(sae_type, rows):
    model = _model(KIND[sae_type])
    x = rows.clone().requires_grad_()
    out = model.forward_train_batch_topk(x, BatchTopK(model, cap=CAP_))
    trainer_loss(sae_type, out, rows, CONFIG)
    want, want_x = _grads(model), x.grad.clone()
    model.zero_grad(set_to_none=True)
    x.grad = None
    ctl = BatchTopK(model, cap=CAP_)
    got = model.forward_train_nested_batch_topk(x, ctl, [H_])
    assert len(got) == len(out) and len(got[1]) == 1 and len(set(host(ctl.counts).tolist())) > 1
    same(got[0], out[0], "latent"), same(got[1][0], out[1], "reconstruction")
    if sae_type == "b_sae":
        same(got[2], out[2], "polarize")
    nested_loss(sae_type, got, rows, CONFIG)
    for k, g in _grads(model).items():
        same(g, want[k], k)
    same(x.grad, want_x, "x.grad")


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_train_nested_batch_topk_levels_and_gradients(sae_type, rows):
    model = _model(KIND[sae_type])
    calls = []

    class Spy:
        def add_compact(self, idx, val):
            calls.append((tuple(idx.shape), int((val > 0).sum())))
    model.activity = Spy()
    ctl = BatchTopK(model, cap=CAP_)
    assert (ctl.k, ctl.cap) == (K_, CAP_) == (K_, 4 * K_)
    latent, levels, *rest = model.forward_train_nested_batch_topk(rows, ctl, M_BOUNDS, dense_latent=False)
    assert latent is None and len(levels) == 4 and levels[0]._base is levels[3]._base
    assert int(ctl.batches) == 1 and ctl.threshold() > 0     # the threshold state is moved once
    idx, val = model._select_cap(rows, CAP_, "test")
    wc, wv, wr = batch_select(host(val), B_ * K_)
    same(ctl.counts, wc, "counts"), same(ctl.report, wr, "report")
    assert calls == [((B_, CAP_), int((wv > 0).sum()))]       # the tracker is fed once, with the selected entries
    saved = levels[0]._base.grad_fn.saved_tensors
    assert sorted(tuple(t.shape) for t in saved) == sorted([(B_, D_), (B_, CAP_), (B_, CAP_), (B_,), (H_, D_)])
    table, step, _ = model._nested_train_decoder()
    dec = model.decoder
    want = R.nested_recons(host(idx), host(val), wc, M_BOUNDS, ("table", host(table), step), host(dec.bias))
    same(levels[0]._base, want, "levels against the restatement")
    same(ctl.level_counts, R.counts_below(host(idx), wc, M_BOUNDS, H_), "level_counts")
    assert int(ctl.level_counts[-1].sum()) == B_ * K_
    # the evaluation forward decodes what forward() decodes from and moves no state
    model.activity = None
    i2, v2, c2, l2 = model.forward_nested_batch_topk(rows, ctl, M_BOUNDS)
    same(i2, idx), same(v2, wv), same(c2, wc)
    decoder, bias = model._nested_decoder()
    hd = (decoder[0], host(decoder[1])) + ((D_,) if decoder[0] == "packed" else ()) + tuple(decoder[2:])
    same(l2, R.nested_recons(host(idx), host(val), wc, M_BOUNDS, hd, host(bias)), "forward_nested_batch_topk")
    same(l2[-1], model.forward_batch_topk(rows, ctl)[3], "its last level is forward_batch_topk's reconstruction")
    assert int(ctl.batches) == 1
    # the gradient of the summed loss against fp64 autograd on the same selection
    losses = nested_loss(sae_type, (latent, levels, *rest), rows, CONFIG)
    assert losses.shape == (4,)
    got = _grads(model)
    lin = model.encoder.linear
    W = lin.weight.detach().cpu().double().requires_grad_()
    b = lin.bias.detach().cpu().double().requires_grad_()
    dp = dec.weight.detach().cpu().double().requires_grad_()
    bd = dec.bias.detach().cpu().double().requires_grad_()
    x64, ii = rows.cpu().double(), idx.cpu().long()
    if sae_type == "baseline_sae":
        t64, coef, pol = dp.t(), 1.0, 0.0
    else:
        bw = 2.0 ** torch.arange(4, dtype=torch.float64)
        pw = bw.clone()
        bw[-1] = -bw[-1]
        p = torch.sigmoid(dp).view(H_, D_, 4)
        t64, coef, pol = (p * bw).sum(-1), 0.5, CONFIG["polarize_lambda"] * (p * (1 - p) * pw).mean()
    prefix = (torch.arange(CAP_)[None, :] < torch.from_numpy(wc.astype(np.int64))[:, None])
    pre = (x64[:, None, :] * W[ii]).sum(-1) + b[ii]
    total = pol
    for l, bound in enumerate(M_BOUNDS):
        keep = (prefix & (ii < bound)).double()
        r64 = step * ((pre * keep)[:, :, None] * t64[ii]).sum(1) + bd
        level_loss = coef * ((r64 - x64) ** 2).mean()
        assert abs(float(losses[l]) - level_loss.item()) <= TOL * level_loss.item()
        total = total + level_loss
    total.backward()
    want = {"encoder.0.weight": W.grad, "encoder.0.bias": b.grad, "decoder.weight": dp.grad, "decoder.bias": bd.grad}
    figures = {k: max_rel_err(got[k], want[k]) for k in want}
    print(sae_type, figures)
    assert sorted(got) == sorted(want) and all(v <= TOL for v in figures.values()), figures
    for bad in ([], [64, 64, 512], [64, 256], [0, 512]):
        with pytest.raises(ValueError, match="bounds|levels"):
            model.forward_train_nested_batch_topk(rows, ctl, bad)
    with pytest.raises(ValueError, match="expected \\[batch"):
        model.forward_nested_batch_topk(rows[:, :8], ctl, M_BOUNDS)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_nested_threshold(sae_type, rows):
    model = _model(KIND[sae_type])
    ctl = BatchTopK(model, cap=CAP_)
    model.forward_train_nested_batch_topk(rows, ctl, M_BOUNDS, dense_latent=False)
    theta = ctl.threshold()
    idx, val_sel, counts, levels = model.forward_nested_threshold(rows, ctl, M_BOUNDS)
    below = ctl.level_counts
    i2, v2, c2, l2 = model.forward_nested_threshold(rows, theta, M_BOUNDS, cap=CAP_)
    same(idx, i2), same(val_sel, v2), same(counts, c2), same(levels, l2)
    i3, v3, c3, r3 = model.forward_threshold(rows, ctl)
    same(idx, i3), same(val_sel, v3), same(counts, c3), same(levels[-1], r3, "the last level is forward_threshold's reconstruction")
    _, val = model._select_cap(rows, CAP_, "test")
    wc, wv, wr = threshold_select(host(val), np.float32(theta))
    same(counts, wc), same(val_sel, wv), same(ctl.report, wr)
    same(below, R.counts_below(host(idx), wc, M_BOUNDS, H_), "level_counts")
    decoder, bias = model._nested_decoder()
    hd = (decoder[0], host(decoder[1])) + ((D_,) if decoder[0] == "packed" else ()) + tuple(decoder[2:])
    same(levels, R.nested_recons(host(idx), host(val), wc, M_BOUNDS, hd, host(bias)), "decoded from what forward() decodes from")
    with pytest.raises(ValueError, match="cap"):
        model.forward_nested_threshold(rows, 0.5, M_BOUNDS, cap=257)


# ---- 8: the Trainer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_two_optimizer_steps_through_the_trainer_reduce_the_summed_loss(sae_type, rows, tmp_path):
    logs = []
    model = _model(KIND[sae_type])
    if sae_type == "baseline_sae":
        model.normalize_decoder_weights()                     # as every step of this type leaves it: the steps are comparable
    t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path), log_fn=logs.append,
                log_every=1, batch_topk=True, batch_topk_cap=CAP_, batch_topk_nested_bounds="default", activity_window=B_, aux_k=4)
    assert t.nested_bounds == M_BOUNDS and (t.batch_topk.k, t.batch_topk.cap) == (K_, CAP_)
    for _ in range(3):                                        # one batch per call: the chunk is one batch of B_ rows
        t.one_epoch(rows)
    assert [len(b) for b in t.trained_batches] == [1, 1, 1] and int(t.batch_topk.batches) == 3
    summed = [sum(m[f"recon_loss_level_{l}"] for l in range(4)) for m in logs]
    print(sae_type, summed, [[m[f"l0_level_{l}"] for l in range(4)] for m in logs])
    assert summed[2] < summed[0]                             # logs[i] is the loss before step i
    key = "recon_loss" if sae_type == "b_sae" else "loss"
    assert all(abs(m[key] - s) <= 1e-6 * s for m, s in zip(logs, summed)) and "aux_loss" in logs[0] and "dead_features" in logs[0]
    for m in logs:
        l0 = [m[f"l0_level_{l}"] for l in range(4)]
        assert l0 == sorted(l0) and "l0_level_4" not in m and m["batch_topk/threshold"] > 0
        assert l0[3] * B_ == B_ * K_                          # the sum rule: every id of a top-k list is in range
    assert logs[2]["l0_level_3"] * B_ == int(t.batch_topk.report[0])
    plain = Trainer(CONFIG, sae_type, False, True, model=_model(KIND[sae_type]), dataset_dir=str(tmp_path), save_dir=str(tmp_path),
                    log_fn=logs.append, log_every=1, batch_topk=True, batch_topk_cap=CAP_)
    plain.one_epoch(rows)
    assert not any(k.startswith("l0_level_") for k in logs[-1])               # BatchTopK alone logs what it logged


# ---- 9: evaluation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_nested_errors_with_a_threshold(sae_type):
    model = _model(KIND[sae_type]).eval()
    ctl = BatchTopK(model, cap=CAP_)
    x = S.activations(92, 2 * B_ + 16, D_)
    x[50, 5] = np.nan                                        # one group of 8 rows is skipped
    loader = [dev(x[:B_]), dev(x[B_:])]
    model.forward_train_nested_batch_topk(loader[0][:32], ctl, M_BOUNDS, dense_latent=False)
    model.zero_grad(set_to_none=True)
    theta = ctl.threshold()
    r = nested_errors(model, loader, M_BOUNDS, group_rows=8, threshold=ctl)
    moments, kept = DatasetMoments(D_, 8, torch.device(DEV)), 0
    for batch in loader:                                      # evaluate_dataset's loop over forward_threshold's reconstruction
        _, _, counts, recon = model.forward_threshold(batch, ctl)
        moments.add(batch, recon)
        kept += int(counts.sum())
    e = moments.finish()
    assert r["mse"][3] == e["mse"] and r["fvu"][3] == e["fvu"] and r["variance"] == e["variance"]
    assert (r["rows"], r["skipped_rows"]) == (e["rows"], e["skipped_rows"]) == (2 * B_ + 16 - 8, 8)
    assert r["threshold"] == theta > 0 and r["l0"].dtype == np.float64 and r["l0"].shape == (4,)
    assert r["l0"][3] * (2 * B_ + 16) == kept and r["l0"].tolist() == sorted(r["l0"].tolist())
    assert len(set(r["mse"].tolist())) == 4
    by_number = nested_errors(model, loader, M_BOUNDS, group_rows=8, threshold=theta, cap=CAP_)
    assert by_number["mse"].tolist() == r["mse"].tolist() and by_number["l0"].tolist() == r["l0"].tolist()
    # without a threshold it is today's function
    plain = nested_errors(model, loader, M_BOUNDS, group_rows=8)
    assert "l0" not in plain and "threshold" not in plain
    moments = [DatasetMoments(D_, 8, torch.device(DEV)) for _ in range(4)]
    for batch in loader:
        levels = model.forward_nested(batch, M_BOUNDS)[2]
        for l, m in enumerate(moments):
            m.add(batch, levels[l])
    assert plain["mse"].tolist() == [m.finish()["mse"] for m in moments]
