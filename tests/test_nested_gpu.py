"""The nested-dictionary objective on the GPU (csrc/nested.hip, include/qsae_nested.h): the forward bit for bit against the
numpy restatement of tests/nested_util.py, against the existing sparse decoders (the last level; every level on the list whose
removed entries carry a value of 0) and on both front ends; the backward bit for bit against the existing gradient ops -- with
one level it IS forward_train's gradient (identity 1), with any bounds it is their composition, one call per level with
g_recon = G[level] (identity 2) -- with absent level gradients, and within the project's 1e-5 of an fp64 restatement; all five
entry points between guard words, twice on one workspace; the dispatcher ops; and the two top-k model classes: forward_nested,
forward_train_nested, the Trainer's ``nested_bounds`` and ``nested_errors``."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard_util as GU  # noqa: E402
import nested_util as U  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call, HostArray, HostPointers  # noqa: E402
from sparsity_curve_util import gaussian  # noqa: E402
from train_util import max_rel_err  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.inference import evaluate_dataset, nested_errors  # noqa: E402
from quantizedsae_amd.inference import framework as F  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import Trainer, nested_loss, trainer_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, F32 = torch.int32, torch.float32
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


# ---- forward ------------------------------------------------------------------------------------------------------------
def decode_nested(mod, idx, val, decoder, bias, bounds):
    """``decoder`` in the host form of tests/nested_util.py, its arrays already on the device"""
    if decoder[0] == "packed":
        return mod.decode_nested_binary(idx, val, decoder[1], decoder[2], decoder[3], decoder[4], bias, bounds)
    return mod.decode_nested_table(idx, val, decoder[1], decoder[2], bias, bounds)


def decode_plain(idx, val, decoder, bias):
    if decoder[0] == "packed":
        return ops.decode_binary_sparse(idx, val, decoder[1], decoder[2], decoder[3], decoder[4], bias)
    return ops.decode_table_sparse(idx, val, decoder[1], decoder[2], bias)


def check_forward(case):
    idx, val, bounds, decoder, bias = case
    want = U.nested_recons(idx, val, bounds, decoder, bias)
    dd = (decoder[0], dev(decoder[1])) + tuple(decoder[2:])
    di, dv, db = dev(idx), dev(val), None if bias is None else dev(bias)
    got = None
    for mod in (ops, torch_ops):
        got = decode_nested(mod, di, dv, dd, db, bounds)
        same(got, want, f"levels ({mod.__name__})")
    H = decoder[1].shape[0]
    if idx.shape[1] >= 1 and ((idx >= 0) & (idx < H)).all() and np.isfinite(decoder[1].astype(np.float64)).all():   # (the decoders take k >= 1)
        assert torch.equal(got[-1], decode_plain(di, dv, dd, db)), "the last level differs from the sparse decoder"
        for l, b in enumerate(bounds):                       # a removed entry with value 0 leaves a finite chain as it is
            masked = torch.where(di < b, dv, torch.zeros_like(dv))
            assert torch.equal(got[l], decode_plain(di, masked, dd, db)), f"level {l} differs from the masked sparse decode"
    return host(got)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_forward_equals_the_restatement_and_the_sparse_decoder(name):
    case = U.build_case(name)
    got = check_forward(case)
    if name.endswith("last_level_only"):                     # every level but the last is the bias alone
        bias = case[4]
        assert all(np.array_equal(got[l], np.broadcast_to((np.float32(0) + bias), got[l].shape)) for l in range(len(case[2]) - 1))


@pytest.mark.parametrize("name", sorted(U.SPECIAL_CASES))
def test_forward_special_values(name):
    U.check_special(name, check_forward(U.special_case(name)))


@pytest.mark.parametrize("kind", ["packed", "table"])
def test_forward_with_an_empty_list_writes_the_bias_rows(kind):
    idx, val, bounds, decoder, bias = U.build_case("packed_D48_n4" if kind == "packed" else "table_D48_s1.0")
    got = check_forward((idx[:, :0], val[:, :0], bounds, decoder, bias))
    assert np.array_equal(got, np.broadcast_to(np.float32(0) + bias, got.shape))
    got = check_forward((idx[:, :0], val[:, :0], bounds, decoder, None))
    assert not got.view(np.uint32).any()                     # +0 without a bias


def test_front_end_validation():
    idx, val, bounds, decoder, bias = U.build_case("table_D48_s1.0")
    di, dv, table = dev(idx), dev(val), dev(decoder[1])
    for bad in ([], [0, 512], [64, 64, 512], [64, 33, 512], [1, 33, 64], [1, 33, 64, 513], list(range(1, 9)) + [512], [1.5, 512]):
        with pytest.raises(ValueError, match="bounds|levels"):
            ops.decode_nested_table(di, dv, table, 1.0, None, bad)
    with pytest.raises(ValueError, match="idx is"):
        ops.decode_nested_table(di, dv[:, :3], table, 1.0, None, bounds)
    with pytest.raises(ValueError, match="bias"):
        ops.decode_nested_table(di, dv, table, 1.0, dev(bias)[:4], bounds)
    with pytest.raises(ValueError, match="level gradients"):
        ops.train_row_grad_nested(di, table, 1.0, [None], bounds, None, None)
    assert ops.decode_nested_table(di[:0], dv[:0], table, 1.0, None, bounds).shape == (4, 0, 48)       # no rows: nothing happens


# ---- backward -----------------------------------------------------------------------------------------------------------
class TrainCase:
    """The operands of one backward at the op level, from the lists of a forward case: x, the encoder weight, BinarySAE's
    logits and their soft table (also the baseline's table), L level gradients, a dense latent gradient and a polarize one."""

    def __init__(self, name: str, n_bits: int = 4, gamma: float = 4.0):
        idx, val, bounds, _, _ = U.build_case(name)
        _, D, _, _, B, k, H, _ = U.CASES[name]
        seed = 5000 + sorted(U.CASES).index(name)
        self.B, self.k, self.H, self.D, self.n_bits, self.bounds = B, k, H, D, n_bits, bounds
        self.step = gamma / 2 ** (n_bits - 1)
        self.idx, self.val = dev(idx), dev(val)
        self.x, self.W = dev(gaussian(seed, B, D)), dev(gaussian(seed + 1, H, D))
        self.logits = dev(gaussian(seed + 2, H, D * n_bits))
        self.table = ops.binary_soft_table(self.logits, D, n_bits)
        self.g = [dev(gaussian(seed + 10 + l, B, D) * np.float32(1.0 / (B * D))) for l in range(len(bounds))]
        self.g_latent = dev(gaussian(seed + 3, B, H) * np.float32(1e-3))
        self.g_pol = torch.tensor(1e-2, dtype=F32, device=DEV)
        self.offsets, self.entries = ops.train_csr(self.idx, H)
        self.levels = dev(U.levels_of(idx, bounds))                         # [B, k]
        self.unit_levels = dev(U.levels_of(np.arange(H), bounds))           # [H]

    def nested(self, mod=ops, g=None, bounds=None, want_dx=True):
        g = self.g if g is None else g
        bounds = self.bounds if bounds is None else bounds
        G, gv, dx = mod.train_row_grad_nested(self.idx, self.table, self.step, g, bounds, self.g_latent, self.W, want_dx=want_dx)
        dW, db, dl = mod.train_unit_grad_nested(self.offsets, self.entries, self.val, gv, self.x, G, bounds, self.logits,
                                                self.n_bits, self.step, self.g_pol)
        tW, tb, tWd = mod.train_table_unit_grad_nested(self.offsets, self.entries, self.val, gv, self.x, G, bounds)
        return dict(G=G, gv=gv, dx=dx, dW=dW, db=db, dl=dl, tW=tW, tb=tb, tWd=tWd)


BACKWARD_CASES = ["table_D4_s1.0", "table_D48_s1.0", "table_D520_s1.0", "table_k256", "table_last_level_only", "packed_eight_levels"]


@pytest.mark.parametrize("n_bits", [1, 4, 8])
@pytest.mark.parametrize("name", ["table_D4_s1.0", "table_D48_s1.0", "table_D520_s1.0", "table_k256"])
def test_one_level_is_forward_trains_gradient_bit_for_bit(name, n_bits):
    """Identity 1: bounds == [H]"""
    c = TrainCase(name, n_bits)
    for mod in (ops, torch_ops):
        n = c.nested(mod, g=c.g[:1], bounds=[c.H])
        same(n["G"][0], c.g[0], "G")
        gv, dx = ops.train_row_grad(c.idx, c.table, c.step, c.g[0], c.g_latent, c.W, want_dx=True)
        same(n["gv"], gv, "gv")
        same(n["dx"], dx, "dx")
        dW, db, dl = ops.train_unit_grad(c.offsets, c.entries, c.val, gv, c.x, c.g[0], c.logits, c.n_bits, c.step, c.g_pol)
        for key, want in (("dW", dW), ("db", db), ("dl", dl)):
            same(n[key], want, key)
        tW, tb, tWd = ops.train_table_unit_grad(c.offsets, c.entries, c.val, gv, c.x, c.g[0])
        for key, want in (("tW", tW), ("tb", tb), ("tWd", tWd)):
            same(n[key], want, key)


def check_composition(c, g, n):
    """Identity 2: every nested result is what the existing ops give when they are called once per level with
    g_recon = G[level] and restricted to that level's entries or units."""
    L = len(c.bounds)
    same(n["G"], U.suffix_sums([None if t is None else host(t) for t in g], c.B, c.D), "G against the restatement")
    G = n["G"]
    gv = torch.full_like(n["gv"], float("nan"))
    for l in range(L):
        gv_l, _ = ops.train_row_grad(c.idx, c.table, c.step, G[l], c.g_latent, None, want_dx=False)
        gv = torch.where(c.levels == l, gv_l, gv)
    same(n["gv"], gv, "gv")
    scattered = torch.zeros((c.B, c.H), dtype=F32, device=DEV).scatter_(1, c.idx.long(), n["gv"])
    _, dx = ops.train_row_grad(c.idx, c.table, c.step, None, scattered, c.W, want_dx=True)
    same(n["dx"], dx, "dx")
    want = {k: torch.full_like(n[k], float("nan")) for k in ("dW", "db", "dl", "tW", "tb", "tWd")}
    for l in range(L):
        mine = c.unit_levels == l
        dW, db, dl = ops.train_unit_grad(c.offsets, c.entries, c.val, n["gv"], c.x, G[l], c.logits, c.n_bits, c.step, c.g_pol)
        tW, tb, tWd = ops.train_table_unit_grad(c.offsets, c.entries, c.val, n["gv"], c.x, G[l])
        for key, t in (("dW", dW), ("db", db), ("dl", dl), ("tW", tW), ("tb", tb)):
            want[key][mine] = t[mine]
        want["tWd"][:, mine] = tWd[:, mine]
    for key, t in want.items():
        same(n[key], t, key)


@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_backward_is_the_composition_of_the_existing_ops_bit_for_bit(name):
    c = TrainCase(name, 8 if name == "table_D48_s1.0" else 1 if name == "table_D4_s1.0" else 4)
    n = c.nested()
    check_composition(c, c.g, n)
    again = c.nested(torch_ops)
    for key in n:                                            # the other front end, and a second run: the same bits
        same(again[key], n[key], key)


@pytest.mark.parametrize("absent", [(0,), (3,), (1, 2), (0, 1, 2), (1, 2, 3), (0, 1, 2, 3)])
def test_an_absent_level_gradient_is_skipped(absent):
    c = TrainCase("table_D48_s1.0")
    g = [None if l in absent else t for l, t in enumerate(c.g)]
    n = c.nested(g=g)
    check_composition(c, g, n)
    last = max((l for l in range(4) if l not in absent), default=-1)
    assert not host(n["G"][last + 1:]).view(np.uint32).any()               # +0 behind the last gradient
    if last >= 0:
        same(n["G"][last], c.g[last], "the last gradient is copied")


@pytest.mark.parametrize("name", ["table_D48_s1.0", "table_D520_s1.0", "table_k256"])
def test_gradients_against_fp64(name):
    c = TrainCase(name)
    n = c.nested()
    G = U.suffix_sums([host(t) for t in c.g], c.B, c.D)
    gl_sel = torch.gather(c.g_latent, 1, c.idx.long())
    w = U.grads64(host(c.x), host(c.W), host(c.table), c.step, host(c.idx), host(c.val), G, c.bounds, host(gl_sel), want_dx=True)
    dl = U.logit_grads64(w["rows"], host(c.logits), c.D, c.n_bits, c.step, float(c.g_pol))
    figures = {"gv": max_rel_err(n["gv"], w["gv"]), "dx": max_rel_err(n["dx"], w["x"]),
               "dW_enc": max_rel_err(n["dW"], w["encoder.0.weight"]), "db_enc": max_rel_err(n["db"], w["encoder.0.bias"]),
               "dlogits": max_rel_err(n["dl"], dl), "dW_dec": max_rel_err(n["tWd"], w["rows"].t()),
               "tW_enc": max_rel_err(n["tW"], w["encoder.0.weight"]),
               "db_dec": max_rel_err(ops.train_col_sum(n["G"][0]), w["decoder.bias"])}
    print(name, figures)
    assert all(v <= TOL for v in figures.values()), figures


# ---- all five entry points between guard words --------------------------------------------------------------------------
def _guard_decode(name):
    def build():
        idx, val, bounds, decoder, bias = U.build_case(name)
        B, k = idx.shape
        H, L = decoder[1].shape[0], len(bounds)
        packed = decoder[0] == "packed"
        D = decoder[2] if packed else decoder[1].shape[1]
        want = U.nested_recons(idx, val, bounds, decoder, bias)

        def front(t):
            dd = (decoder[0], t["dict"]) + tuple(decoder[2:])
            return {"recon": decode_nested(ops, t["idx"], t["val"], dd, t.get("bias"), bounds)}
        dict_args = [Buf("dict", "in", dev(decoder[1])), H, D] + ([decoder[3], decoder[4]] if packed else [decoder[2]])
        entry = "qsaen_decode_nested_binary" if packed else "qsaen_decode_nested_table"
        return Call(name, entry,
                    [Buf("idx", "in", dev(idx)), Buf("val", "in", dev(val)), B, k, *dict_args,
                     Buf("bias", "in", dev(bias)) if bias is not None else None, HostArray(bounds), L,
                     Buf("recon", "out", shape=(L, B, D), dtype=F32), STREAM],
                    front, expect={"recon": torch.from_numpy(want)})
    return build


def _guard_row(name, absent=()):
    def build():
        c = TrainCase(name)
        L = len(c.bounds)
        gbufs = [None if l in absent else Buf(f"g{l}", "in", c.g[l]) for l in range(L)]

        def front(t):
            g = [t.get(f"g{l}") for l in range(L)]
            G, gv, dx = ops.train_row_grad_nested(t["idx"], t["table"], c.step, g, c.bounds, t["g_latent"], t["W"], want_dx=True)
            return {"G": G, "gv": gv, "dx": dx}
        return Call(name, "qsaen_row_grad_nested",
                    [Buf("idx", "in", c.idx), c.B, c.k, Buf("table", "in", c.table), c.H, c.D, c.step, HostPointers(gbufs),
                     HostArray(c.bounds), L, Buf("g_latent", "in", c.g_latent), c.H, Buf("W", "in", c.W),
                     Buf("G", "out", shape=(L, c.B, c.D), dtype=F32), Buf("gv", "out", shape=(c.B, c.k), dtype=F32),
                     Buf("dx", "out", shape=(c.B, c.D), dtype=F32), STREAM], front)
    return build


def _guard_units(name, table: bool):
    def build():
        c = TrainCase(name)
        L = len(c.bounds)
        G, gv, _ = ops.train_row_grad_nested(c.idx, c.table, c.step, c.g, c.bounds, c.g_latent, None)
        common = [Buf("offsets", "in", c.offsets), Buf("entries", "in", c.entries), Buf("val", "in", c.val), Buf("gv", "in", gv),
                  c.B, c.k, Buf("x", "in", c.x), Buf("G", "in", G), HostArray(c.bounds), L]
        if table:
            def front(t):
                dW, db, dWd = ops.train_table_unit_grad_nested(t["offsets"], t["entries"], t["val"], t["gv"], t["x"], t["G"], c.bounds)
                return {"dW": dW, "db": db, "dWd": dWd}
            entry = "qsaen_train_table_unit_grad_nested"
            args = common + [c.H, c.D, Buf("dW", "out", shape=(c.H, c.D), dtype=F32), Buf("db", "out", shape=(c.H,), dtype=F32),
                             Buf("dWd", "out", shape=(c.D, c.H), dtype=F32), c.H, WS, WS_BYTES, STREAM]
        else:
            def front(t):
                dW, db, dl = ops.train_unit_grad_nested(t["offsets"], t["entries"], t["val"], t["gv"], t["x"], t["G"], c.bounds,
                                                        t["logits"], c.n_bits, c.step, t["g_pol"])
                return {"dW": dW, "db": db, "dl": dl}
            entry = "qsaen_train_unit_grad_nested"
            args = common + [Buf("logits", "in", c.logits), c.H, c.D, c.n_bits, c.step, Buf("g_pol", "in", c.g_pol.reshape(1)),
                             Buf("dW", "out", shape=(c.H, c.D), dtype=F32), Buf("db", "out", shape=(c.H,), dtype=F32),
                             Buf("dl", "out", shape=(c.H, c.D * c.n_bits), dtype=F32), WS, WS_BYTES, STREAM]
        return Call(name, entry, args, front, sizer=(entry + "_workspace_bytes", (c.B, c.k, c.H, c.D)))
    return build


#: label -> (entry point, builder of its guard_util.Call); tests/test_nested_host.py reads the entry points for its ledger.
#: Building a case touches the GPU; importing this table does not.
GUARD_CASES = {
    "decode_binary_minimal": ("qsaen_decode_nested_binary", _guard_decode("packed_D4_n1")),
    "decode_binary_row_tail": ("qsaen_decode_nested_binary", _guard_decode("packed_D520_n4")),
    "decode_binary_long_list": ("qsaen_decode_nested_binary", _guard_decode("packed_k256")),
    "decode_table_minimal": ("qsaen_decode_nested_table", _guard_decode("table_D4_s1.0")),
    "decode_table_row_tail": ("qsaen_decode_nested_table", _guard_decode("table_D520_s0.5_nobias")),
    "decode_table_long_list": ("qsaen_decode_nested_table", _guard_decode("table_k256")),
    "row_grad_minimal": ("qsaen_row_grad_nested", _guard_row("table_D4_s1.0")),
    "row_grad_row_tail_absent_levels": ("qsaen_row_grad_nested", _guard_row("table_D520_s1.0", absent=(1, 3))),
    "row_grad_long_list": ("qsaen_row_grad_nested", _guard_row("table_k256")),
    "unit_grad_row_tail": ("qsaen_train_unit_grad_nested", _guard_units("table_D520_s1.0", False)),
    "unit_grad_split_lists": ("qsaen_train_unit_grad_nested", _guard_units("table_k256", False)),
    "table_unit_grad_row_tail": ("qsaen_train_table_unit_grad_nested", _guard_units("table_D520_s1.0", True)),
    "table_unit_grad_split_lists": ("qsaen_train_table_unit_grad_nested", _guard_units("table_k256", True)),
}


@pytest.mark.parametrize("label", sorted(GUARD_CASES))
def test_entry_point_between_guard_words(label):
    entry, build = GUARD_CASES[label]
    call = build()
    assert call.entry == entry
    GU.run_call(call, _lib.load(), DEV)


# ---- the dispatcher ops ---------------------------------------------------------------------------------------------------
def test_dispatcher_ops():
    c = TrainCase("table_D48_s1.0")
    Q = torch.ops.qsae
    torch.library.opcheck(Q.decode_nested_table.default, (c.idx, c.val, c.table, c.step, None, c.bounds))
    g = [c.g[0], None, c.g[2], c.g[3]]
    torch.library.opcheck(Q.train_row_grad_nested.default, (c.idx, c.table, c.step, g, c.bounds, c.g_latent, c.W, True))
    G, gv, _ = ops.train_row_grad_nested(c.idx, c.table, c.step, g, c.bounds, c.g_latent, None)
    torch.library.opcheck(Q.train_unit_grad_nested.default, (c.offsets, c.entries, c.val, gv, c.x, G, c.bounds, c.logits, c.n_bits,
                                                              c.step, c.g_pol, True, True))
    torch.library.opcheck(Q.train_table_unit_grad_nested.default, (c.offsets, c.entries, c.val, gv, c.x, G, c.bounds, True, True))


# ---- the two top-k model classes ----------------------------------------------------------------------------------------
D_, H_, K_, B_ = 48, 512, 6, 64
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
def test_forward_train_nested_with_one_level_is_forward_train(sae_type, rows):
    """Identity 1 through the model: outputs and every .grad, bit for bit"""
    model = _model(KIND[sae_type])
    x = rows.clone().requires_grad_()
    out = model.forward_train(x)
    trainer_loss(sae_type, out, rows, CONFIG)
    want, want_x = _grads(model), x.grad.clone()
    model.zero_grad(set_to_none=True)
    x.grad = None
    nested = model.forward_train_nested(x, [H_])
    assert isinstance(nested[1], tuple) and len(nested[1]) == 1 and len(nested) == len(out)
    same(nested[0], out[0], "latent")
    same(nested[1][0], out[1], "reconstruction")
    if sae_type == "b_sae":
        same(nested[2], out[2], "polarize")
    nested_loss(sae_type, nested, rows, CONFIG)
    for k, g in _grads(model).items():
        same(g, want[k], k)
    same(x.grad, want_x, "x.grad")


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_train_nested_levels_and_gradients(sae_type, rows):
    model = _model(KIND[sae_type])
    model.activity = None
    latent, levels, *rest = model.forward_train_nested(rows, M_BOUNDS, dense_latent=False)
    assert latent is None and len(levels) == 4 and levels[0]._base is levels[3]._base
    plain = model.forward_train(rows)
    same(levels[3], plain[1], "the last level is forward_train's reconstruction")
    idx, val, inf_levels = model.forward_nested(rows, M_BOUNDS)
    decode_mode = getattr(model.decoder, "decode_mode", None)
    if sae_type == "b_sae":                                  # forward_nested honours decode_mode; training decodes the soft table
        model.decoder.decode_mode = "soft"
        same(model.forward_nested(rows, M_BOUNDS)[2], levels[0]._base, "soft levels")
        model.decoder.decode_mode = "hard"
        hard = model.forward_nested(rows, M_BOUNDS)
        st = model.decoder.packed()
        same(hard[2], ops.decode_nested_binary(hard[0], hard[1], st["packed"], D_, 4, model.decoder.quantization_step,
                                               model.decoder.bias.detach(), M_BOUNDS), "hard levels")
        same(hard[2][3], model.forward_compact(rows)[2], "the last hard level is forward's reconstruction")
        model.decoder.decode_mode = decode_mode
    else:
        same(inf_levels, levels[0]._base, "levels")
        same(inf_levels[3], model.forward_compact(rows)[2], "the last level is forward's reconstruction")
    # the gradient of the summed loss against fp64 autograd on the same selection
    losses = nested_loss(sae_type, (latent, levels, *rest), rows, CONFIG)
    assert losses.shape == (4,)
    got = _grads(model)
    lin = model.encoder.linear
    W = lin.weight.detach().cpu().double().requires_grad_()
    b = lin.bias.detach().cpu().double().requires_grad_()
    dec = model.decoder.weight.detach().cpu().double().requires_grad_()
    bd = model.decoder.bias.detach().cpu().double().requires_grad_()
    x64, ii = rows.cpu().double(), idx.cpu().long()
    if sae_type == "baseline_sae":
        table, step, coef, pol = dec.t(), 1.0, 1.0, 0.0
    else:
        bw = 2.0 ** torch.arange(4, dtype=torch.float64)
        pw = bw.clone()
        bw[-1] = -bw[-1]
        p = torch.sigmoid(dec).view(H_, D_, 4)
        table, step, coef = (p * bw).sum(-1), model.decoder.quantization_step, 0.5
        pol = CONFIG["polarize_lambda"] * (p * (1 - p) * pw).mean()
    pre = (x64[:, None, :] * W[ii]).sum(-1) + b[ii]
    total = pol
    for l, bound in enumerate(M_BOUNDS):
        keep = (ii < bound).double()
        recon = step * ((pre * keep)[:, :, None] * table[ii]).sum(1) + bd
        level_loss = coef * ((recon - x64) ** 2).mean()
        assert abs(float(losses[l]) - level_loss.item()) <= TOL * level_loss.item()
        total = total + level_loss
    total.backward()
    want = {"encoder.0.weight": W.grad, "encoder.0.bias": b.grad, "decoder.weight": dec.grad, "decoder.bias": bd.grad}
    assert sorted(got) == sorted(want)
    figures = {k: max_rel_err(got[k], want[k]) for k in want}
    print(sae_type, figures)
    assert all(v <= TOL for v in figures.values()), figures


def test_forward_train_nested_feeds_the_tracker_once_and_saves_four_tensors(rows, monkeypatch):
    model = _model("baseline")
    calls = []

    class Spy:
        def add_compact(self, idx, val):
            calls.append(tuple(idx.shape))
    model.activity = Spy()
    _, levels = model.forward_train_nested(rows, M_BOUNDS)
    assert calls == [(B_, K_)]
    saved = levels[0]._base.grad_fn.saved_tensors
    assert len(saved) == 4 and sorted(tuple(t.shape) for t in saved) == sorted([(B_, D_), (B_, K_), (B_, K_), (H_, D_)])
    for bad in ([], [64, 64, 512], [64, 256], [0, 512]):
        with pytest.raises(ValueError, match="bounds|levels"):
            model.forward_train_nested(rows, bad)
    with pytest.raises(ValueError, match="expected \\[batch"):
        model.forward_nested(rows[:, :8], M_BOUNDS)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_two_optimizer_steps_through_the_trainer_reduce_the_summed_loss(sae_type, rows, tmp_path):
    logs = []
    model = _model(KIND[sae_type])
    if sae_type == "baseline_sae":
        model.normalize_decoder_weights()                     # as every step of this type leaves it: the steps are comparable
    t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path),
                log_fn=logs.append, log_every=1, nested_bounds=M_BOUNDS, activity_window=B_, aux_k=4)
    assert t.nested_bounds == M_BOUNDS
    for _ in range(3):                                        # one batch per call: the chunk is one batch of B_ rows
        t.one_epoch(rows)
    assert [len(b) for b in t.trained_batches] == [1, 1, 1]
    summed = [sum(m[f"recon_loss_level_{l}"] for l in range(4)) for m in logs]
    print(sae_type, summed)
    assert summed[2] < summed[0]                             # logs[i] is the loss before step i
    key = "recon_loss" if sae_type == "b_sae" else "loss"
    assert all(abs(m[key] - s) <= 1e-6 * s for m, s in zip(logs, summed)) and "aux_loss" in logs[0]
    default = Trainer(CONFIG, sae_type, False, True, model=_model(KIND[sae_type]), dataset_dir=str(tmp_path),
                      save_dir=str(tmp_path), nested_bounds="default")
    assert default.nested_bounds == [64, 128, 256, 512]


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_nested_errors_last_level_equals_evaluate_dataset(sae_type):
    model = _model(KIND[sae_type]).eval()
    sae = F.SAEWrapper(F.SAE_REGISTRY[sae_type], model, DEV)
    x = S.activations(92, 3 * B_, D_)
    x[70, 5] = np.nan                                        # one group of 32 rows is skipped
    loader = [dev(x[:B_]), dev(x[B_:])]
    r = nested_errors(sae, loader, M_BOUNDS, group_rows=32)
    e = evaluate_dataset(sae, loader, group_rows=32)
    assert r["mse"][3] == e["mse"] and r["fvu"][3] == e["fvu"] and r["variance"] == e["variance"]
    assert (r["rows"], r["skipped_rows"]) == (e["rows"], e["skipped_rows"]) == (3 * B_ - 32, 32)
    assert r["bounds"] == M_BOUNDS and r["mse"].shape == (4,) and r["fvu"].shape == (4,) and len(r["levels"]) == 4
    assert len(set(r["mse"].tolist())) == 4                  # four different reconstructions
    assert nested_errors(model, loader, group_rows=32)["bounds"] == [64, 128, 256, 512]
