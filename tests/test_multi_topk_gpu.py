"""The Multi-TopK objective on the GPU (csrc/multi_topk.hip, include/qsae_multik.h): all five entry points between guard words,
twice on one poisoned workspace, bit for bit against the numpy restatement of tests/multi_topk_util.py (the logit gradient,
which goes through a sigmoid, against the front end's bits and within the project's 1e-5 of fp64); every decode point bit for
bit the existing sparse decoder on the truncated list, and the model rebuilt with top_k = ks[p]; with one point every call
and the model's forward_train_multi_topk bit for bit the plain call and forward_train with its gradients; absent point
gradients; a unit list that passes 256 entries with chunks that mix points; the dispatcher ops; and a 20-step
``Trainer(multi_topk="default")`` run that gives the same parameters twice."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard_util as GU  # noqa: E402
import multi_topk_util as U  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call, HostArray, HostPointers  # noqa: E402
from sparsity_curve_util import gaussian  # noqa: E402
from train_util import max_rel_err  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402
from quantizedsae_amd.training import Trainer, multi_topk_loss, trainer_loss  # noqa: E402

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


def decode_multik(mod, idx, val, decoder, bias, ks):
    """``decoder`` in the host form of tests/multi_topk_util.py, its arrays already on the device"""
    if decoder[0] == "packed":
        return mod.decode_multik_binary(idx, val, decoder[1], decoder[2], decoder[3], decoder[4], bias, ks)
    return mod.decode_multik_table(idx, val, decoder[1], decoder[2], bias, ks)


def decode_plain(idx, val, decoder, bias):
    if decoder[0] == "packed":
        return ops.decode_binary_sparse(idx, val, decoder[1], decoder[2], decoder[3], decoder[4], bias)
    return ops.decode_table_sparse(idx, val, decoder[1], decoder[2], bias)


# ---- forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_every_point_is_the_sparse_decoder_on_the_truncated_list(name):
    idx, val, ks, decoder, bias = U.build_case(name)
    dd = (decoder[0], dev(decoder[1])) + tuple(decoder[2:])
    di, dv, db = dev(idx), dev(val), None if bias is None else dev(bias)
    got = decode_multik(ops, di, dv, dd, db, ks)
    same(decode_multik(torch_ops, di, dv, dd, db, ks), got, "the dispatcher op")
    for p, k in enumerate(ks):
        same(got[p], decode_plain(di[:, :k].contiguous(), dv[:, :k].contiguous(), dd, db), f"point {p} (k = {k})")
    if name in ("packed_K65_D48_n1_five", "table_K256_D48", "table_split_lists"):            # one restatement per family is enough
        same(got, U.recons(idx, val, ks, decoder, bias), "the restatement")


# ---- backward -----------------------------------------------------------------------------------------------------------
class TrainCase:
    """The operands of the gradient calls of a table case on the device, the CSR lists of its idx, and a binary decoder's
    logits next to it (the unit sums of BinarySAE read logits; their reconstruction gradient is G all the same)."""

    def __init__(self, name: str, n_bits: int = 4):
        c = U.grad_inputs(name)
        self.host = c
        self.name, self.ks, self.step, self.n_bits = name, c["ks"], c["step"], n_bits
        self.B, self.K, self.H, self.D = c["B"], c["K"], c["H"], c["D"]
        self.idx, self.val, self.table = dev(c["idx"]), dev(c["val"]), dev(c["table"])
        self.g = [dev(t) for t in c["g"]]
        self.g_latent, self.W, self.x = dev(c["g_latent"]), dev(c["W"]), dev(c["x"])
        self.logits = dev(gaussian(7000 + n_bits, self.H, self.D * n_bits))
        self.g_pol = torch.tensor(0.25, dtype=F32, device=DEV)
        self.offsets, self.entries = ops.train_csr(self.idx, self.H)

    def multik(self, mod=ops, g=None, ks=None):
        g = self.g if g is None else g
        ks = self.ks if ks is None else ks
        G, gv, dx = mod.train_row_grad_multik(self.idx, self.table, self.step, g, ks, self.g_latent, self.W, want_dx=True)
        dW, db, dl = mod.train_unit_grad_multik(self.offsets, self.entries, self.val, gv, self.x, G, ks, self.logits, self.n_bits,
                                                self.step, self.g_pol)
        tW, tb, tWd = mod.train_table_unit_grad_multik(self.offsets, self.entries, self.val, gv, self.x, G, ks)
        return {"G": G, "gv": gv, "dx": dx, "dW": dW, "db": db, "dl": dl, "tW": tW, "tb": tb, "tWd": tWd}


@pytest.mark.parametrize("n_bits", [1, 4, 8])
@pytest.mark.parametrize("name", ["table_K1_D4", "table_K256_D48_one", "table_K12_D520_nobias", "table_split_lists"])
def test_one_point_is_the_plain_call_bit_for_bit(name, n_bits):
    """n_ks == 1, ks = [K]: every call is the call it extends"""
    c = TrainCase(name, n_bits)
    for mod in (ops, torch_ops):
        n = c.multik(mod, g=c.g[:1], ks=[c.K])
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
    same(ops.decode_multik_table(c.idx, c.val, c.table, c.step, None, [c.K])[0],
         ops.decode_table_sparse(c.idx, c.val, c.table, c.step, None), "decode")


def check_restatement(c, g, n):
    """G, gv, dx, dW_enc, db_enc and the table form's decoder gradient bit for bit; the logit gradient within TOL of fp64"""
    h = c.host
    gh = [None if t is None else host(t) for t in g]
    G, gv, dx = U.row_grad(h["idx"], h["table"], c.step, gh, c.ks, h["g_latent"], h["W"])
    same(n["G"], G, "G")
    same(n["gv"], gv, "gv")
    same(n["dx"], dx, "dx")
    u = U.unit_grads(h["idx"], h["val"], gv, h["x"], G, c.ks, c.H)
    for key in ("dW", "tW"):
        same(n[key], u["dW"], key)
    for key in ("db", "tb"):
        same(n[key], u["db"], key)
    same(n["tWd"], np.ascontiguousarray(u["rows"].T), "tWd")
    dl = U.logit_grads64(u["rows"].astype(np.float64), host(c.logits), c.D, c.n_bits, c.step, float(c.g_pol))
    err = max_rel_err(n["dl"], dl)
    print(c.name, "dlogits against fp64:", err)
    assert err <= TOL


@pytest.mark.parametrize("name", ["table_K7_D48", "table_K12_D516_s0.5", "table_K12_D520_nobias", "table_K65_D48_five",
                                  "table_K12_D48_eight", "table_split_lists"])
def test_backward_equals_the_restatement_bit_for_bit(name):
    c = TrainCase(name, 8 if name == "table_K7_D48" else 1 if name == "table_K12_D48_eight" else 4)
    n = c.multik()
    check_restatement(c, c.g, n)
    again = c.multik(torch_ops)
    for key in n:                                            # the other front end, and a second run: the same bits
        same(again[key], n[key], key)


@pytest.mark.parametrize("absent", [(0,), (3,), (1, 2), (1, 2, 3), (0, 1, 2, 3)])
def test_an_absent_point_gradient_is_skipped(absent):
    c = TrainCase("table_K12_D520_nobias")                   # ks = [1, 2, 3, 12]
    g = [None if p in absent else t for p, t in enumerate(c.g)]
    n = c.multik(g=g)
    same(n["G"], U.suffix_sums([None if t is None else host(t) for t in g], c.B, c.D), "G")
    last = max((p for p in range(4) if p not in absent), default=-1)
    assert not host(n["G"][last + 1:]).view(np.uint32).any()               # +0 behind the last gradient
    if last >= 0:
        same(n["G"][last], c.g[last], "the last gradient is copied")
    # the composition with the existing ops: an entry of point p gets what the plain call gives with g_recon = G[p]
    pts = dev(U.points_of(c.K, c.ks))[None, :].expand(c.B, c.K)
    gv = torch.full_like(n["gv"], float("nan"))
    for p in range(4):
        gv_p, _ = ops.train_row_grad(c.idx, c.table, c.step, n["G"][p], c.g_latent, None, want_dx=False)
        gv = torch.where(pts == p, gv_p, gv)
    same(n["gv"], gv, "gv")


def test_split_lists_mix_points_in_a_chunk():
    """B = 300, K = 4, H = 8 with unit 0 in every row: what the case is there for"""
    c = TrainCase("table_split_lists")
    counts = host(c.offsets[1:] - c.offsets[:-1])
    assert counts.max() > 256                                 # a list is split into chunks
    ranks = host(c.entries) % c.K
    h = int(counts.argmax())
    first_chunk = ranks[int(c.offsets[h]):int(c.offsets[h]) + 256]
    assert len(set(U.points_of(c.K, c.ks)[first_chunk].tolist())) == 2       # and its first chunk mixes the two points


# ---- all five entry points between guard words --------------------------------------------------------------------------
def _guard_decode(name, outside=False):
    def build():
        idx, val, ks, decoder, bias = U.build_case(name, outside=outside)
        B, K = idx.shape
        H, P = decoder[1].shape[0], len(ks)
        packed = decoder[0] == "packed"
        D = decoder[2] if packed else decoder[1].shape[1]
        want = U.recons(idx, val, ks, decoder, bias)

        def front(t):
            dd = (decoder[0], t["dict"]) + tuple(decoder[2:])
            return {"recon": decode_multik(ops, t["idx"], t["val"], dd, t.get("bias"), ks)}
        dict_args = [Buf("dict", "in", dev(decoder[1])), H, D] + ([decoder[3], decoder[4]] if packed else [decoder[2]])
        entry = "qsaek_decode_multik_binary" if packed else "qsaek_decode_multik_table"
        return Call(name, entry,
                    [Buf("idx", "in", dev(idx)), Buf("val", "in", dev(val)), B, K, *dict_args,
                     Buf("bias", "in", dev(bias)) if bias is not None else None, HostArray(ks), P,
                     Buf("recon", "out", shape=(P, B, D), dtype=F32), STREAM],
                    front, expect={"recon": torch.from_numpy(want)})
    return build


def _guard_row(name, absent=(), outside=False):
    def build():
        c = TrainCase(name)
        P = len(c.ks)
        idx_h = U.build_case(name, outside=True)[0] if outside else c.host["idx"]
        gbufs = [None if p in absent else Buf(f"g{p}", "in", c.g[p]) for p in range(P)]
        G, gv, dx = U.row_grad(idx_h, c.host["table"], c.step, [None if p in absent else c.host["g"][p] for p in range(P)], c.ks,
                               c.host["g_latent"], c.host["W"])

        def front(t):
            g = [t.get(f"g{p}") for p in range(P)]
            G_, gv_, dx_ = ops.train_row_grad_multik(t["idx"], t["table"], c.step, g, c.ks, t["g_latent"], t["W"], want_dx=True)
            return {"G": G_, "gv": gv_, "dx": dx_}
        return Call(name, "qsaek_row_grad_multik",
                    [Buf("idx", "in", dev(idx_h)), c.B, c.K, Buf("table", "in", c.table), c.H, c.D, c.step, HostPointers(gbufs),
                     HostArray(c.ks), P, Buf("g_latent", "in", c.g_latent), c.H, Buf("W", "in", c.W),
                     Buf("G", "out", shape=(P, c.B, c.D), dtype=F32), Buf("gv", "out", shape=(c.B, c.K), dtype=F32),
                     Buf("dx", "out", shape=(c.B, c.D), dtype=F32), STREAM], front,
                    expect={"G": torch.from_numpy(G), "gv": torch.from_numpy(gv), "dx": torch.from_numpy(dx)})
    return build


def _guard_units(name, table: bool):
    def build():
        c = TrainCase(name)
        h = c.host
        P = len(c.ks)
        G, gv, _ = ops.train_row_grad_multik(c.idx, c.table, c.step, c.g, c.ks, c.g_latent, None)
        u = U.unit_grads(h["idx"], h["val"], host(gv), h["x"], host(G), c.ks, c.H)
        common = [Buf("offsets", "in", c.offsets), Buf("entries", "in", c.entries), Buf("val", "in", c.val), Buf("gv", "in", gv),
                  c.B, c.K, Buf("x", "in", c.x), Buf("G", "in", G), HostArray(c.ks), P]
        expect = {"dW": torch.from_numpy(u["dW"]), "db": torch.from_numpy(u["db"])}
        verify = None
        if table:
            def front(t):
                dW, db, dWd = ops.train_table_unit_grad_multik(t["offsets"], t["entries"], t["val"], t["gv"], t["x"], t["G"], c.ks)
                return {"dW": dW, "db": db, "dWd": dWd}
            entry = "qsaek_train_table_unit_grad_multik"
            expect["dWd"] = torch.from_numpy(np.ascontiguousarray(u["rows"].T))
            args = common + [c.H, c.D, Buf("dW", "out", shape=(c.H, c.D), dtype=F32), Buf("db", "out", shape=(c.H,), dtype=F32),
                             Buf("dWd", "out", shape=(c.D, c.H), dtype=F32), c.H, WS, WS_BYTES, STREAM]
        else:
            def front(t):
                dW, db, dl = ops.train_unit_grad_multik(t["offsets"], t["entries"], t["val"], t["gv"], t["x"], t["G"], c.ks,
                                                        t["logits"], c.n_bits, c.step, t["g_pol"])
                return {"dW": dW, "db": db, "dl": dl}
            dl64 = U.logit_grads64(u["rows"].astype(np.float64), host(c.logits), c.D, c.n_bits, c.step, float(c.g_pol))

            def verify(got):                                  # the sigmoid keeps the logit gradient out of the restatement's bits
                assert max_rel_err(got["dl"], dl64) <= TOL
            entry = "qsaek_train_unit_grad_multik"
            args = common + [Buf("logits", "in", c.logits), c.H, c.D, c.n_bits, c.step, Buf("g_pol", "in", c.g_pol.reshape(1)),
                             Buf("dW", "out", shape=(c.H, c.D), dtype=F32), Buf("db", "out", shape=(c.H,), dtype=F32),
                             Buf("dl", "out", shape=(c.H, c.D * c.n_bits), dtype=F32), WS, WS_BYTES, STREAM]
        return Call(name, entry, args, front, sizer=(entry + "_workspace_bytes", (c.B, c.K, c.H, c.D)), expect=expect, verify=verify)
    return build


#: label -> (entry point, builder of its guard_util.Call); tests/test_multi_topk_host.py reads the entry points for its ledger.
#: Building a case touches the GPU; importing this table does not.
GUARD_CASES = {
    "decode_binary_minimal": ("qsaek_decode_multik_binary", _guard_decode("packed_K1_D4_n1")),
    "decode_binary_row_tail": ("qsaek_decode_multik_binary", _guard_decode("packed_K12_D520_n4")),
    "decode_binary_half_octet_n8": ("qsaek_decode_multik_binary", _guard_decode("packed_K12_D516_n8")),
    "decode_binary_five_points_n1": ("qsaek_decode_multik_binary", _guard_decode("packed_K65_D48_n1_five")),
    "decode_binary_long_list": ("qsaek_decode_multik_binary", _guard_decode("packed_K256_D48_n4")),
    "decode_binary_eight_points": ("qsaek_decode_multik_binary", _guard_decode("packed_K12_D48_n8_eight")),
    "decode_binary_ids_outside": ("qsaek_decode_multik_binary", _guard_decode("packed_K7_D48_n4", outside=True)),
    "decode_table_minimal": ("qsaek_decode_multik_table", _guard_decode("table_K1_D4")),
    "decode_table_half_octet": ("qsaek_decode_multik_table", _guard_decode("table_K12_D516_s0.5")),
    "decode_table_row_tail": ("qsaek_decode_multik_table", _guard_decode("table_K12_D520_nobias")),
    "decode_table_five_points": ("qsaek_decode_multik_table", _guard_decode("table_K65_D48_five")),
    "decode_table_k_4k": ("qsaek_decode_multik_table", _guard_decode("table_K256_D48_k_4k")),
    "decode_table_ids_outside": ("qsaek_decode_multik_table", _guard_decode("table_K65_D48_five", outside=True)),
    "row_grad_minimal": ("qsaek_row_grad_multik", _guard_row("table_K1_D4")),
    "row_grad_row_tail_absent_points": ("qsaek_row_grad_multik", _guard_row("table_K12_D520_nobias", absent=(1, 3))),
    "row_grad_no_gradient_at_all": ("qsaek_row_grad_multik", _guard_row("table_K7_D48", absent=(0, 1))),
    "row_grad_five_points": ("qsaek_row_grad_multik", _guard_row("table_K65_D48_five")),
    "row_grad_ids_outside": ("qsaek_row_grad_multik", _guard_row("table_K7_D48", outside=True)),
    "unit_grad_row_tail": ("qsaek_train_unit_grad_multik", _guard_units("table_K12_D520_nobias", False)),
    "unit_grad_split_lists": ("qsaek_train_unit_grad_multik", _guard_units("table_split_lists", False)),
    "table_unit_grad_half_octet": ("qsaek_train_table_unit_grad_multik", _guard_units("table_K12_D516_s0.5", True)),
    "table_unit_grad_eight_points": ("qsaek_train_table_unit_grad_multik", _guard_units("table_K12_D48_eight", True)),
    "table_unit_grad_split_lists": ("qsaek_train_table_unit_grad_multik", _guard_units("table_split_lists", True)),
}


@pytest.mark.parametrize("label", sorted(GUARD_CASES))
def test_entry_point_between_guard_words(label):
    entry, build = GUARD_CASES[label]
    call = build()
    assert call.entry == entry
    GU.run_call(call, _lib.load(), DEV)


# ---- the dispatcher ops ---------------------------------------------------------------------------------------------------
def test_dispatcher_ops():
    c = TrainCase("table_K12_D520_nobias")
    Q = torch.ops.qsae
    torch.library.opcheck(Q.decode_multik_table.default, (c.idx, c.val, c.table, c.step, None, c.ks))
    g = [c.g[0], None, c.g[2], c.g[3]]
    torch.library.opcheck(Q.train_row_grad_multik.default, (c.idx, c.table, c.step, g, c.ks, c.g_latent, c.W, True))
    G, gv, _ = ops.train_row_grad_multik(c.idx, c.table, c.step, g, c.ks, c.g_latent, None)
    torch.library.opcheck(Q.train_unit_grad_multik.default, (c.offsets, c.entries, c.val, gv, c.x, G, c.ks, c.logits, c.n_bits,
                                                              c.step, c.g_pol, True, True))
    torch.library.opcheck(Q.train_table_unit_grad_multik.default, (c.offsets, c.entries, c.val, gv, c.x, G, c.ks, True, True))


# ---- the two top-k model classes ----------------------------------------------------------------------------------------
D_, H_, K_, B_ = 48, 512, 6, 64
M_KS = [3, 6, 24]
CONFIG = {"input_dim": D_, "n_bits": 4, "hidden_dim": H_, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": K_,
          "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": B_}
KIND = {"baseline_sae": "baseline", "b_sae": "binary"}


def _model(kind: str, seed: int = 11, top_k: int = K_):
    if kind == "baseline":
        sd = S.baseline_sae_params(seed, D_, H_, bias_std=0.1)
        model = BaselineSparseAutoencoder(D_, H_)
        model.topk = top_k
    else:
        sd = S.binary_sae_params(seed, D_, H_, 4, dec_bias_std=0.1, logit_std=0.5)
        model = BinarySAE(D_, H_, gamma=4.0, n_bits=4)
        model.k = (top_k + 0.5) / H_
        assert model.top_k == top_k
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(DEV)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.fixture(scope="module")
def rows():
    return dev(S.activations(91, B_, D_))


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_forward_train_multi_topk_with_one_point_is_forward_train(sae_type, rows):
    """n_ks == 1 through the model: outputs and every .grad, bit for bit"""
    model = _model(KIND[sae_type])
    x = rows.clone().requires_grad_()
    out = model.forward_train(x)
    trainer_loss(sae_type, out, rows, CONFIG)
    want, want_x = _grads(model), x.grad.clone()
    model.zero_grad(set_to_none=True)
    x.grad = None
    multi = model.forward_train_multi_topk(x, [K_])
    assert isinstance(multi[1], tuple) and len(multi[1]) == 1 and len(multi) == len(out)
    same(multi[0], out[0], "latent")
    same(multi[1][0], out[1], "reconstruction")
    if sae_type == "b_sae":
        same(multi[2], out[2], "polarize")
    multi_topk_loss(sae_type, multi, rows, CONFIG)
    for k, g in _grads(model).items():
        same(g, want[k], k)
    same(x.grad, want_x, "x.grad")


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_every_point_is_the_model_rebuilt_with_that_top_k(sae_type, rows):
    model = _model(KIND[sae_type])
    model.activity = None
    latent, points, *rest = model.forward_train_multi_topk(rows, M_KS)
    assert len(points) == 3 and points[0]._base is points[2]._base and latent.shape == (B_, H_)
    assert int((latent != 0).sum(1).max()) <= M_KS[-1]      # the latent is the whole list's
    inf_latent, inf_points = model.forward_multi_topk(rows, M_KS)
    same(inf_latent, latent, "latent")
    for p, k in enumerate(M_KS):
        other = _model(KIND[sae_type], top_k=k)
        same(points[p], other.forward_train(rows)[1], f"training point {p} = forward_train at top_k = {k}")
        same(inf_points[p], other.forward_compact(rows)[2], f"point {p} = forward at top_k = {k}")
    # the gradient of the weighted loss against fp64 autograd on the same selection
    weights = [0.125, 1.0, 0.125]
    losses = multi_topk_loss(sae_type, (latent, points, *rest), rows, CONFIG, weights)
    assert losses.shape == (3,)
    got = _grads(model)
    lin = model.encoder.linear
    W = lin.weight.detach().cpu().double().requires_grad_()
    b = lin.bias.detach().cpu().double().requires_grad_()
    dec = model.decoder.weight.detach().cpu().double().requires_grad_()
    bd = model.decoder.bias.detach().cpu().double().requires_grad_()
    x64 = rows.cpu().double()
    ii = _model(KIND[sae_type], top_k=M_KS[-1]).forward_compact(rows)[0].cpu().long()    # the list, in rank order
    if sae_type == "baseline_sae":
        table, step, coef, pol = dec.t(), 1.0, 1.0, 0.0
    else:
        bw = 2.0 ** torch.arange(4, dtype=torch.float64)
        pw = bw.clone()
        bw[-1] = -bw[-1]
        pr = torch.sigmoid(dec).view(H_, D_, 4)
        table, step, coef = (pr * bw).sum(-1), model.decoder.quantization_step, 0.5
        pol = CONFIG["polarize_lambda"] * (pr * (1 - pr) * pw).mean()
    pre = (x64[:, None, :] * W[ii]).sum(-1) + b[ii]
    total = pol
    for p, k in enumerate(M_KS):
        recon = step * (pre[:, :k, None] * table[ii[:, :k]]).sum(1) + bd
        point_loss = coef * ((recon - x64) ** 2).mean()
        assert abs(float(losses[p]) - point_loss.item()) <= TOL * point_loss.item()
        total = total + weights[p] * point_loss
    total.backward()
    want = {"encoder.0.weight": W.grad, "encoder.0.bias": b.grad, "decoder.weight": dec.grad, "decoder.bias": bd.grad}
    assert sorted(got) == sorted(want)
    figures = {k: max_rel_err(got[k], want[k]) for k in want}
    print(sae_type, figures)
    assert all(v <= TOL for v in figures.values()), figures


def test_the_tracker_is_fed_with_the_ranks_below_the_models_top_k(rows):
    model = _model("baseline")
    calls = []

    class Spy:
        def add_compact(self, idx, val):
            calls.append((tuple(idx.shape), idx.is_contiguous(), idx.clone()))
    model.activity = Spy()
    _, points = model.forward_train_multi_topk(rows, M_KS)
    assert len(calls) == 1 and calls[0][0] == (B_, K_) and calls[0][1]
    same(calls[0][2], model.forward_compact(rows)[0], "the model's own selection")
    saved = points[0]._base.grad_fn.saved_tensors
    assert len(saved) == 4 and sorted(tuple(t.shape) for t in saved) == sorted([(B_, D_), (B_, 24), (B_, 24), (H_, D_)])
    for bad in ([], [6, 6, 24], [24, 6], [0, 24], [6, 513]):
        with pytest.raises(ValueError, match="ks|points"):
            model.forward_train_multi_topk(rows, bad)
    with pytest.raises(ValueError, match="expected \\[batch"):
        model.forward_multi_topk(rows[:, :8], M_KS)


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_twenty_trainer_steps_give_the_same_parameters_twice(sae_type, rows, tmp_path):
    def run():
        torch.manual_seed(5)                                  # the epoch's row order comes from the default generator
        logs = []
        model = _model(KIND[sae_type])
        if sae_type == "baseline_sae":
            model.normalize_decoder_weights()
        t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path),
                    log_fn=logs.append, log_every=1, multi_topk="default", activity_window=B_, aux_k=4)
        assert t.multi_topk == [K_, 4 * K_] and t.multi_topk_weights == [1.0, 0.125]
        for _ in range(20):                                   # one batch per call: the chunk is one batch of B_ rows
            t.one_epoch(rows)
        return {k: v.detach().clone() for k, v in model.state_dict().items()}, logs
    first, logs = run()
    second, _ = run()
    for k in first:
        same(first[k], second[k], k)
    m = logs[0]
    assert {f"recon_loss_k{K_}", f"recon_loss_k{4 * K_}", "recon_loss", "aux_loss"} <= set(m)
    assert m["recon_loss"] == m[f"recon_loss_k{K_}"]
    objective = m[f"recon_loss_k{K_}"] + 0.125 * m[f"recon_loss_k{4 * K_}"]
    pol = CONFIG["polarize_lambda"] * m["polarize_loss"] if sae_type == "b_sae" else 0.0
    assert abs(m["loss"] - objective - pol) <= 1e-6 * abs(m["loss"])
    assert logs[-1][f"recon_loss_k{K_}"] < logs[0][f"recon_loss_k{K_}"]
    assert all(torch.isfinite(v).all() for v in first.values() if v.is_floating_point())


@pytest.mark.parametrize("sae_type", ["baseline_sae", "b_sae"])
def test_one_point_through_the_trainer_is_the_plain_trainer(sae_type, rows, tmp_path):
    """``multi_topk=[top_k]`` (one point, weight 1) and the default ``None`` leave the same parameters after three steps"""
    def run(**kw):
        torch.manual_seed(5)                                  # the epoch's row order comes from the default generator
        model = _model(KIND[sae_type])
        t = Trainer(CONFIG, sae_type, False, True, model=model, dataset_dir=str(tmp_path), save_dir=str(tmp_path), **kw)
        for _ in range(3):
            t.one_epoch(rows)
        return {k: v.detach().clone() for k, v in model.state_dict().items()}
    plain, one_point = run(), run(multi_topk=[K_])
    for k in plain:                                          # one point with weight 1 is the plain objective, bit for bit
        same(one_point[k], plain[k], k)
