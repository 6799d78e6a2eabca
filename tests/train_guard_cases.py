"""The case table of tests/test_train_guards_gpu.py: one builder per C-ABI entry point of csrc/train.hip, csrc/train_gemm.hip
and csrc/train_mask.hip (the ``*_workspace_bytes`` sizers are used, not tabled).  A builder takes a shape name and returns
the valid calls (guard_util.Call) that cover the entry point at that shape: its nullable operands, and every kernel form the
entry chooses between.  Roles follow the comments in include/qsae.h.

Shapes -- the smallest at which these kernels can go wrong, not the workload's (kernel tiles are 128 x 128 x 32):
* ``minimal``: B = 1, D = 4, H = 4 (32 where the entry takes H % 32), k = 1, one level; masks D x H = 2 x 2.
* ``tails``: B = 129 (a second M tile of one row; a K tail of 1 behind four full slices in the TN contractions), D = 132 (a
  second tile of 4, D % 32 = 4), H = 1060 (1056 where H % 32 is required), k = 65, n_bits = 4, and for the level-wise entries
  the padded layout of a 1000-unit matryoshka model (levels 125, 125, 250, 500 in slots of 128, 128, 256, 512).

Inputs are quantizedsae_amd.synthetic streams at fixed seeds; index inputs (top-k lists, CSR lists, z bits, masks) come from
the package's own front end on those inputs.  Importing this module touches no GPU: the builders do.
"""
from __future__ import annotations

import numpy as np
import torch

from quantizedsae_amd import ops, synthetic as S
from quantizedsae_amd.sae.quantized_matryoshka import _pad32, nested_sizes

from guard_util import STREAM, WS, WS_BYTES, Buf, Call, HostArray

DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32
SHAPES = ("minimal", "tails")
DIMS = {
    "minimal": dict(B=1, D=4, H=4, H32=32, k=1, n_bits=1, units=[32], mask=(2, 2)),
    "tails": dict(B=129, D=132, H=1060, H32=1056, k=65, n_bits=4, units=nested_sizes(1000, 4), mask=(132, 1060)),
}
assert DIMS["tails"]["units"] == [125, 125, 250, 500]


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def normal(seed, shape, stream, std=1.0) -> torch.Tensor:
    return dev(S.normal(seed, shape, stream=stream, std=std))


def In(name, t):
    return Buf(name, "in", data=t)


def InOut(name, t):
    return Buf(name, "inout", data=t)


def Out(name, shape, dtype=F32):
    return Buf(name, "out", shape=tuple(shape), dtype=dtype)


# ---- shared inputs -------------------------------------------------------------------------------------------------------
def topk_inputs(seed, B, D, H, k):
    """x, the encoder, an incoming reconstruction / latent gradient, and the top-k lists of the encoder's pre-activation."""
    x = dev(S.activations(seed, B, D))
    W = dev(S.xavier_uniform(seed, H, D, stream=1))
    b = normal(seed, (H,), 3, 0.1)
    Ht = H - H % 4                                  # topk_rows takes H % 4 == 0: the last H % 4 units are never selected
    idx, val = ops.topk_rows(ops.encode_dense(x, W[:Ht], b[:Ht], ops.ACT_NONE), k, False)
    assert int(idx.min()) >= 0 and int(idx.max()) < Ht
    return dict(x=x, W=W, b=b, idx=idx, val=val, gR=normal(seed, (B, D), 11), gL=normal(seed, (B, H), 12),
                table=normal(seed, (H, D), 13))


def matryoshka_inputs(seed, B, D, units, abs_range=4.0):
    """A matryoshka model of sum(units) hidden units in the packed order the kernels take: every level padded to a multiple of
    32 slots, index[slot] = the unit of a slot or -1 (None when nothing is padded), as QuantizedMatryoshkaDecoder lays it out."""
    n = len(units)
    sizes = [_pad32(u) for u in units]
    Hu, Hs = sum(units), sum(sizes)
    w = dev(S.uniform(seed, (Hu, D), -1.0, 1.0, stream=2))
    wm = dev(S.uniform(seed, (Hu, D), -1.0, 1.0, stream=5))
    index = None
    wp, wmp = w, wm
    W = dev(S.xavier_uniform(seed, Hs, D, stream=1))
    b = torch.zeros((Hs,), device=DEV)
    if sizes != list(units):
        parts, start = [], 0
        for u, p in zip(units, sizes):
            parts += [torch.arange(start, start + u), torch.full((p - u,), -1, dtype=torch.long)]
            start += u
        idx64 = torch.cat(parts).to(DEV)
        valid = idx64 >= 0
        wp = torch.zeros((Hs, D), device=DEV)
        wmp = -torch.ones((Hs, D), device=DEV)                  # S = 0 on pad slots
        wp[valid], wmp[valid] = w[idx64[valid]], wm[idx64[valid]]
        W[~valid], b[~valid] = 0.0, -1.0                        # an inert pad slot: z = 0
        index = idx64.to(I32)
    x = dev(S.activations(seed, B, D))
    pre = ops.encode_dense(x, W, b, ops.ACT_NONE)
    zbits = ops.train_pre_bits(pre)
    _, scale = ops.pack_matryoshka(wp, wmp, n, abs_range, sizes)
    counts = ops.activation_counts_bits(zbits)
    n_entries = int(counts.sum())
    assert n_entries >= 1
    return dict(B=B, D=D, n=n, units=list(units), sizes=sizes, Hu=Hu, Hs=Hs, w=w, wm=wm, index=index, x=x, pre=pre, zbits=zbits,
                scale=scale, counts=counts, n_entries=n_entries, sign_rows=ops.train_matryoshka_sign_rows(w, wm, index),
                G=normal(seed, (n, B, D), 11), gg=normal(seed, (n,), 12))


def ternary_inputs(seed, B, D, H):
    sd = S.ternary_sae_params(seed, D, H)
    x = dev(S.activations(seed, B, D))
    w = dev(sd["decoder.weight"])
    h = ops.encode_dense(x, dev(sd["encoder.0.weight"]), dev(sd["encoder.0.bias"]), ops.ACT_RELU)
    wm, mask = w.clone(), torch.ones_like(w)
    ops.train_mask_init(wm, mask, int(0.7 * D * H))
    return dict(w=w, h=h, mask=mask, t_rows=ops.train_ternary_rows(w), G=normal(seed, (B, D), 11), gh=normal(seed, (B, H), 12))


def blatent_inputs(seed, B, D, H):
    from quantizedsae_amd.sae.binary_latent import _GE_HALF_CUTOFF
    x = dev(S.activations(seed, B, D))
    W = dev(S.xavier_uniform(seed, H, D, stream=1))
    pre = ops.encode_dense(x, W, normal(seed, (H,), 3, 0.1), ops.ACT_NONE)
    _, zbits = ops.blatent_binarize(pre, _GE_HALF_CUTOFF)
    return dict(pre=pre, zbits=zbits, cutoff=_GE_HALF_CUTOFF, G=normal(seed, (B, D), 11),
                w_dec=dev(S.uniform(seed, (D, H), -0.1, 0.1, stream=2)))


# ---- train.hip -----------------------------------------------------------------------------------------------------------
def soft_table_polarize(shape):
    d = DIMS[shape]
    H, D, n = d["H"], d["D"], d["n_bits"]
    logits = normal(1101, (H, D * n), 2)

    def front(t):
        table, pol = ops.binary_soft_table_polarize(t["logits"], D, n)
        return {"table": table, "polarize": pol}
    return [Call(f"H {H} D {D} n_bits {n}", "qsae_binary_soft_table_polarize",
                 [In("logits", logits), H, D, n, Out("table", (H, D)), Out("polarize", ()), WS, WS_BYTES, STREAM], front,
                 sizer=("qsae_binary_soft_table_polarize_workspace_bytes", (H, D)))]


def train_csr(shape):
    d = DIMS[shape]
    B, D, H, k = d["B"], d["D"], d["H"], d["k"]
    t = topk_inputs(1102, B, D, H, k)

    def front(p):
        offsets, entries = ops.train_csr(p["idx"], H)
        return {"offsets": offsets, "entries": entries}
    return [Call(f"B {B} k {k} H {H}", "qsae_train_csr",
                 [In("idx", t["idx"]), B, k, H, Out("offsets", (H + 1,), I32), Out("entries", (B * k,), I32), WS, WS_BYTES, STREAM],
                 front, sizer=("qsae_train_csr_workspace_bytes", (B, k, H)))]


def train_row_grad(shape):
    d = DIMS[shape]
    B, D, H, k = d["B"], d["D"], d["H"], d["k"]
    t = topk_inputs(1103, B, D, H, k)
    step = 0.25
    calls = []
    for want_dx in (True, False):
        def front(p, want_dx=want_dx):
            gv, dx = ops.train_row_grad(p["idx"], p["table"], step, p["g_recon"], p["g_latent"], p.get("W_enc"), want_dx)
            return {"gv": gv, "dx": dx} if want_dx else {"gv": gv}
        calls.append(Call(f"B {B} k {k} H {H} D {D} dx {want_dx}", "qsae_train_row_grad",
                          [In("idx", t["idx"]), B, k, In("table", t["table"]), H, D, step, In("g_recon", t["gR"]),
                           In("g_latent", t["gL"]), H, In("W_enc", t["W"]) if want_dx else None, Out("gv", (B, k)),
                           Out("dx", (B, D)) if want_dx else None, STREAM], front))
    return calls


def _unit_inputs(seed, d):
    B, D, H, k = d["B"], d["D"], d["H"], d["k"]
    t = topk_inputs(seed, B, D, H, k)
    t["offsets"], t["entries"] = ops.train_csr(t["idx"], H)
    t["gv"], _ = ops.train_row_grad(t["idx"], t["table"], 0.25, t["gR"], t["gL"], None, False)
    return t


def train_unit_grad(shape):
    d = DIMS[shape]
    B, D, H, k, n = d["B"], d["D"], d["H"], d["k"], d["n_bits"]
    t = _unit_inputs(1104, d)
    logits = normal(1104, (H, D * n), 2)
    gP = normal(1104, (), 14)
    step = 0.25
    calls = []
    for enc, lg in ((True, True), (True, False), (False, True)):
        def front(p, enc=enc, lg=lg):
            dW, db, dl = ops.train_unit_grad(p["offsets"], p["entries"], p["val"], p["gv"], p["x"], p["g_recon"], p["logits"], n,
                                             step, p["g_polarize"], enc, lg)
            out = {"dW_enc": dW, "db_enc": db} if enc else {}
            if lg:
                out["dlogits"] = dl
            return out
        calls.append(Call(f"B {B} k {k} H {H} D {D} n_bits {n} encoder {enc} logits {lg}", "qsae_train_unit_grad",
                          [In("offsets", t["offsets"]), In("entries", t["entries"]), In("val", t["val"]), In("gv", t["gv"]), B, k,
                           In("x", t["x"]), In("g_recon", t["gR"]), In("logits", logits), H, D, n, step, In("g_polarize", gP),
                           Out("dW_enc", (H, D)) if enc else None, Out("db_enc", (H,)) if enc else None,
                           Out("dlogits", (H, D * n)) if lg else None, WS, WS_BYTES, STREAM], front,
                          sizer=("qsae_train_unit_grad_workspace_bytes", (B, k, H, D))))
    return calls


def train_col_sum(shape):
    d = DIMS[shape]
    B, D = d["B"], d["D"]
    g = normal(1105, (B, D), 11)
    return [Call(f"B {B} D {D}", "qsae_train_col_sum", [In("g", g), B, D, Out("out", (D,)), WS, WS_BYTES, STREAM],
                 lambda p: {"out": ops.train_col_sum(p["g"])}, sizer=("qsae_train_col_sum_workspace_bytes", (B, D)))]


def table_unit_grad_form(dW_dec_ld) -> str:
    """qsae_train_table_unit_grad: the transposed store of dW_dec goes 16 bytes at a time when its rows allow it."""
    return "16-byte store" if dW_dec_ld % 4 == 0 else "element store"


def train_table_unit_grad(shape):
    """The nullable outputs and the nullable g_recon; H a multiple of 4 takes the 16-byte store of the transposed decoder
    gradient, H + 2 (6 and 1062) its element-wise store."""
    d = DIMS[shape]
    B, D, k = d["B"], d["D"], d["k"]
    calls = []
    for H, expect, variants in ((d["H"], "16-byte store", ((True, True, True), (True, False, True), (False, True, True),
                                                            (False, True, False))),
                                (d["H"] + 2, "element store", ((True, True, True),))):
        t = _unit_inputs(1106 + H, dict(d, H=H))
        for enc, dec, with_g in variants:
            def front(p, enc=enc, dec=dec):
                dW, db, dWd = ops.train_table_unit_grad(p["offsets"], p["entries"], p["val"], p["gv"], p["x"], p.get("g_recon"),
                                                        enc, dec)
                out = {"dW_enc": dW, "db_enc": db} if enc else {}
                if dec:
                    out["dW_dec"] = dWd
                return out
            calls.append(Call(f"B {B} k {k} H {H} D {D} encoder {enc} decoder {dec} g_recon {with_g}", "qsae_train_table_unit_grad",
                              [In("offsets", t["offsets"]), In("entries", t["entries"]), In("val", t["val"]), In("gv", t["gv"]), B,
                               k, In("x", t["x"]), In("g_recon", t["gR"]) if with_g else None, H, D,
                               Out("dW_enc", (H, D)) if enc else None, Out("db_enc", (H,)) if enc else None,
                               Out("dW_dec", (D, H)) if dec else None, H, WS, WS_BYTES, STREAM], front,
                              sizer=("qsae_train_table_unit_grad_workspace_bytes", (B, k, H, D)),
                              form=(expect, table_unit_grad_form(H))))
    return calls


def normalize_columns_table(shape):
    d = DIMS[shape]
    D, H = d["D"], d["H"]
    W = normal(1107, (D, H), 2)
    calls = []
    for want in (True, False):
        def front(p, want=want):
            table = ops.normalize_columns_table(p["W"], want)
            return {"W": p["W"], "table": table} if want else {"W": p["W"]}
        calls.append(Call(f"D {D} H {H} table {want}", "qsae_normalize_columns_table",
                          [InOut("W", W), D, H, Out("table", (H, D)) if want else None, STREAM], front))
    return calls


def train_ternary_rows(shape):
    d = DIMS[shape]
    D, H = d["D"], d["H"]
    w = normal(1108, (D, H), 2, 0.5)
    return [Call(f"D {D} H {H}", "qsae_train_ternary_rows", [In("w", w), D, H, Out("t_rows", (H, D)), STREAM],
                 lambda p: {"t_rows": ops.train_ternary_rows(p["w"])})]


def transpose_rows(shape):
    d = DIMS[shape]
    D, H = d["D"], d["H"]
    src = normal(1109, (H, D), 2)
    return [Call(f"H {H} D {D}", "qsae_transpose_rows", [In("src", src), H, D, Out("dst", (D, H)), STREAM],
                 lambda p: {"dst": ops.transpose_rows(p["src"])})]


def train_pre_bits(shape):
    d = DIMS[shape]
    B, H = d["B"], d["H32"]
    pre = normal(1110, (B, H), 2)
    return [Call(f"B {B} H {H}", "qsae_train_pre_bits", [In("pre", pre), H, B, H, Out("zbits", (B, H // 32), I32), H // 32, STREAM],
                 lambda p: {"zbits": ops.train_pre_bits(p["pre"])})]


def _matryoshka(shape, seed):
    d = DIMS[shape]
    return matryoshka_inputs(seed, d["B"], d["D"], d["units"])


def train_bits_csr(shape):
    m = _matryoshka(shape, 1111)
    B, H, n_e = m["B"], m["Hs"], m["n_entries"]

    def front(p):
        offsets, entries = ops.train_bits_csr(p["zbits"], H, n_e)
        return {"offsets": offsets, "entries": entries}
    return [Call(f"B {B} H {H} entries {n_e}", "qsae_train_bits_csr",
                 [In("zbits", m["zbits"]), H // 32, B, H, Out("offsets", (H + 1,), I32), Out("entries", (n_e,), I32), n_e, WS,
                  WS_BYTES, STREAM], front, sizer=("qsae_train_bits_csr_workspace_bytes", (B, H)))]


def train_matryoshka_dsum_lists(shape):
    m = _matryoshka(shape, 1112)
    B, D, H, n, n_e, sizes = m["B"], m["D"], m["Hs"], m["n"], m["n_entries"], m["sizes"]
    offsets, entries = ops.train_bits_csr(m["zbits"], H, n_e)
    return [Call(f"B {B} D {D} levels {sizes} entries {n_e}", "qsae_train_matryoshka_dsum_lists",
                 [In("offsets", offsets), In("entries", entries), n_e, In("g_levels", m["G"]), B, D, H, n, HostArray(sizes),
                  Out("dsum", (H, D)), WS, WS_BYTES, STREAM],
                 lambda p: {"dsum": ops.train_matryoshka_dsum_lists(p["offsets"], p["entries"], n_e, p["g_levels"], sizes)},
                 sizer=("qsae_train_matryoshka_dsum_lists_workspace_bytes", (B, n_e, H, D)))]


def _index_arg(m):
    return In("index", m["index"]) if m["index"] is not None else None


def train_matryoshka_sign_rows(shape):
    m = _matryoshka(shape, 1113)
    return [Call(f"units {m['Hu']} slots {m['Hs']} D {m['D']}", "qsae_train_matryoshka_sign_rows",
                 [In("w", m["w"]), In("wm", m["wm"]), _index_arg(m), m["Hs"], m["D"], Out("sign_rows", (m["Hs"], m["D"])), STREAM],
                 lambda p: {"sign_rows": ops.train_matryoshka_sign_rows(p["w"], p["wm"], p.get("index"))})]


def train_matryoshka_finish(shape):
    m = _matryoshka(shape, 1114)
    Hs, Hu, D = m["Hs"], m["Hu"], m["D"]
    dsum = ops.train_matryoshka_dsum_dense(m["zbits"], m["G"], Hs, m["sizes"])
    calls = []
    for with_dsum in (True, False):
        def front(p):
            dw, dwm = ops.train_matryoshka_finish(p.get("dsum"), p["scale"], p.get("index"), p["w"], p["wm"])
            return {"dweight": dw, "dweight_mirror": dwm}
        calls.append(Call(f"units {Hu} slots {Hs} D {D} dsum {with_dsum}", "qsae_train_matryoshka_finish",
                          [In("dsum", dsum) if with_dsum else None, In("scale", m["scale"]), _index_arg(m), In("w", m["w"]),
                           In("wm", m["wm"]), Hs, D, Out("dweight", (Hu, D)), Out("dweight_mirror", (Hu, D)), STREAM], front))
    return calls


def train_matryoshka_secant(shape):
    m = _matryoshka(shape, 1115)
    Hs, Hu, D = m["Hs"], m["Hu"], m["D"]
    c = 1.0 / (m["B"] * D)
    gw, gwm = normal(1115, (Hu, D), 21), normal(1115, (Hu, D), 22)

    def front(p):
        ops.train_matryoshka_secant(p["grad_weight"], p["grad_weight_mirror"], p["counts"], c, p["scale"], p.get("index"), p["w"],
                                    p["wm"])
        return {"grad_weight": p["grad_weight"], "grad_weight_mirror": p["grad_weight_mirror"]}
    return [Call(f"units {Hu} slots {Hs} D {D}", "qsae_train_matryoshka_secant",
                 [In("counts", m["counts"]), c, In("scale", m["scale"]), _index_arg(m), In("w", m["w"]), In("wm", m["wm"]), Hs, D,
                  InOut("grad_weight", gw), InOut("grad_weight_mirror", gwm), STREAM], front)]


# ---- train_gemm.hip ------------------------------------------------------------------------------------------------------
def dpre_form(g) -> str:
    """qsae_train_matryoshka_dpre / qsae_train_ternary_dpre: without an incoming reconstruction gradient there is nothing to
    contract, and an elementwise kernel writes the constant term."""
    return "constant kernel" if g is None else "matrix pipe"


def train_matryoshka_dpre(shape):
    m = _matryoshka(shape, 1116)
    B, D, H, n, sizes = m["B"], m["D"], m["Hs"], m["n"], m["sizes"]
    calls = []
    for with_levels, with_groups, expect in ((True, True, "matrix pipe"), (True, False, "matrix pipe"),
                                             (False, True, "constant kernel")):
        def front(p):
            return {"pre": ops.train_matryoshka_dpre(p["pre"], p.get("g_levels"), p.get("g_groups"), p["sign_rows"], p["scale"],
                                                     sizes)}
        calls.append(Call(f"B {B} D {D} levels {sizes} g_levels {with_levels} g_groups {with_groups}", "qsae_train_matryoshka_dpre",
                          [In("g_levels", m["G"]) if with_levels else None, In("g_groups", m["gg"]) if with_groups else None,
                           In("sign_rows", m["sign_rows"]), In("scale", m["scale"]), B, D, H, n, HostArray(sizes),
                           InOut("pre", m["pre"]), H, STREAM], front,
                          form=(expect, dpre_form(m["G"] if with_levels else None))))
    return calls


def train_gemm_tn(shape):
    d = DIMS[shape]
    K, M, N = d["B"], d["H"], d["D"]
    A, X = normal(1117, (K, M), 2), normal(1117, (K, N), 3)
    return [Call(f"K {K} M {M} N {N}", "qsae_train_gemm_tn", [In("A", A), M, In("X", X), N, K, M, N, Out("C", (M, N)), N, STREAM],
                 lambda p: {"C": ops.train_gemm_tn(p["A"], p["X"])})]


def dsum_dense_form(sizes) -> str:
    """qsae_train_matryoshka_dsum_dense: one launch over all levels when every level lies on 128-unit tiles."""
    return "one launch" if all(s % 128 == 0 for s in sizes) else "per level"


def train_matryoshka_dsum_dense(shape):
    """minimal: one level of 32 (per level).  tails: the padded 1000-unit layout -- its slots 128, 128, 256, 512 all lie on
    128-unit tiles, so it takes the one-launch form, as do four 128-unit levels (H = 512); the padded layout of 1056 units
    (160, 160, 288, 544) is the per-level form with a partial tile in every level."""
    d = DIMS[shape]
    layouts = [(d["units"], "per level" if shape == "minimal" else "one launch")]
    if shape == "tails":
        layouts += [([128, 128, 128, 128], "one launch"), (nested_sizes(1056, 4), "per level")]
    calls = []
    for i, (units, expect) in enumerate(layouts):
        m = matryoshka_inputs(1118 + i, d["B"], d["D"], units)
        B, D, H, n, sizes = m["B"], m["D"], m["Hs"], m["n"], m["sizes"]
        calls.append(Call(f"B {B} D {D} levels {sizes}", "qsae_train_matryoshka_dsum_dense",
                          [In("zbits", m["zbits"]), H // 32, In("g_levels", m["G"]), B, D, H, n, HostArray(sizes), Out("dsum", (H, D)),
                           STREAM],
                          lambda p, H=H, sizes=sizes: {"dsum": ops.train_matryoshka_dsum_dense(p["zbits"], p["g_levels"], H, sizes)},
                          form=(expect, dsum_dense_form(sizes))))
    return calls


def train_ternary_dpre(shape):
    d = DIMS[shape]
    B, D, H = d["B"], d["D"], d["H"]
    t = ternary_inputs(1119, B, D, H)
    calls = []
    for with_G, expect in ((True, "matrix pipe"), (False, "constant kernel")):
        for with_gh in (True, False):
            def front(p):
                return {"dpre": ops.train_ternary_dpre(p["h_act"], p.get("g_recon"), p.get("g_latent"), p["t_rows"])}
            calls.append(Call(f"B {B} D {D} H {H} g_recon {with_G} g_latent {with_gh}", "qsae_train_ternary_dpre",
                              [In("g_recon", t["G"]) if with_G else None, In("t_rows", t["t_rows"]),
                               In("g_latent", t["gh"]) if with_gh else None, In("h_act", t["h"]), B, D, H, Out("dpre", (B, H)), STREAM],
                              front, form=(expect, dpre_form(t["G"] if with_G else None))))
    return calls


def train_ternary_dweight(shape):
    d = DIMS[shape]
    B, D, H = d["B"], d["D"], d["H"]
    t = ternary_inputs(1120, B, D, H)
    return [Call(f"B {B} D {D} H {H}", "qsae_train_ternary_dweight",
                 [In("g_recon", t["G"]), In("h_act", t["h"]), In("mask", t["mask"]), B, D, H, Out("dweight", (D, H)), STREAM],
                 lambda p: {"dweight": ops.train_ternary_dweight(p["g_recon"], p["h_act"], p["mask"])})]


def blatent_binarize(shape):
    d = DIMS[shape]
    B, D, H = d["B"], d["D"], d["H32"]
    t = blatent_inputs(1121, B, D, H)
    calls = []
    for want in (True, False):
        def front(p, want=want):
            latent, zbits = ops.blatent_binarize(p["pre"], t["cutoff"], want)
            return {"latent": latent, "zbits": zbits} if want else {"zbits": zbits}
        calls.append(Call(f"B {B} H {H} latent {want}", "qsae_blatent_binarize",
                          [In("pre", t["pre"]), B, H, t["cutoff"], Out("latent", (B, H)) if want else None,
                           Out("zbits", (B, H // 32), I32), STREAM], front))
    return calls


def blatent_dpre_form(D) -> str:
    """qsae_train_blatent_dpre: the loader of g_recon that needs whole 32-wide K slices, or the one that clamps the K tail."""
    return "whole K slices" if D % 32 == 0 else "clamped K tail"


def train_blatent_dpre(shape):
    d = DIMS[shape]
    B, H = d["B"], d["H32"]
    calls = []
    for D, expect in ((d["D"], "clamped K tail"), (32 if shape == "minimal" else 160, "whole K slices")):
        t = blatent_inputs(1122 + D, B, D, H)
        calls.append(Call(f"B {B} D {D} H {H}", "qsae_train_blatent_dpre",
                          [In("g_recon", t["G"]), In("w_dec", t["w_dec"]), B, D, H, InOut("pre", t["pre"]), STREAM],
                          lambda p: {"pre": ops.train_blatent_dpre(p["pre"], p["g_recon"], p["w_dec"])},
                          form=(expect, blatent_dpre_form(D))))
    return calls


def train_blatent_dweight(shape):
    d = DIMS[shape]
    B, D, H = d["B"], d["D"], d["H32"]
    t = blatent_inputs(1123, B, D, H)
    return [Call(f"B {B} D {D} H {H}", "qsae_train_blatent_dweight",
                 [In("g_recon", t["G"]), In("zbits", t["zbits"]), H // 32, B, D, H, Out("dweight", (D, H)), STREAM],
                 lambda p: {"dweight": ops.train_blatent_dweight(p["g_recon"], p["zbits"], H)})]


# ---- train_mask.hip ------------------------------------------------------------------------------------------------------
def _mask_counts(shape, D, H):
    return (0, 1, D * H) if shape == "minimal" else (0, int(0.7 * D * H), D * H)


def train_mask_init(shape):
    D, H = DIMS[shape]["mask"]
    w = normal(1124, (D, H), 2, 0.5)
    calls = []
    for n in _mask_counts(shape, D, H):
        def front(p, n=n):
            ops.train_mask_init(p["w"], p["mask"], n)
            return {"w": p["w"], "mask": p["mask"]}
        calls.append(Call(f"D {D} H {H} n_inactive {n}", "qsae_train_mask_init",
                          [InOut("w", w), InOut("mask", torch.ones_like(w)), D, H, n, WS, WS_BYTES, STREAM], front,
                          sizer=("qsae_train_mask_workspace_bytes", (D, H))))
    return calls


def train_mask_update(shape):
    D, H = DIMS[shape]["mask"]
    w, mask = normal(1125, (D, H), 2, 0.5), torch.ones((D, H), device=DEV)
    ops.train_mask_init(w, mask, (D * H) // 2)
    a, delta = normal(1125, (H,), 5).abs(), normal(1125, (D,), 6, 1e-3)
    counts = (0, 1, D * H) if shape == "minimal" else (0, int(0.3 * 0.3 * D * H), D * H)
    calls = []
    for stats in (True, False):
        for n in counts:
            def front(p, n=n):
                ops.train_mask_update(p["w"], p["mask"], p.get("a"), p.get("delta"), n)
                return {"w": p["w"], "mask": p["mask"]}
            calls.append(Call(f"D {D} H {H} n {n} a / delta {stats}", "qsae_train_mask_update",
                              [InOut("w", w), InOut("mask", mask), In("a", a) if stats else None,
                               In("delta", delta) if stats else None, D, H, n, WS, WS_BYTES, STREAM], front,
                              sizer=("qsae_train_mask_workspace_bytes", (D, H))))
    return calls


#: C symbol -> builder(shape name) -> [Call]
CASES = {
    "qsae_binary_soft_table_polarize": soft_table_polarize,
    "qsae_train_csr": train_csr,
    "qsae_train_row_grad": train_row_grad,
    "qsae_train_unit_grad": train_unit_grad,
    "qsae_train_col_sum": train_col_sum,
    "qsae_train_table_unit_grad": train_table_unit_grad,
    "qsae_normalize_columns_table": normalize_columns_table,
    "qsae_train_ternary_rows": train_ternary_rows,
    "qsae_transpose_rows": transpose_rows,
    "qsae_train_pre_bits": train_pre_bits,
    "qsae_train_bits_csr": train_bits_csr,
    "qsae_train_matryoshka_dsum_lists": train_matryoshka_dsum_lists,
    "qsae_train_matryoshka_sign_rows": train_matryoshka_sign_rows,
    "qsae_train_matryoshka_finish": train_matryoshka_finish,
    "qsae_train_matryoshka_secant": train_matryoshka_secant,
    "qsae_train_matryoshka_dpre": train_matryoshka_dpre,
    "qsae_train_gemm_tn": train_gemm_tn,
    "qsae_train_matryoshka_dsum_dense": train_matryoshka_dsum_dense,
    "qsae_train_ternary_dpre": train_ternary_dpre,
    "qsae_train_ternary_dweight": train_ternary_dweight,
    "qsae_blatent_binarize": blatent_binarize,
    "qsae_train_blatent_dpre": train_blatent_dpre,
    "qsae_train_blatent_dweight": train_blatent_dweight,
    "qsae_train_mask_init": train_mask_init,
    "qsae_train_mask_update": train_mask_update,
}
