"""The sparsity-fidelity curve on the GPU (csrc/sparsity_curve.hip, quantizedsae_amd.inference.sparsity_curve): the kernel bit
for bit against the numpy restatement of tests/sparsity_curve_util.py (``sums``, ``counts``, ``recon_out``) -- both sides
perform the same IEEE operations in the same order and the library is built without contracted multiply-adds, so the
tolerance is zero -- and every point's reconstruction ``torch.equal`` to the existing sparse decoder on the truncated lists;
two calls cut at a group boundary against one; ``SparsityCurve`` on the two top-k model classes against the model rebuilt
with ``top_k = k'`` and run through ``evaluate_dataset``'s route; the reference's own forward at four k' (tests/golden/
sparsity_curve_*.npz, tools/gen_golden_sparsity_curve.py); both entry points between guard words; and the dispatcher op."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard_util as GU  # noqa: E402
import sparsity_curve_util as U  # noqa: E402
from guard_util import STREAM, WS, WS_BYTES, Buf, Call, HostArray  # noqa: E402
from quantizedsae_amd import _lib, ops, synthetic as S  # noqa: E402
from quantizedsae_amd import torch_ops  # noqa: E402
from quantizedsae_amd.inference import DatasetMoments, SparsityCurve, sparsity_curve  # noqa: E402
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64
GOLDEN = Path(__file__).resolve().parent / "golden"


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t) -> np.ndarray:
    return t.detach().cpu().numpy()


def same(got, want, what=""):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gb, wb = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
    assert np.array_equal(gb, wb), f"{what}: {int((gb != wb).sum())} bytes differ"


def dev_decoder(decoder):
    """the host form of tests/sparsity_curve_util.py -> the front end's decoder description on the device"""
    if decoder[0] == "packed":
        return "packed", dev(decoder[1]), decoder[3], decoder[4]
    return "table", dev(decoder[1]), decoder[2]


def state(n_ks):
    return torch.zeros((n_ks,), dtype=F64, device=DEV), torch.zeros((2,), dtype=I64, device=DEV)


def run(case, mod=ops, want_recon=True):
    x, idx, val, ks, decoder, bias, group_rows = case
    sums, counts = state(len(ks))
    recon = torch.full((len(ks),) + x.shape, float("nan"), dtype=F32, device=DEV) if want_recon else None
    mod.prefix_errors(dev(x), dev(idx), dev(val), ks, dev_decoder(decoder), None if bias is None else dev(bias), group_rows, sums,
                      counts, recon)
    return sums, counts, recon


def sparse_decode(idx, val, decoder, bias, D):
    if decoder[0] == "packed":
        return ops.decode_binary_sparse(idx, val, decoder[1], D, decoder[2], decoder[3], bias)
    return ops.decode_table_sparse(idx, val, decoder[1], decoder[2], bias)


def check(case):
    """kernel == restatement bit for bit, on both front ends, and every point == the existing sparse decoder"""
    x, idx, val, ks, decoder, bias, group_rows = case
    wsums, wcounts, wrecons = U.prefix_errors(x, idx, val, ks, decoder, bias, group_rows)
    for mod in (ops, torch_ops):
        sums, counts, recon = run(case, mod)
        same(sums, wsums, "sums")
        same(counts, wcounts, "counts")
        same(recon, wrecons, "recon_out")
    sums2, counts2, _ = run(case, want_recon=False)                        # without recon_out, and a second run: the same bits
    same(sums2, wsums, "sums without recon_out")
    same(counts2, wcounts, "counts without recon_out")
    H = decoder[1].shape[0]
    if ((idx >= 0) & (idx < H)).all():
        dd, db = dev_decoder(decoder), None if bias is None else dev(bias)
        for i, k in enumerate(ks):
            if k == 0:
                continue                                                    # the decoders take k >= 1
            got = sparse_decode(dev(idx[:, :k]).contiguous(), dev(val[:, :k]).contiguous(), dd, db, x.shape[1])
            assert torch.equal(recon[i], got), f"point k' = {k} differs from the sparse decoder"
    return recon


# ---- the kernel against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_kernel_equals_the_restatement_and_the_sparse_decoder(name):
    check(U.build_case(name))


@pytest.mark.parametrize("name", sorted(U.SPECIAL_CASES))
def test_special_values(name):
    case = U.special_case(name)
    recon = check(case)
    U.check_special(name, case, host(recon))


def test_ks_zero_without_a_bias_is_plus_zero():
    _, _, recon = run(U.build_case("table_one_point_0_no_bias"))
    assert not host(recon).view(np.uint32).any()


@pytest.mark.parametrize("name", ["packed_B10_nan", "table_B10_nan"])
def test_two_calls_cut_at_a_group_boundary_give_the_bits_of_one(name):
    x, idx, val, ks, decoder, bias, group_rows = U.build_case(name)
    one_s, one_c, _ = run((x, idx, val, ks, decoder, bias, group_rows), want_recon=False)
    sums, counts = state(len(ks))
    dd, db = dev_decoder(decoder), dev(bias)
    for r0, r1 in ((0, 2 * group_rows), (2 * group_rows, x.shape[0])):
        ops.prefix_errors(dev(x[r0:r1]), dev(idx[r0:r1]), dev(val[r0:r1]), ks, dd, db, group_rows, sums, counts)
    same(sums, host(one_s), "sums")
    same(counts, host(one_c), "counts")
    assert host(counts).tolist() == [6, 4]


def test_front_end_validation():
    x, idx, val, ks, decoder, bias, group_rows = U.build_case("table_B1")
    xd, idd, vd, dd = dev(x), dev(idx), dev(val), dev_decoder(decoder)
    sums, counts = state(len(ks))
    for bad in ([3, 1, 8], [1, 1], [-1, 2], [1, 9], list(range(17)), []):
        s, c = state(max(len(bad), 1))
        with pytest.raises(ValueError):
            ops.prefix_errors(xd, idd, vd, bad, dd, None, group_rows, s, c)
    with pytest.raises(ValueError, match="state"):
        ops.prefix_errors(xd, idd, vd, ks, dd, None, group_rows, sums[:2], counts)
    with pytest.raises(ValueError, match="recon_out"):
        ops.prefix_errors(xd, idd, vd, ks, dd, None, group_rows, sums, counts, torch.empty((1, 1, 36), dtype=F32, device=DEV))
    with pytest.raises(ValueError, match="group_rows"):
        ops.prefix_errors(xd, idd, vd, ks, dd, None, 0, sums, counts)
    with pytest.raises(ValueError, match="decoder"):
        ops.prefix_errors(xd, idd, vd, ks, ("dense", dd[1]), None, group_rows, sums, counts)
    assert not host(sums).any() and not host(counts).any()
    ops.prefix_errors(xd[:0], idd[:0], vd[:0], ks, dd, None, group_rows, sums, counts)           # no rows: nothing happens
    assert not host(sums).any() and not host(counts).any()


# ---- the model route --------------------------------------------------------------------------------------------------
MODEL_H, MODEL_D = 4096, 512
MODEL_KS = [1, 8, 32, 64]
#: (hidden_dim, rows, path): the issue's two shapes -- at hidden_dim 4096 no batch size reaches the prefilter (its kernels
#: start at 8192 units), so 4096 rows and 96 rows both select in place there -- and the smallest shape that does reach it
MODEL_SHAPES = [(4096, 4096, "inplace"), (4096, 96, "inplace"), (8192, 2048, "prefilter")]


def _model(kind: str, H: int = MODEL_H):
    if kind == "baseline":
        sd = S.baseline_sae_params(31, MODEL_D, H, bias_std=0.1)
        model = BaselineSparseAutoencoder(MODEL_D, H)
    else:
        # "hard": saturated logits (the packed dictionary); "soft": bell-shaped logits decoded through the soft table
        sd = S.binary_sae_params(31, MODEL_D, H, 4, dec_bias_std=0.1, logit_std=None if kind == "hard" else 0.5)
        model = BinarySAE(MODEL_D, H, gamma=4.0, n_bits=4)
        model.decoder.decode_mode = kind
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(DEV).eval()


def _set_k(model, k: int) -> None:
    if isinstance(model, BinarySAE):
        model.k = (k + 0.5) / model.hidden_dim
        assert model.top_k == k
    else:
        model.topk = k


@pytest.fixture(scope="module")
def model_rows():
    x = S.activations(77, 4096, MODEL_D)
    x[1500, 7] = np.nan                                      # one group of 1024 rows is skipped
    return dev(x)


@pytest.mark.parametrize("H,rows,path", MODEL_SHAPES)
@pytest.mark.parametrize("kind", ["hard", "soft", "baseline"])
def test_curve_equals_the_model_rebuilt_at_every_k(kind, H, rows, path, model_rows):
    """Both sides sum the same N = rows * D non-negative fp32 terms in fp64, in different orders: each partial sum is below
    sse and every addition rounds by at most 2^-53 of it, so the two differ by less than N * 2^-52 * sse."""
    model = _model(kind, H)
    x = model_rows[:rows] if rows >= 2048 else model_rows[2000:2000 + rows]
    group_rows = 1024 if rows >= 2048 else 32
    assert model.resolved_latent_path(rows) == path
    curve = SparsityCurve(model, ks=MODEL_KS, group_rows=group_rows)
    assert curve._path(rows, MODEL_KS[-1]) == path
    curve.add(x)
    r = curve.finish()
    assert r["ks"] == MODEL_KS and r["model_k"] == (32 if kind == "baseline" else int(H * 0.002))
    assert r["skipped_rows"] == (1024 if rows >= 2048 else 0) and r["rows"] == rows - r["skipped_rows"]
    for i, k in enumerate(MODEL_KS):
        _set_k(model, k)
        moments = DatasetMoments(MODEL_D, group_rows, DEV)
        with torch.no_grad():
            recon = model.forward_compact(x)[2]              # what SAEWrapper.reconstruct returns for these classes
        moments.add(x, recon)
        m = moments.finish()
        assert (m["rows"], m["skipped_rows"]) == (r["rows"], r["skipped_rows"])
        N = m["rows"] * MODEL_D
        sse = m["mse"] * N
        bound = N * 2.0 ** -52 * sse
        print(f"{kind} rows {rows} k' {k}: sse {r['sse'][i]!r} against {sse!r}, bound {bound:.3e}")
        assert abs(r["sse"][i] - sse) <= bound, (k, r["sse"][i], sse, bound)
        assert abs(r["variance"] - m["variance"]) <= 1e-12 * abs(m["variance"])
        assert abs(r["fvu"][i] - m["fvu"]) <= 1e-9 * m["fvu"] and abs(r["mse"][i] - m["mse"]) <= 1e-9 * m["mse"]
    # k_at: the smallest listed k at or below the target (the synthetic dictionaries are untrained: the curve need not fall)
    for target in (r["mse"][2], r["mse"].min(), r["mse"].max()):
        assert curve.k_at(mse=target) == next(k for k, v in zip(MODEL_KS, r["mse"]) if v <= target)
    assert curve.k_at(fvu=r["fvu"][1]) == next(k for k, v in zip(MODEL_KS, r["fvu"]) if v <= r["fvu"][1])
    assert curve.k_at(fvu=r["fvu"].min() / 2) is None and curve.k_at(mse=r["mse"].min() / 2) is None
    with pytest.raises(ValueError):
        curve.k_at()


def test_reconstructions_of_the_model_route_are_the_models_bits(model_rows):
    """recon_out of SparsityCurve.add at k' = the model's own k is forward_compact's reconstruction, bit for bit."""
    for kind in ("hard", "baseline"):
        model = _model(kind)
        x = model_rows[:2048]
        k = 8 if kind == "hard" else 32
        curve = SparsityCurve(model, ks=[1, k, 64], group_rows=1024)
        out = torch.empty((3, 2048, MODEL_D), dtype=F32, device=DEV)
        curve.add(x, recon_out=out)
        keep = torch.ones(2048, dtype=torch.bool, device=DEV)
        keep[1500] = False                                   # the NaN row: NaN != NaN
        assert torch.equal(out[1][keep], model.forward_compact(x)[2][keep])


def test_sparsity_curve_over_a_loader_equals_add_per_batch(model_rows):
    model = _model("hard")
    batches = [model_rows[:2048], model_rows[2048:3072], model_rows[3072:]]
    r = sparsity_curve(model, batches, ks=MODEL_KS)
    curve = SparsityCurve(model, ks=MODEL_KS)
    curve.add(model_rows)
    one = curve.finish()
    assert r["rows"] == one["rows"] == 3072 and r["skipped_rows"] == 1024
    assert np.array_equal(r["sse"].view(np.uint64), one["sse"].view(np.uint64))      # cut at multiples of group_rows
    with pytest.raises(ValueError, match="empty"):
        sparsity_curve(model, [])


# ---- the reference's own forward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["binary", "baseline"])
def test_reference_goldens(variant):
    """recon_out within 1e-5 of the row's largest |x| and the MSE within 1e-5 relative, on every row (the generator asserts
    that no listed k' sits on a near-tie of any row)."""
    z = np.load(GOLDEN / f"sparsity_curve_{variant}.npz")
    ks = [int(k) for k in z["ks"]]
    D, H, n_bits, seed, rows = (int(z[k]) for k in ("D", "H", "n_bits", "seed", "rows"))
    x = S.activations(seed, rows, D)
    assert float(z["min_gap"]) >= 4e-6
    if variant == "binary":
        sd = S.binary_sae_params(seed, D, H, n_bits, dec_bias_std=0.1)
        model = BinarySAE(D, H, gamma=4.0, n_bits=n_bits)
    else:
        sd = S.baseline_sae_params(seed, D, H, bias_std=0.1)
        model = BaselineSparseAutoencoder(D, H)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(DEV).eval()
    curve = SparsityCurve(model, ks=ks, group_rows=rows)
    out = torch.empty((len(ks), rows, D), dtype=F32, device=DEV)
    curve.add(dev(x), recon_out=out)
    r = curve.finish()
    got, want = host(out).astype(np.float64), z["recons"].astype(np.float64)
    scale = np.abs(x).max(axis=1)[None, :, None]
    assert (np.abs(got - want) <= 1e-5 * scale).all(), float((np.abs(got - want) / scale).max())
    for i in range(len(ks)):
        assert abs(r["mse"][i] - z["mse"][i]) <= 1e-5 * z["mse"][i], (ks[i], r["mse"][i], z["mse"][i])
        row_mse = ((got[i] - x) ** 2).mean(axis=1)
        ref_row = ((want[i] - x) ** 2).mean(axis=1)
        assert (np.abs(row_mse - ref_row) <= 1e-5 * ref_row).all()


# ---- both entry points between guard words ----------------------------------------------------------------------------------
def _guard(name, x_offset_bytes):
    def build():
        x, idx, val, ks, decoder, bias, group_rows = U.build_case(name)
        B, D = x.shape
        K, H, n = idx.shape[1], decoder[1].shape[0], len(ks)
        wsums, wcounts, wrecons = U.prefix_errors(x, idx, val, ks, decoder, bias, group_rows)
        packed = decoder[0] == "packed"

        def front(t):
            sums, counts = t["sums"], t["counts"]
            recon = torch.empty((n, B, D), dtype=F32, device=DEV)
            dd = ("packed", t["dict"], decoder[3], decoder[4]) if packed else ("table", t["dict"], decoder[2])
            ops.prefix_errors(t["x"], t["idx"], t["val"], ks, dd, t.get("bias"), group_rows, sums, counts, recon)
            return {"sums": sums, "counts": counts, "recon": recon}
        dict_args = [Buf("dict", "in", dev(decoder[1])), H, D] + ([decoder[3], decoder[4]] if packed else [decoder[2]])
        entry = "qsaec_prefix_errors_binary" if packed else "qsaec_prefix_errors_table"
        return Call(name, entry,
                    [Buf("x", "in", dev(x), offset_bytes=x_offset_bytes), Buf("idx", "in", dev(idx)), Buf("val", "in", dev(val)), B, K,
                     *dict_args, Buf("bias", "in", dev(bias)) if bias is not None else None, HostArray(ks), n, group_rows,
                     Buf("sums", "inout", torch.zeros((n,), dtype=F64, device=DEV)),
                     Buf("counts", "inout", torch.zeros((2,), dtype=I64, device=DEV)),
                     Buf("recon", "out", shape=(n, B, D), dtype=F32, offset_bytes=x_offset_bytes), WS, WS_BYTES, STREAM],
                    front, sizer=(entry + "_workspace_bytes", (B, n, group_rows)),
                    expect={"sums": torch.from_numpy(wsums), "counts": torch.from_numpy(wcounts), "recon": torch.from_numpy(wrecons)})
    return build


#: label -> (entry point, builder of its guard_util.Call); tests/test_sparsity_curve_host.py reads the entry points for its
#: ledger.  Building a case touches the GPU; importing this table does not.  x (and recon_out) start 4 bytes off a 16-byte
#: boundary in the tile-tail cases: the contract asks 4-byte alignment of them.
GUARD_CASES = {
    "binary_minimal": ("qsaec_prefix_errors_binary", _guard("packed_D4_n1", 0)),
    "binary_tile_tails": ("qsaec_prefix_errors_binary", _guard("packed_B10_nan", 4)),
    "binary_wide_row_tail": ("qsaec_prefix_errors_binary", _guard("packed_D1028_n2", 4)),
    "table_minimal": ("qsaec_prefix_errors_table", _guard("table_D4_s1.0_b0", 0)),
    "table_tile_tails": ("qsaec_prefix_errors_table", _guard("table_B10_nan", 4)),
    "table_wide_row_tail": ("qsaec_prefix_errors_table", _guard("table_D1028_s0.5_b1", 4)),
}


@pytest.mark.parametrize("label", sorted(GUARD_CASES))
def test_entry_point_between_guard_words(label):
    entry, build = GUARD_CASES[label]
    call = build()
    assert call.entry == entry
    GU.run_call(call, _lib.load(), DEV)


# ---- the dispatcher op ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["packed_B10_nan", "table_B10_nan"])
def test_dispatcher_op(name):
    x, idx, val, ks, decoder, bias, group_rows = U.build_case(name)
    dd = dev_decoder(decoder)
    sums, counts = state(len(ks))
    recon = torch.zeros((len(ks),) + x.shape, dtype=F32, device=DEV)
    n_bits, mult = (dd[2], dd[3]) if dd[0] == "packed" else (0, dd[2])
    args = (dev(x), dev(idx), dev(val), ks, dd[1], n_bits, mult, dev(bias), group_rows, sums, counts, recon)
    torch.library.opcheck(torch.ops.qsae.prefix_errors.default, args)
    torch.library.opcheck(torch.ops.qsae.prefix_errors.default, args[:-1] + (None,))
