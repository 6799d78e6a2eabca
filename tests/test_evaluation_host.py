"""The evaluation reports without a GPU: the C ABI's symbols, workspace sizes and the argument checks that are answered
before any HIP call; the Python front-end's own errors; the numpy restatement (tests/evaluation_util.py) against what the
reference's own functions recorded (tests/golden/evaluation_*.npz, tools/gen_golden_evaluation.py), within the fp32
summation bound of the reference's sums plus the soft-side eps; the report's text; and what the planted inputs promise."""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import evaluation_util as U
from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, _lib, build
from quantizedsae_amd.inference import (DatasetMoments, estimate_baseline_error, evaluate_dataset,  # noqa: F401
                                        format_quantization_report, quantization_error)

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("qsae_quantization_error", "qsae_quantization_error_workspace_bytes", "qsae_dataset_moments_add",
         "qsae_dataset_moments_workspace_bytes")


def _golden(name):
    z = np.load(ROOT / "tests" / "golden" / f"evaluation_{name}.npz")
    return z, json.loads(bytes(z["meta"]).decode())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "qsae.h").read_text()
    lib = _lib.load()
    assert _lib.DEBUG_LIB_PATH.exists(), "build with `python -m quantizedsae_amd.build`"
    for exported in (build.exported_symbols(_lib.LIB_PATH), build.exported_symbols(_lib.DEBUG_LIB_PATH)):
        for name in NAMES:
            assert re.search(rf"\b{name}\(", header)
            assert name in _lib.SIGNATURES and name in exported
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "evaluation.hip" in build.SOURCES
    assert lib.qsae_abi_version() == _lib.ABI_VERSION == 4     # an additive change
    assert "#define QSAE_QUANT_ERROR_WORDS 48" in header


def _r256(v):
    return (v + 255) // 256 * 256


def test_workspace_helpers_return_the_documented_sizes():
    lib = _lib.load()
    q, m = lib.qsae_quantization_error_workspace_bytes, lib.qsae_dataset_moments_workspace_bytes
    for H, D, n in U.QUANT_CASES + [(32768, 512, 4), (32768, 512, 8)]:
        assert q(H, D, n) == _r256((11 + 3 * n) * H * 8)
    assert q(0, 4, 4) == q(4, 0, 4) == q(4, 4, 0) == q(4, 4, 9) == q(65536, 32768, 4) == 0
    for B, D, g in [(1, 4, 1024), (1025, 20, 1024), (3000, 516, 1024), (65536, 512, 1024), (70, 7, 16)]:
        G = (B + g - 1) // g
        assert m(B, D, g, 0) == _r256(2 * G * D * 8) + _r256(G * 4)
        assert m(B, D, g, 1) == _r256(3 * G * D * 8) + _r256(G * 4)
    assert m(-1, 4, 4, 0) == m(4, 0, 4, 0) == m(4, 4, 0, 0) == 0


def test_unsupported_sizes_are_answered_before_any_pointer_is_looked_at():
    lib = _lib.load()
    null = ctypes.c_void_p(0)

    def call(H, D, n):
        return lib.qsae_quantization_error(null, H, D, n, 1.0, 1.0, null, null, null, 0, null)
    assert call(4, 4, 9) == _lib.ERR_UNSUPPORTED and b"n_bits" in lib.qsae_last_error()
    assert call(4, 4, 0) == _lib.ERR_UNSUPPORTED
    assert call(65536, 32768, 4) == _lib.ERR_UNSUPPORTED and b"2^31" in lib.qsae_last_error()      # H D = 2^31: sizes only
    assert call(65536, 32767, 4) == _lib.ERR_INVALID_ARG                                            # supported; the null pointers
    assert call(0, 4, 4) == _lib.ERR_INVALID_ARG
    mom = lib.qsae_dataset_moments_add
    assert mom(null, 3, null, 4, 4, 4, null, null, null, 0, null) == _lib.ERR_UNSUPPORTED           # unknown dtype
    assert mom(null, 0, null, 4, 0, 4, null, null, null, 0, null) == _lib.ERR_INVALID_ARG
    assert mom(null, 0, null, 4, 4, 0, null, null, null, 0, null) == _lib.ERR_INVALID_ARG
    assert mom(null, 0, null, 0, 4, 4, null, null, null, 0, null) == _lib.OK                        # no rows: nothing to do
    assert mom(null, 0, null, 4, 4, 4, null, null, null, 0, null) == _lib.ERR_INVALID_ARG


# ---- the Python front-end -------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_other_models_raise():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quantization_error(BinarySAE(8, 16, n_bits=4))
    with pytest.raises(TypeError, match="BinarySAE"):
        quantization_error(BaselineSparseAutoencoder(8, 16))
    m = DatasetMoments(4, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(torch.zeros(3, 4))
    with pytest.raises(ValueError):
        m.add(torch.zeros(3, 5))
    with pytest.raises(ValueError, match="no row was kept"):
        m.finish()
    with pytest.raises(ValueError):
        DatasetMoments(4, group_rows=0, device="cpu")
    with pytest.raises(ValueError, match="empty"):
        estimate_baseline_error([])


def test_ops_are_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "Tensor(a3!) sums" in str(torch.ops.qsae.dataset_moments_add.default._schema)
    with FakeTensorMode():
        block, unit = torch.ops.qsae.quantization_error(torch.empty(7, 20 * 3), 20, 3, 0.5, 1.0)
        assert block.shape == (48,) and unit.shape == (7,) and block.dtype == unit.dtype == torch.float64
        assert torch.ops.qsae.dataset_moments_add(torch.empty(5, 4), None, 2, torch.empty(3, 4, dtype=torch.float64),
                                                  torch.empty(2, dtype=torch.int64)) is None


# ---- the restatement against the reference's numbers ----------------------------------------------------------------------
def _mean_bound(terms, soft, value):
    """|fp32 mean the reference computed - exact mean of our terms|: its fp32 sum in any order, one rounding per term (a
    square or an abs of fp32 values), our soft-side error per term, and the final fp32 division."""
    return (U.fp32_sum_bound(terms) + U.U24 * np.abs(terms).sum()) / terms.size + soft + 2 * U.U24 * abs(value)


@pytest.mark.parametrize("kind", ["kaiming", "polarised"])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_restatement_reproduces_the_reference_numbers(kind, n):
    z, meta = _golden("quantization")
    case = next(c for c in meta["cases"] if c["name"] == f"{kind}_n{n}")
    H, D, step = meta["H"], meta["D"], case["step"]
    assert step == U.step_of(n, meta["gamma"])
    logits = z[f"{kind}_n{n}_logits"]
    eps, N = U.eps_of(n, step), H * D
    wf, wq, diff = U.entries(logits, D, n, step)            # the kernel's fp32 chain on this machine's expf
    got = U.quant_restate(logits, D, n, step)
    s, e = case["stats"], case["entry"]
    sq = lambda v: 2 * np.abs(v).max() * eps + eps * eps     # noqa: E731
    assert abs(s["mse"] - got["sums"][0] / N) <= _mean_bound(diff * diff, sq(diff), s["mse"])
    assert abs(s["mean_abs"] - got["sums"][1] / N) <= _mean_bound(np.abs(diff), eps, s["mean_abs"])
    assert abs(s["max_abs"] - got["max_abs"]) <= eps
    assert abs(s["l2_norm"] ** 2 - got["sums"][0]) <= N * _mean_bound(diff * diff, sq(diff), s["mse"]) + 4 * U.U24 * s["l2_norm"] ** 2
    for prefix, v, soft in (("float", wf, eps), ("quant", wq, 0.0)):
        total, total2 = got["sums"][2 if prefix == "float" else 4], got["sums"][3 if prefix == "float" else 5]
        assert abs(s[f"{prefix}_mean"] - total / N) <= _mean_bound(v, soft, s[f"{prefix}_mean"])
        assert abs(s[f"{prefix}_min"] - v.min()) <= soft and abs(s[f"{prefix}_max"] - v.max()) <= soft
        sq_soft = (2 * np.abs(v).max() * soft + soft * soft)
        assert abs(s[f"{prefix}_l2_norm"] ** 2 - total2) <= N * _mean_bound(v * v, sq_soft, total2 / N) + 4 * U.U24 * total2
        # population variance: the reference sums (x - mean)^2 in fp32; ours is sum x^2 / N - mean^2 in fp64
        c = v - v.mean()
        var = total2 / N - (total / N) ** 2
        c_soft = 2 * np.abs(c).max() * 2 * soft + 4 * soft * soft          # x and the mean both move by <= soft
        assert abs(s[f"{prefix}_std"] ** 2 - var) <= _mean_bound(c * c, c_soft, var) + 4 * U.U24 * var + 4 * U.U24 * np.abs(c).max() ** 2
    assert got["sums"][4] == wq.sum() and got["sums"][5] == (wq * wq).sum()                  # exact in fp64 in any order
    flat, lead = U.lead_over_runner_up(logits, D, n, step)
    ref_flat = e["row_index"] * D + e["col_index"]
    if lead > 4 * eps:                                       # unambiguous on any expf: the same tuple, its lowest index
        assert np.array_equal(logits.reshape(N, n)[ref_flat], logits.reshape(N, n)[got["flat"]])
        assert got["flat"] == flat and got["flat"] <= ref_flat
    assert abs(abs(diff.reshape(-1)[ref_flat]) - got["max_abs"]) <= eps
    assert e["w_quant_value"] == wq.reshape(-1)[ref_flat] and abs(e["w_float_value"] - wf.reshape(-1)[ref_flat]) <= eps
    assert abs(e["abs_diff"] - got["max_abs"]) <= eps


def test_report_has_the_reference_layout():
    z, meta = _golden("quantization")
    for case in meta["cases"]:
        keys = ("bit_index", "logit", "prob", "hard", "bit_weight", "float_contrib", "quant_contrib")
        bits = [{k: (int(v) if k in ("bit_index", "hard") else float(v)) for k, v in zip(keys, row)}
                for row in z[f"{case['name']}_bit_details"]]
        result = {**case["stats"], **case["entry"], "bit_details": tuple(bits)}
        assert format_quantization_report(result) == case["report"]
    assert case["report"].count("\n") == 19 + 8 and case["report"].startswith("=== Decoder Weight Quantization Report ===")


def test_moments_restatement_and_finish_reproduce_the_reference_baseline():
    z, meta = _golden("baseline")
    x, ref = z["x"], meta["result"]
    g = meta["batch_rows"]
    sums, kept, skipped = U.moments_restate(x, None, g)
    assert (kept, skipped) == (meta["rows"] - g, g) and g <= meta["nan_row"] < 2 * g
    m = DatasetMoments(meta["D"], g, device="cpu")             # the Python arithmetic of finish() on the restated state
    m.sums[:] = torch.from_numpy(sums)
    m.counts[:] = torch.tensor([kept, skipped])
    out = m.finish()
    assert out["total_samples"] == ref["total_samples"] == kept * meta["D"] and out["rows"] == kept and out["skipped_rows"] == skipped
    keep = np.concatenate([x[:g], x[2 * g:]]).astype(np.float64)
    n_el = keep.size
    # the reference adds one fp32 .sum() per batch: the fp32 bound over each batch's terms, and one rounding per square
    b1 = sum(U.fp32_sum_bound(b) for b in (keep[:g], keep[g:])) + U.fp64_sum_bound(keep)
    b2 = sum(U.fp32_sum_bound(b * b) + U.U24 * (b * b).sum() for b in (keep[:g], keep[g:])) + U.fp64_sum_bound(keep * keep)
    assert abs(out["mean"] - ref["mean"]) <= b1 / n_el
    assert abs(out["baseline_mse_zeros"] - ref["baseline_mse_zeros"]) <= b2 / n_el
    assert abs(out["variance"] - ref["variance"]) <= b2 / n_el + 2 * abs(ref["mean"]) * b1 / n_el + (b1 / n_el) ** 2
    assert out["baseline_mse_mean"] == out["variance"] and "mse" not in out
    assert abs(sums[0].sum() - keep.sum()) <= U.fp64_sum_bound(keep) and abs(sums[1].sum() - (keep * keep).sum()) <= U.fp64_sum_bound(keep * keep)
    assert np.allclose(out["variance_per_dim"].numpy(), keep.var(0), rtol=1e-12) and out["mean_per_dim"].shape == (meta["D"],)


# ---- the planted inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.QUANT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_planted_cases_hold_what_they_promise(case):
    H, D, n = case
    step = U.step_of(n)
    assert np.log2(step) == int(np.log2(step))
    logits = U.quant_logits(H, D, n)
    flat = logits.reshape(-1)
    for v in (30.0, -30.0, 100.0, -100.0):
        assert (flat == v).any()
    assert (np.signbit(flat) & (flat == 0)).any()
    for bits in (U.SIG_GT_BITS, U.SIG_GT_BITS - 1, U.SIG_GE_BITS, U.SIG_GE_BITS - 1):
        assert (flat.view(np.uint32) == bits).any()
    ref = U.quant_restate(logits, D, n, step, exact=True)
    assert (ref["und"] > 0).all() and ref["n_nan"] == 0 and U.quant_restate(U.quant_logits(H, D, n, "nan"), D, n, step)["n_nan"] == 1
    if n > 1:
        # at n = 1 the supremum 0.5 step is reached to within an ulp by all four cutoff plants: nothing can lead there
        for variant in ("plain", "tie"):
            at, lead = U.lead_over_runner_up(U.quant_logits(H, D, n, variant), D, n, step)
            assert at == 3 and lead > 4 * U.eps_of(n, step)
        tie = U.quant_logits(H, D, n, "tie").reshape(H * D, n)
        assert np.array_equal(tie[3], tie[H * D - 3])
