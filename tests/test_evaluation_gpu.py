"""The evaluation reports on the GPU: qsae_quantization_error and qsae_dataset_moments_add through ``ops`` and through the
public API (``quantization_error``, ``DatasetMoments``, ``estimate_baseline_error``, ``evaluate_dataset``) against the numpy
restatements of tests/evaluation_util.py -- the hard side, the counts, the index of the largest difference and the moments
for equality, the soft side (the device's expf) within the eps derived there -- and against the reference's own numbers
(tests/golden/evaluation_*.npz).

At n = 1 the index of the largest difference is checked through its value only: the supremum 0.5 step is reached to
within an ulp by each of the four planted cutoff logits, so no entry can lead the others by 4 eps there."""
import functools
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import evaluation_util as U
from quantizedsae_amd import BinarySAE, ops, synthetic as S
from quantizedsae_amd.inference import (DatasetMoments, estimate_baseline_error, evaluate_dataset, format_quantization_report,
                                        quantization_error)
from quantizedsae_amd.inference import analysis as A
from quantizedsae_amd.inference import framework as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
QUANT = [(c, v) for c in U.QUANT_CASES for v in ("plain", "tie", "nan")]
QUANT_IDS = ["x".join(map(str, c)) + "_" + v for c, v in QUANT]


@functools.lru_cache(maxsize=None)
def _quant(case, variant):
    H, D, n = case
    logits = U.quant_logits(H, D, n, variant)
    block, unit = ops.quantization_error(torch.from_numpy(logits).to(DEV), D, n, U.step_of(n), U.MARGIN)
    return logits, block.cpu().numpy(), unit.cpu().numpy()


def _model(case, variant):
    H, D, n = case
    model = BinarySAE(D, H, gamma=4.0, n_bits=n)
    with torch.no_grad():
        model.decoder.weight.copy_(torch.from_numpy(U.quant_logits(H, D, n, variant)))
    return model.to(DEV).eval()


# ---- quantization error ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant", QUANT, ids=QUANT_IDS)
def test_quantization_error_equals_the_restatement(case, variant):
    H, D, n = case
    logits, block, unit = _quant(case, variant)
    got = U.parse_block(block)
    U.check_quant(got, unit, logits, D, n, U.step_of(n))
    if variant != "nan" and n > 1:
        assert got["flat"] == 3                            # the planted maximum; of two identical tuples the lower index


def test_quantization_error_gives_the_same_bits_on_every_run():
    case = (300, 516, 4)
    logits, block, unit = _quant(case, "plain")
    again, unit2 = ops.quantization_error(torch.from_numpy(logits).to(DEV), 516, 4, U.step_of(4), U.MARGIN)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), block.view(np.uint64)) and np.array_equal(unit2.cpu().numpy(), unit)
    # a copy 4 bytes off the vector boundary takes the scalar loads: the same bits
    shifted = torch.empty(logits.size + 1, dtype=torch.float32, device=DEV)[1:]
    shifted.copy_(torch.from_numpy(logits).reshape(-1))
    assert shifted.data_ptr() % 16 == 4
    b3, u3 = ops.quantization_error(shifted.view(300, 516 * 4), 516, 4, U.step_of(4), U.MARGIN)
    assert np.array_equal(b3.cpu().numpy().view(np.uint64), block.view(np.uint64)) and np.array_equal(u3.cpu().numpy(), unit)


@pytest.mark.parametrize("case,variant", QUANT, ids=QUANT_IDS)
def test_public_quantization_error(case, variant):
    H, D, n = case
    step, N = U.step_of(n), H * D
    logits, block, unit = _quant(case, variant)
    got = U.parse_block(block)
    model = _model(case, variant)
    r = quantization_error(model)
    assert np.array_equal(r["unit_err_sq"].cpu().numpy(), unit, equal_nan=True)
    assert r["n_nan"] == got["n_nan"] and r["undecided_per_bit"] == got["und"][:n].tolist()
    assert (r["row_index"], r["col_index"]) == divmod(got["flat"], D)
    # soft_gap is the packer's number, bit for bit (step is a power of two); polarize_loss the training forward's
    _, _, gap = ops.pack_binary(model.decoder.weight.detach(), D, n, want_soft_gap=True)
    assert np.float32(r["soft_gap"]) == np.float32(gap.item()) and float(np.float32(r["soft_gap"])) == r["soft_gap"]
    assert np.array_equal([b["logit"] for b in r["bit_details"]], logits.reshape(N, n)[got["flat"]].astype(np.float64), equal_nan=True)
    text = format_quantization_report(r)
    assert text.count("\n") == 19 + n and f"({r['row_index']}, {r['col_index']})" in text
    if variant == "nan":
        assert r["soft_gap"] == math.inf and all(math.isnan(r[k]) for k in ("mse", "max_abs", "float_min", "float_max", "float_std"))
        assert r["quant_min"] == got["min_q"] and r["quant_mean"] == got["sums"][4] / N
        return
    eps = U.eps_of(n, step)
    ref = U.quant_restate(logits, D, n, step, exact=True)
    assert r["mse"] == got["sums"][0] / N and r["l2_norm"] == math.sqrt(got["sums"][0]) and r["max_abs"] == got["max_abs"]
    assert abs(r["mean_abs"] - ref["sums"][1] / N) <= eps and abs(r["float_mean"] - ref["sums"][2] / N) <= eps
    assert r["quant_mean"] == ref["sums"][4] / N and r["quant_l2_norm"] == math.sqrt(ref["sums"][5])
    assert r["quant_min"] == ref["min_q"] and r["quant_max"] == ref["max_q"]
    assert abs(r["float_min"] - ref["min_f"]) <= eps and abs(r["float_max"] - ref["max_f"]) <= eps
    # squared statistics of the float side: the sum of squares moves by <= N (2 max|w| eps + eps^2), the mean by <= eps
    max_f = max(abs(ref["min_f"]), abs(ref["max_f"]))
    sq_f = 2 * max_f * eps + eps * eps
    assert abs(r["float_l2_norm"] ** 2 - ref["sums"][3]) <= N * sq_f + 4 * U.U53 * ref["sums"][3]
    mean_f = ref["sums"][2] / N
    var_f = ref["sums"][3] / N - mean_f * mean_f
    assert abs(r["float_std"] ** 2 - var_f) <= sq_f + 2 * abs(mean_f) * eps + eps * eps + 8 * U.U53 * ref["sums"][3] / N
    assert abs(r["l2_norm"] ** 2 - ref["sums"][0]) <= N * (2 * ref["max_abs"] * eps + eps * eps) + 4 * U.U53 * ref["sums"][0]
    mean_q = ref["sums"][4] / N
    assert r["quant_std"] == math.sqrt(max(ref["sums"][5] / N - mean_q * mean_q, 0.0))
    assert r["w_quant_value"] == U.entries(logits, D, n, step, exact=True)[1].reshape(-1)[got["flat"]]
    assert abs(r["w_float_value"] - U.entries(logits, D, n, step, exact=True)[0].reshape(-1)[got["flat"]]) <= eps
    assert abs(abs(r["signed_diff"]) - r["abs_diff"]) <= eps and r["abs_diff"] == r["max_abs"]
    assert np.allclose(r["mean_abs_logit_per_bit"], np.abs(logits.reshape(N, n)).astype(np.float64).mean(0), rtol=1e-12)
    # p (1 - p) 2^b: per term <= 7 u 2^b (tests/evaluation_util.py), so the mean over [H, D, n] moves by <= 7 u (2^n - 1) / n
    # <= eps / (step n); the training forward rounds its fp64 mean to fp32 once
    _, pol = ops.binary_soft_table_polarize(model.decoder.weight.detach(), D, n)
    assert abs(r["polarize_loss"] - float(pol)) <= eps / (step * n) + U.U24 * abs(r["polarize_loss"])
    want_pol = sum(ref["pol"][b] * 2.0 ** b for b in range(n)) / (N * n)
    assert abs(r["polarize_loss"] - want_pol) <= eps / (step * n)


def test_quantization_error_reproduces_the_reference_numbers():
    z = np.load(ROOT / "tests" / "golden" / "evaluation_quantization.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    H, D = meta["H"], meta["D"]
    for case in meta["cases"]:
        n, step, s = case["n_bits"], case["step"], case["stats"]
        logits = z[f"{case['name']}_logits"]
        model = BinarySAE(D, H, gamma=meta["gamma"], n_bits=n)
        with torch.no_grad():
            model.decoder.weight.copy_(torch.from_numpy(logits))
        r = quantization_error(F.SAEWrapper(F.SAE_REGISTRY["b_sae"], model, DEV))
        eps, N = U.eps_of(n, step), H * D
        wf, wq, diff = U.entries(logits, D, n, step, exact=True)
        # the reference's fp32 sums: n 2^-24 sum |terms| and one rounding per term, plus eps on the soft side
        for key, terms, soft in (("mse", diff * diff, 2 * np.abs(diff).max() * eps + eps * eps), ("mean_abs", np.abs(diff), eps),
                                 ("float_mean", wf, eps), ("quant_mean", wq, 0.0)):
            bound = (U.fp32_sum_bound(terms) + U.U24 * np.abs(terms).sum()) / N + soft + 2 * U.U24 * abs(s[key])
            assert abs(r[key] - s[key]) <= bound, (case["name"], key)
        for key in ("max_abs", "float_min", "float_max"):
            assert abs(r[key] - s[key]) <= eps
        assert r["quant_min"] == s["quant_min"] and r["quant_max"] == s["quant_max"]
        flat, lead = U.lead_over_runner_up(logits, D, n, step)
        if lead > 4 * eps:
            assert r["row_index"] * D + r["col_index"] == flat <= case["entry"]["row_index"] * D + case["entry"]["col_index"]
        assert abs(r["abs_diff"] - case["entry"]["abs_diff"]) <= eps


# ---- dataset moments ---------------------------------------------------------------------------------------------------------
def _to_device(x):
    if x.dtype == np.uint16:
        return torch.from_numpy(x.view(np.int16)).to(DEV).view(torch.bfloat16)
    return torch.from_numpy(x).to(DEV)


def _moment_case(B, D, dtype, special=None):
    x = U.moment_rows(B, D, dtype)
    xf = U.moments_as_f32(x)
    recon = (xf * np.float32(0.75) + np.float32(0.125)).astype(np.float32)
    if special in ("nan", "nan_inf"):
        xf[1500, 7] = np.nan                               # group 1 of the 1024-row groups
    if special == "nan_inf":
        xf[10, 3] = np.inf                                 # group 0: summed, not skipped
    return (xf if special else x), xf, recon


MOMENTS = [(c, None) for c in U.MOMENT_CASES] + [((3000, 516, "float32"), "nan"), ((3000, 516, "float32"), "nan_inf")]


@pytest.mark.parametrize("with_recon", [False, True], ids=["x", "x_recon"])
@pytest.mark.parametrize("case,special", MOMENTS, ids=["x".join(map(str, c)) + ("_" + s if s else "") for c, s in MOMENTS])
def test_dataset_moments(case, special, with_recon):
    B, D, dtype = case
    x, xf, recon = _moment_case(B, D, dtype, special)
    recon = recon if with_recon else None
    xd, rd = _to_device(x), (torch.from_numpy(recon).to(DEV) if with_recon else None)
    want = U.moments_restate(xf, recon, 1024)

    def run(cuts):
        m = DatasetMoments(D, 1024, DEV)
        for a, b in zip(cuts[:-1], cuts[1:]):
            m.add(xd[a:b], rd[a:b] if with_recon else None)
        return m, m.sums.cpu().numpy(), m.counts.cpu().tolist()
    m, sums, counts = run([0, B])
    assert counts == [want[1], want[2]] and counts[0] + counts[1] == B
    if special:
        assert counts == [3000 - 1024, 1024]
    q = 3 if with_recon else 2
    assert np.array_equal(sums[:q], want[0][:q]) and not sums[q:].any()           # the restated order: the same bits
    keep = np.concatenate([xf[:1024], xf[2048:]]).astype(np.float64) if special else xf.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for row, terms in ((0, keep), (1, keep * keep)):
            exact = terms.sum(0)
            fin = np.isfinite(exact)
            assert np.all(np.abs(sums[row] - exact)[fin] <= U.fp64_sum_bound(terms, 0)[fin]) and np.array_equal(sums[row][~fin], exact[~fin])
        assert fin.all() == (special != "nan_inf") and (special != "nan_inf" or (sums[0][3] == np.inf and sums[1][3] == np.inf))
    _, again, counts2 = run([0, B])
    assert np.array_equal(again, sums) and counts2 == counts                      # run to run
    if B > 1024:
        _, split, counts3 = run(sorted({0, 1024, min(2048, B), B}))
        assert np.array_equal(split, sums) and counts3 == counts                  # cut at multiples of group_rows
    out = m.finish()
    assert out["rows"] == counts[0] and out["skipped_rows"] == counts[1] and out["total_samples"] == counts[0] * D
    total = counts[0] * D
    s1, s2 = float(np.cumsum(sums[0])[-1]), float(np.cumsum(sums[1])[-1])
    if special != "nan_inf":
        assert out["mean"] == s1 / total and out["baseline_mse_zeros"] == s2 / total
        assert out["variance"] == out["baseline_mse_mean"] == s2 / total - (s1 / total) ** 2
    assert ("mse" in out) == with_recon
    if with_recon and special != "nan_inf":
        assert out["mse"] == float(np.cumsum(sums[2])[-1]) / total and out["fvu"] == out["mse"] / out["variance"]
        assert torch.equal(out["fvu_per_dim"], out["mse_per_dim"] / out["variance_per_dim"])


def test_moments_of_nothing_but_nan_raise_and_states_merge():
    m = DatasetMoments(4, 2, DEV)
    m.add(torch.full((5, 4), float("nan"), device=DEV))
    assert m.counts.cpu().tolist() == [0, 5]
    with pytest.raises(ValueError, match="no row was kept"):
        m.finish()
    x = torch.from_numpy(U.moment_rows(1025, 20, "float32")).to(DEV)
    whole, a, b = DatasetMoments(20, 1024, DEV), DatasetMoments(20, 1024, DEV), DatasetMoments(20, 1024, DEV)
    whole.add(x)
    a.add(x[:1024])
    b.add(x[1024:])
    a.merge(b)
    assert torch.equal(a.sums, whole.sums) and torch.equal(a.counts, whole.counts)
    with pytest.raises(ValueError, match="recon"):
        whole.add(x, x)


def test_estimate_baseline_error_reproduces_the_reference_numbers():
    z = np.load(ROOT / "tests" / "golden" / "evaluation_baseline.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    x, ref, g = z["x"], meta["result"], meta["batch_rows"]
    out = estimate_baseline_error([torch.from_numpy(x[a:a + g]) for a in range(0, x.shape[0], g)], group_rows=g, device=DEV)
    assert out["total_samples"] == ref["total_samples"] and out["skipped_rows"] == g
    keep = np.concatenate([x[:g], x[2 * g:]]).astype(np.float64)
    n_el = keep.size
    b1 = sum(U.fp32_sum_bound(b) for b in (keep[:g], keep[g:])) + U.fp64_sum_bound(keep)
    b2 = sum(U.fp32_sum_bound(b * b) + U.U24 * (b * b).sum() for b in (keep[:g], keep[g:])) + U.fp64_sum_bound(keep * keep)
    assert abs(out["mean"] - ref["mean"]) <= b1 / n_el and abs(out["baseline_mse_zeros"] - ref["baseline_mse_zeros"]) <= b2 / n_el
    assert abs(out["variance"] - ref["variance"]) <= b2 / n_el + 2 * abs(ref["mean"]) * b1 / n_el + (b1 / n_el) ** 2


def test_evaluate_dataset_agrees_with_the_reconstruction_error():
    D, H, n = 64, 1024, 4
    model = BinarySAE(D, H, gamma=4.0, n_bits=n)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in S.binary_sae_params(5, D, H, n).items()})
    sae = F.SAEWrapper(F.SAE_REGISTRY["b_sae"], model, DEV)
    x = S.activations(6, 600, D)
    loader = [torch.from_numpy(x[a:a + 200]) for a in range(0, 600, 200)]
    out = evaluate_dataset(sae, loader)
    mse = float(A.compute_reconstruction_error_by_level(sae, loader)[0])
    # both add the same fp32 squares in fp64, in two different orders
    recon = torch.cat([sae.reconstruct(b) for b in loader]).cpu().numpy()
    e = (recon - x).astype(np.float32)
    terms = (e * e).astype(np.float64)
    assert abs(out["mse"] - mse) <= 2 * U.fp64_sum_bound(terms) / terms.size and out["mse"] > 0
    assert out["fvu"] == out["mse"] / out["variance"] and out["rows"] == 600 and out["skipped_rows"] == 0
    assert abs(out["variance"] - x.astype(np.float64).var()) <= 1e-12 * x.astype(np.float64).var()
