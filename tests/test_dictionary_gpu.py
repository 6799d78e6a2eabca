"""Decoder-dictionary comparison on the GPU (csrc/dictionary.hip): parity with the reference's fixtures, edge shapes,
self-consistency of the stats-only pass with the stored matrix, symmetry, determinism, and full size against fp64."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import quantizedsae_amd as Q
from quantizedsae_amd import synthetic as S
from quantizedsae_amd.inference import compare_decoders, decoder_atoms, decoder_cosine_similarity

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import dictionary_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDENS = sorted(p.stem for p in (ROOT / "tests" / "golden").glob("dictionary_*.npz"))


def _model(spec, D, H):
    return U.build(Q, spec, D, H).to(DEV)


def _f64_cos(a, b):
    a, b = a.double(), b.double()
    return torch.nn.functional.normalize(a, dim=1, eps=1e-12) @ torch.nn.functional.normalize(b, dim=1, eps=1e-12).t()


def _best_from_matrix(m, dim):
    """(value, lowest index of the max) along dim, as the kernel's keys define them."""
    mx = m.max(dim).values
    hit = m == (mx.unsqueeze(dim))
    return mx + 0.0, hit.int().argmax(dim)


def _check_against_f64(out, a, b, self_mode=False):
    ref = _f64_cos(a, b)
    if self_mode:
        ref.fill_diagonal_(-float("inf"))
    rmax, cmax = ref.max(1).values, ref.max(0).values
    finite = torch.isfinite(rmax)
    assert torch.all((out["a_to_b_max"].double() - rmax)[finite].abs() <= 1e-5)
    picked = ref.gather(1, out["a_to_b_argmax"].clamp(min=0).unsqueeze(1)).squeeze(1)
    assert torch.all((rmax - picked)[finite] <= 2e-5)
    if not self_mode:
        assert torch.all((out["b_to_a_max"].double() - cmax).abs() <= 1e-5)
        picked = ref.gather(0, out["b_to_a_argmax"].unsqueeze(0)).squeeze(0)
        assert torch.all(cmax - picked <= 2e-5)
    vals = ref[torch.triu(torch.ones_like(ref, dtype=torch.bool), 1)] if self_mode else ref.flatten()
    if vals.numel():
        assert abs(out["mean"] - vals.mean().item()) <= 1e-6
        assert abs(out["max"] - vals.max().item()) <= 1e-5 and abs(out["min"] - vals.min().item()) <= 1e-5


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_parity(name):
    z = np.load(ROOT / "tests" / "golden" / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    D, H = meta["D"], meta["H"]
    lhs, rhs = _model(meta["lhs"], D, H), _model(meta["rhs"], D, H)
    a, b = decoder_atoms(lhs), decoder_atoms(rhs)
    assert a.device == torch.device(DEV) and a.dtype == torch.float32
    assert torch.equal(a.cpu(), torch.from_numpy(U.atoms_np(meta["lhs"], D, H)))
    out = compare_decoders(lhs, rhs, top=100)
    m64 = _f64_cos(a, b).cpu().numpy()
    for key, want, idx_key, axis in (("a_to_b_max", z["row_max"], "a_to_b_argmax", 1),
                                     ("b_to_a_max", z["col_max"], "b_to_a_argmax", 0)):
        got = out[key].cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
        gi = out[idx_key].cpu().numpy()
        ri = z["row_argmax"] if axis == 1 else z["col_argmax"]
        diff = gi != ri
        if axis == 1:
            vg, vr = m64[np.arange(len(gi)), gi], m64[np.arange(len(ri)), ri]
        else:
            vg, vr = m64[gi, np.arange(len(gi))], m64[ri, np.arange(len(ri))]
        assert np.all(np.abs(vg - vr)[diff] <= 2e-5), f"{key}: {diff.sum()} argmax differ by more than 2e-5"
    assert abs(out["mean"] - float(z["mean"])) <= 1e-5
    assert abs(out["mean_top_k"] - float(z["mean_top"])) <= 1e-5
    rows = decoder_cosine_similarity(lhs, rhs)[torch.from_numpy(z["rows"]).to(DEV)].cpu().numpy()
    np.testing.assert_allclose(rows, z["matrix_rows"], rtol=0, atol=1e-5)


def _rand_atoms(seed, H, D):
    return torch.from_numpy(S.normal(seed, (H, D), stream=7)).to(DEV)


@pytest.mark.parametrize("D", [48, 100, 512])
@pytest.mark.parametrize("Ha,Hb", [(1, 777), (777, 1000), (1000, 1), (1, 1)])
def test_edge_shapes(Ha, Hb, D):
    a, b = _rand_atoms(Ha + D, Ha, D), _rand_atoms(Hb + 3 * D, Hb, D)
    out = compare_decoders(a, b, thresholds=(0.1, 0.2), bins=64)
    _check_against_f64(out, a, b)
    assert out["histogram"].sum().item() == Ha * Hb
    if Ha > 1:
        _check_against_f64(compare_decoders(a), a, a, self_mode=True)


def test_zero_atom_square_and_errors():
    a = _rand_atoms(5, 300, 64)
    a[17] = 0
    out = compare_decoders(a, _rand_atoms(6, 200, 64), return_matrix=True)
    assert torch.all(out["matrix"][17] == 0) and out["a_to_b_max"][17].item() == 0 and out["a_to_b_argmax"][17].item() == 0
    self_out = compare_decoders(a)
    _check_against_f64(self_out, a, a, self_mode=True)
    # square dictionaries keep the reference's orientation: not transposed
    base = _model({"variant": "baseline", "seed": 9}, 64, 64)
    assert torch.equal(decoder_atoms(base), base.decoder.weight.detach())
    one = compare_decoders(a[:1])
    assert one["a_to_b_max"].item() == -float("inf") and one["a_to_b_argmax"].item() == -1 and one["n_pairs"] == 0
    with pytest.raises(ValueError):
        compare_decoders(a, _rand_atoms(6, 20, 60))
    with pytest.raises(ValueError):
        compare_decoders(a, a.cpu())


def _derived(m, thresholds, bins, self_mode):
    n = m.shape[0]
    mask = torch.triu(torch.ones_like(m, dtype=torch.bool), 1) if self_mode else torch.ones_like(m, dtype=torch.bool)
    vals = m[mask]
    mm = m.masked_fill(~mask, -float("inf"))
    if self_mode:
        mm = torch.maximum(mm, mm.t())              # row i: partners j > i (c(i, j)) and j < i (c(j, i))
    rmax, rarg = _best_from_matrix(mm, 1)
    cmax, carg = _best_from_matrix(mm, 0)
    b = ((vals + 1.0) * (bins * 0.5)).floor().clamp(0, bins - 1).long()
    return dict(rmax=rmax, rarg=rarg, cmax=cmax, carg=carg, vals=vals,
                counts=[int((vals > t).sum()) for t in thresholds], hist=torch.bincount(b, minlength=bins))


@pytest.mark.parametrize("self_mode", [False, True])
def test_stats_match_same_call_matrix(self_mode):
    a = _rand_atoms(11, 1000, 100)
    b = None if self_mode else _rand_atoms(12, 777, 100)
    thr = (-0.1, 0.0, 0.05, 0.2)
    out = compare_decoders(a, b, thresholds=thr, bins=4096, return_matrix=True)
    d = _derived(out["matrix"], thr, 4096, self_mode)
    assert torch.equal(out["a_to_b_max"], d["rmax"]) and torch.equal(out["a_to_b_argmax"], d["rarg"])
    if not self_mode:
        assert torch.equal(out["b_to_a_max"], d["cmax"]) and torch.equal(out["b_to_a_argmax"], d["carg"])
    assert out["max"] == d["vals"].max().item() + 0.0 and out["min"] == d["vals"].min().item() + 0.0
    assert [out["count_above"][t] for t in thr] == d["counts"]
    assert torch.equal(out["histogram"], d["hist"])
    v = d["vals"].double()
    assert abs(out["mean"] - v.mean().item()) <= 1e-12 * abs(v.mean().item()) + 1e-15
    var = (v * v).mean().item() - v.mean().item() ** 2
    assert abs(out["std"] ** 2 - var) <= 1e-12 * var


def test_symmetry_and_self_mode_row_bests():
    a = _rand_atoms(13, 1000, 512)
    cross = compare_decoders(a, a, return_matrix=True)
    m = cross["matrix"]
    assert torch.equal(m.view(torch.int32), m.t().contiguous().view(torch.int32))
    masked = m.clone()
    masked.fill_diagonal_(-float("inf"))
    rmax, rarg = _best_from_matrix(masked, 1)
    self_out = compare_decoders(a)
    assert torch.equal(self_out["a_to_b_max"], rmax) and torch.equal(self_out["a_to_b_argmax"], rarg)


def test_determinism():
    a, b = _rand_atoms(14, 1000, 100), _rand_atoms(15, 900, 100)
    for rhs in (b, None):
        r1 = torch.ops.qsae.cosine_compare(a, rhs, [0.1], 128, False)
        r2 = torch.ops.qsae.cosine_compare(a, rhs, [0.1], 128, False)
        for x, y in zip(r1, r2):
            assert torch.equal(x, y)


def _full_check(lhs, rhs):
    a, b = decoder_atoms(lhs), decoder_atoms(rhs)
    assert a.shape == (32768, 512) and b.shape == (32768, 512)
    thr = (0.3, 0.5)
    out = compare_decoders(lhs, rhs, thresholds=thr)
    an = torch.nn.functional.normalize(a.double(), dim=1, eps=1e-12)
    bn = torch.nn.functional.normalize(b.double(), dim=1, eps=1e-12)
    cmax = torch.full((b.shape[0],), -2.0, dtype=torch.float64, device=DEV)
    near = {t: 0 for t in thr}
    exact = {t: 0 for t in thr}
    for i0 in range(0, a.shape[0], 4096):
        blk = an[i0:i0 + 4096] @ bn.t()
        rmax = blk.max(1).values
        sl = slice(i0, i0 + 4096)
        assert torch.all((out["a_to_b_max"][sl].double() - rmax).abs() <= 1e-5)
        picked = blk.gather(1, out["a_to_b_argmax"][sl].unsqueeze(1)).squeeze(1)
        assert torch.all(rmax - picked <= 2e-5)
        cmax = torch.maximum(cmax, blk.max(0).values)
        for t in thr:
            exact[t] += int((blk > t).sum())
            near[t] += int(((blk - t).abs() <= 1e-5).sum())
        del blk
    assert torch.all((out["b_to_a_max"].double() - cmax).abs() <= 1e-5)
    picked = torch.stack([(an[out["b_to_a_argmax"][j0:j0 + 4096]] * bn[j0:j0 + 4096]).sum(1)
                          for j0 in range(0, b.shape[0], 4096)]).flatten()
    assert torch.all(cmax - picked <= 2e-5)
    for t in thr:
        assert abs(out["count_above"][t] - exact[t]) <= near[t]
    rows = torch.arange(0, a.shape[0], a.shape[0] // 64, device=DEV)[:64]
    got = decoder_cosine_similarity(lhs, rhs)[rows].double()
    assert torch.all((got - an[rows] @ bn.t()).abs() <= 1e-5)


@pytest.fixture(scope="module")
def full_baseline():
    return _model({"variant": "baseline", "seed": 71}, 512, 32768)


def test_full_size_binary_vs_baseline(full_baseline):
    _full_check(_model({"variant": "binary", "seed": 72}, 512, 32768), full_baseline)


def test_full_size_residual_vs_baseline(full_baseline):
    rq = _model({"variant": "residual", "seed": 73}, 512, 32768)
    assert len(rq.saes) == 4 and sum(s.decoder.weight.shape[0] for s in rq.saes) == 32768
    _full_check(rq, full_baseline)
