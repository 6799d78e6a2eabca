#!/usr/bin/env python3
"""Generate tests/golden/sparsity_curve_binary.npz and sparsity_curve_baseline.npz by running the REFERENCE's own forward at
several test-time k (container-only).

The reference classes are loaded as tools/ref_loader.py does; the parameters come from quantizedsae_amd.synthetic by seed
(D = 64, H = 1024, 32 rows; BinarySAE with polarised logits and n_bits = 4), so only arrays are written: per listed k' the
reference's reconstruction [32, 64] and its fp64 MSE, and the smallest gap between the latent values of rank k' and k' + 1
over all rows and listed k'.  BinarySAE takes k' through ``model.k = (k' + 0.5) / H``, the baseline through ``model.topk``.

The gap is asserted to be at least golden_util.NEAR_TIE_EPS: the reference's sgemm moves a latent by less than that against
the fmaf chain, so every row selects the same units on both sides and no row needs excluding.  The seeds below were chosen so
that this holds.

Run:  python tools/gen_golden_sparsity_curve.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

from golden_util import NEAR_TIE_EPS  # noqa: E402
from quantizedsae_amd import synthetic as S  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
D, H, ROWS, N_BITS = 64, 1024, 32, 4
KS = [1, 8, 33, 64]
SEEDS = {"binary": 400, "baseline": 400}


def build(ref, variant: str, seed: int):
    if variant == "binary":
        sd = S.binary_sae_params(seed, D, H, N_BITS, dec_bias_std=0.1)
        model = ref.BinarySAE(D, H, gamma=4.0, n_bits=N_BITS)
    else:
        sd = S.baseline_sae_params(seed, D, H, bias_std=0.1)
        model = ref.BaselineSparseAutoencoder(D, H)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.eval()


def min_gap(model, x: torch.Tensor) -> float:
    """the smallest gap between the values of rank k' and k' + 1 over all rows and listed k'"""
    with torch.no_grad():
        latent = model.encoder(x)
    v = torch.sort(latent, dim=1, descending=True).values.double()
    return float(min((v[:, k - 1] - v[:, k]).min() for k in KS))


def generate(ref, variant: str) -> None:
    seed = SEEDS[variant]
    model = build(ref, variant, seed)
    x = torch.from_numpy(S.activations(seed, ROWS, D))
    gap = min_gap(model, x)
    assert gap >= NEAR_TIE_EPS, f"{variant}: a listed k' sits on a near-tie (gap {gap:.3g}); choose another seed"
    recons, mse = [], []
    with torch.no_grad():
        for k in KS:
            if variant == "binary":
                model.k = (k + 0.5) / H
                assert int(model.hidden_dim * model.k) == k
            else:
                model.topk = k
            recon = model(x)[1]
            recons.append(recon.numpy().copy())
            mse.append(float(((recon.double() - x.double()) ** 2).mean()))
    path = OUT / f"sparsity_curve_{variant}.npz"
    np.savez_compressed(path, ks=np.array(KS, np.int32), recons=np.stack(recons).astype(np.float32), mse=np.array(mse, np.float64),
                        min_gap=np.float64(gap), seed=np.int64(seed), D=np.int64(D), H=np.int64(H), rows=np.int64(ROWS),
                        n_bits=np.int64(N_BITS))
    print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB  mse {mse}  min gap {gap:.3g}")


if __name__ == "__main__":
    ref = load_reference()
    if "--search" in sys.argv:                               # the first seeds from 400 on that clear the near-tie audit
        for variant in SEEDS:
            for seed in range(400, 500):
                if min_gap(build(ref, variant, seed), torch.from_numpy(S.activations(seed, ROWS, D))) >= NEAR_TIE_EPS:
                    print(variant, seed)
                    break
    else:
        for variant in SEEDS:
            generate(ref, variant)
