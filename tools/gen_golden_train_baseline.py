#!/usr/bin/env python3
"""Generate tests/golden/train_baseline_*.npz by running the REFERENCE BaselineSparseAutoencoder forward and loss.backward()
(container-only).

Weights and inputs come from the portable PRNG recipes of tests/train_baseline_util.py (quantizedsae_amd/synthetic.py),
loaded into the reference class (tools/ref_loader.py) with its topk set to the recipe's k.  The loss is the baseline_sae
branch of training/trainer.py:166-173, mse(recon, x), plus mu * |h_sparse|.sum() / B where a recipe asks for it (with x
requiring grad).  A seed whose smallest relative gap between the k-th and (k+1)-th latent of a row is under 1e-4 is
advanced by 1000, so that the reference's sgemm order cannot decide the selection.  Only data is written: the recipe and
seed, the reference's selection and values, the gap, the loss, every gradient, and for the first recipe decoder.weight after
the reference's normalize_decoder_weights().

Run:  python tools/gen_golden_train_baseline.py        (needs the reference checkout; CPU only, seconds)
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import train_baseline_util as U  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
MIN_GAP = 1e-4
MAX_BYTES = 600 * 1024


def selection_gap(latent: torch.Tensor, k: int) -> float:
    top = latent.topk(k + 1, dim=1).values
    gap = (top[:, k - 1] - top[:, k]) / top[:, k - 1].abs().clamp_min(1e-30)
    return float(gap.min())


def run_case(ref, name: str, case: dict, seed: int):
    sd, x_np = U.case_inputs(case, seed)
    model = ref.BaselineSparseAutoencoder(case["D"], case["H"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.topk = case["k"]
    x = torch.from_numpy(x_np).requires_grad_(case["x_grad"])
    with torch.no_grad():
        latent_full = model.encoder(x)
    gap = selection_gap(latent_full, case["k"])
    sparse, recon = model(x)
    loss = F.mse_loss(recon, x)
    if case["mu"]:
        loss = loss + case["mu"] * sparse.abs().sum() / x.shape[0]
    loss.backward()
    vals, ids = latent_full.topk(case["k"], dim=1)
    arrays = {"idx": ids.numpy().astype(np.int32), "val": vals.numpy().astype(np.float32), "gap": np.float64(gap),
              "loss": np.float64(loss.item())}
    for pname, p in model.named_parameters():
        arrays["grad." + pname] = p.grad.numpy().astype(np.float32)
    if case["x_grad"]:
        arrays["grad.x"] = x.grad.numpy().astype(np.float32)
    if name == U.NORMALIZED_CASE:
        model.normalize_decoder_weights()
        arrays["normalized.decoder.weight"] = model.decoder.weight.detach().numpy().astype(np.float32)
    return gap, arrays


def main():
    ref = load_reference()
    torch.manual_seed(0)
    OUT.mkdir(parents=True, exist_ok=True)
    for name, case in U.CASES.items():
        seed = case["seed"]
        while True:
            gap, arrays = run_case(ref, name, case, seed)
            if gap >= MIN_GAP:
                break
            seed += 1000
        meta = dict(case, seed=seed, min_gap=MIN_GAP)
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
        size = path.stat().st_size
        assert size <= MAX_BYTES, f"{path.name} is {size} bytes"
        print(f"  wrote {path.name}: {size / 1024:.1f} KiB  seed {seed}  gap {gap:.3g}  loss {arrays['loss']:.6g}")


if __name__ == "__main__":
    main()
