#!/usr/bin/env python3
"""Generate tests/golden/train_blatent_*.npz by running the REFERENCE BinaryLatentSAE forward and loss.backward()
(container-only, CPU).

Weights and inputs come from the portable PRNG recipes of tests/train_blatent_util.py (quantizedsae_amd/synthetic.py), loaded
into the reference class (tools/ref_loader.py).  Every recipe must make the reference itself unambiguous, which is checked
here and recorded in the fixture's meta: no encoder pre-activation of the batch may lie within NEAR_TIE_EPS
(tests/golden_util.py, 4e-6) of the binarisation cutoff -- a seed that has one is advanced by 1000 -- so no element has to be
left out of any comparison.  Only data is written: the recipe and the seed it settled on, x, the reference's binary latent
(packed bits), reconstruction, loss = F.mse_loss(recon, x), every parameter gradient and x.grad (the mse target is detached,
so x.grad is the encoder path alone).

train_blatent_loop.npz holds the losses of LOOP["steps"] steps of forward, F.mse_loss, backward, torch.optim.Adam on a fixed
batch, run once in fp32 and once with the reference model in fp64, the largest relative gap between the two runs and the
bound the GPU loop is held to (ten times that gap, at least 1e-5).  The two runs must set the same latent bits at every step
(asserted; a seed where they do not is advanced by 1000), and beyond that no fp64 pre-activation of any step may lie within
LOOP_MARGIN of the band between the fp32 cutoff (-1.79e-7) and the fp64 one (0): a third fp32 summation order -- the GPU's --
then sets the same bits as well.

Run:  python tools/gen_golden_train_blatent.py        (needs the reference checkout; CPU only, a minute)
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

import train_blatent_util as U  # noqa: E402
from golden_util import NEAR_TIE_EPS  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
MAX_BYTES = 600 * 1024
MAX_LOOP_GAP = 1e-2
LOOP_MARGIN = 1.5e-7                # beyond either end of [CUTOFF, 0]: an fp32 chain of 64 terms of O(0.1) is off by ~3e-8
MAX_TRIES = 400


def build(ref, D: int, H: int, sd: dict, dtype=torch.float32):
    model = ref.BinaryLatentSAE(D, H)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(dtype)


def save(name: str, meta: dict, arrays: dict):
    path = OUT / f"{name}.npz"
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    size = path.stat().st_size
    assert size <= MAX_BYTES, f"{path.name} is {size} bytes"
    return size


def run_case(ref, case: dict, seed: int):
    sd, x_np = U.case_inputs(case, seed)
    model = build(ref, case["D"], case["H"], sd)
    x = torch.from_numpy(x_np).requires_grad_(True)
    with torch.no_grad():
        pre = model.encoder[0](x)
        gap = float((pre - U.CUTOFF).abs().min())
    z, recon = model(x)
    assert not z.requires_grad and recon.grad_fn is not None
    assert torch.equal(z, (pre >= U.CUTOFF).float()), "the fp32 cutoff does not restate sigmoid(pre) >= 0.5"
    loss = F.mse_loss(recon, x.detach())
    loss.backward()
    arrays = {"x": x_np, "loss": np.float64(loss.item()), "min_cutoff_distance": np.float64(gap),
              "binary_latent": U.pack_latent(z.numpy()), "recon": recon.detach().numpy(), "grad.x": x.grad.numpy()}
    for pname, p in model.named_parameters():
        arrays["grad." + pname] = p.grad.numpy().astype(np.float32)
    return gap, float(z.mean()), arrays


def run_loop(ref, seed: int, dtype):
    """-> (losses, bits per step, smallest distance of a pre-activation to the band [CUTOFF, 0] over all steps)."""
    L = U.LOOP
    model = build(ref, L["D"], L["H"], U.blatent_params(seed, L["D"], L["H"]), dtype)
    x = torch.from_numpy(U.S.activations(seed, L["B"], L["D"])).to(dtype)
    opt = torch.optim.Adam(model.parameters(), lr=L["lr"])
    losses, bits, margin = [], [], float("inf")
    for _ in range(L["steps"]):
        with torch.no_grad():
            pre = model.encoder[0](x).double()
            margin = min(margin, float(torch.maximum(pre, U.CUTOFF - pre).min()))      # <= 0 inside the band
        z, recon = model(x)
        loss = F.mse_loss(recon, x)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
        bits.append(U.pack_latent(z.numpy()))
    return np.array(losses, np.float64), bits, margin


def main():
    ref = load_reference()
    torch.manual_seed(0)
    OUT.mkdir(parents=True, exist_ok=True)
    for name, case in U.CASES.items():
        seed = case["seed"]
        for _ in range(MAX_TRIES):
            gap, frac, arrays = run_case(ref, case, seed)
            if gap >= NEAR_TIE_EPS:
                break
            seed += 1000
        assert gap >= NEAR_TIE_EPS, f"{name}: no seed keeps every pre-activation {NEAR_TIE_EPS} from the cutoff"
        meta = dict(case, seed=seed, min_cutoff_distance=gap, near_tie_eps=NEAR_TIE_EPS, excluded=0, active_fraction=frac)
        size = save(name, meta, arrays)
        print(f"  wrote {name}.npz: {size / 1024:.1f} KiB  seed {seed}  min |pre - cutoff| {gap:.3g}  active {frac:.3f}  "
              f"loss {arrays['loss']:.6g}")
    seed = U.LOOP["seed"]
    for _ in range(MAX_TRIES):
        l32, b32, m32 = run_loop(ref, seed, torch.float32)
        l64, b64, m64 = run_loop(ref, seed, torch.float64)
        same = all(np.array_equal(a, b) for a, b in zip(b32, b64))
        if same and min(m32, m64) >= LOOP_MARGIN:
            break
        seed += 1000
    assert same and min(m32, m64) >= LOOP_MARGIN, "no loop seed found"
    gap = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
    assert gap <= MAX_LOOP_GAP, f"loop recipe unfit: fp32-to-fp64 gap {gap}"
    assert l32[-1] < l32[0]
    bound = max(10.0 * gap, 1e-5)
    meta = dict(U.LOOP, seed=seed, gap=gap, bound=bound, same_bits_fp32_fp64=True, band_margin=min(m32, m64))
    size = save(U.LOOP_FIXTURE, meta, {"loss32": l32, "loss64": l64, "binary_latent_final": b64[-1]})
    print(f"  wrote {U.LOOP_FIXTURE}.npz: {size / 1024:.1f} KiB  seed {seed}  loss {l32[0]:.5f} -> {l32[-1]:.5f}  gap {gap:.3g}  "
          f"bound {bound:.3g}  band margin {min(m32, m64):.3g}")


if __name__ == "__main__":
    main()
