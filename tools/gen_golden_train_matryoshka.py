#!/usr/bin/env python3
"""Generate tests/golden/train_matryoshka_*.npz by running the REFERENCE QuantizedMatryoshkaSAE / ResidualQuantizedSAE
forward, loss.backward() and apply_secant_grad() (container-only, CPU).

Weights and inputs come from the portable PRNG recipes of tests/train_matryoshka_util.py (quantizedsae_amd/synthetic.py),
loaded into the reference classes (tools/ref_loader.py).  The loss is the q_sae / rq_sae branch of training/trainer.py:88-142.
A seed whose smallest |encoder pre-activation| over the whole batch is under 1e-4 is advanced by 1000, so that no summation
order decides a z bit.  Only data is written: the recipe and seed, the reference's z bits, outputs, loss, and every gradient
before and after apply_secant_grad().  train_matryoshka_loop.npz holds the losses of 30 trainer steps on a fixed batch per
recipe, run once in fp32 and once with the reference model in fp64, the largest relative gap between the two runs, and the
bound the GPU loop is held to (ten times that gap, at least 1e-5).

Run:  python tools/gen_golden_train_matryoshka.py        (needs the reference checkout; CPU only, seconds)
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

import train_matryoshka_util as U  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
MIN_ABS_PRE = 1e-4
MAX_BYTES = 600 * 1024


def build(ref, case: dict, sd: dict, dtype=torch.float32):
    if case["kind"] == "rq":
        model = ref.ResidualQuantizedSAE(case["D"], case["H"], 32, abs_range=U.ABS_RANGE, n_bits=case["n_bits"])
    else:
        model = ref.QuantizedMatryoshkaSAE(case["D"], case["H"], 32, abs_range=U.ABS_RANGE, n_bits=case["n_bits"],
                                           allow_bias=case.get("allow_bias", True))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(dtype)


def trainer_loss(case: dict, model, x):
    """(loss, stage inputs) of the q_sae / rq_sae branch."""
    groups, recons = model(x)
    lam = case["lam"]
    if case["kind"] == "rq":
        residual, rec, sp = x, [], 0
        for i, r in enumerate(recons):
            rec.append(0.5 * F.mse_loss(r, residual))
            residual = (residual - r).detach() * 2
            sp = sp + groups[i] * lam * U.RQ_STAGE_WEIGHTS[i]
        return sum(rec) + sp, groups, recons
    return sum(0.5 * F.mse_loss(r, x) for r in recons) + sum(groups) * lam, groups, recons


def stage_pre(case: dict, model, x):
    """[(z bool [B, H_i], min |pre|)] per stage (one stage for the plain model)."""
    out = []
    with torch.no_grad():
        if case["kind"] == "rq":
            residual = x
            for sae in model.saes:
                pre = sae.encoder[0](residual)
                out.append((pre > 0, float(pre.abs().min())))
                _, recs = sae(residual)
                residual = (residual - recs[-1]) * 2
        else:
            pre = model.encoder[0](x)
            out.append((pre > 0, float(pre.abs().min())))
    return out


def run_case(ref, case: dict, seed: int):
    sd, x_np = U.case_inputs(case, seed)
    model = build(ref, case, sd)
    x = torch.from_numpy(x_np)
    stages = stage_pre(case, model, x)
    gap = min(s[1] for s in stages)
    loss, groups, recons = trainer_loss(case, model, x)
    loss.backward()
    arrays = {"loss": np.float64(loss.item()), "min_abs_pre": np.float64(gap),
              "groups": np.array([float(g.detach()) for g in groups], np.float32),
              "levels": torch.stack([r.detach() for r in recons]).numpy().astype(np.float32)}
    for i, (z, _) in enumerate(stages):
        arrays[f"z.{i}"] = np.packbits(z.numpy().astype(np.uint8), axis=1, bitorder="little")
    for pname, p in model.named_parameters():
        arrays["grad." + pname] = (p.grad.numpy().astype(np.float32) if p.grad is not None
                                   else np.zeros((0,), np.float32))          # empty = None (bias without allow_bias)
    (model.apply_secant_grad if case["kind"] == "rq" else model.decoder.apply_secant_grad)()
    for pname, p in model.named_parameters():
        if pname.endswith("decoder.weight") or pname.endswith("decoder.weight_mirror"):
            arrays["secant." + pname] = p.grad.numpy().astype(np.float32)
    return gap, arrays


def run_loop(ref, name: str, lc: dict, dtype):
    case = dict(U.LOOP, **lc)
    sd, x_np = U.case_inputs(case, case["seed"])
    model = build(ref, case, sd, dtype)
    x = torch.from_numpy(x_np).to(dtype)
    opt = torch.optim.Adam(model.parameters(), lr=lc["lr"])
    losses = []
    for _ in range(case["steps"]):
        loss, _, _ = trainer_loss(case, model, x)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        (model.apply_secant_grad if case["kind"] == "rq" else model.decoder.apply_secant_grad)()
        opt.step()
        losses.append(float(loss.item()))
    return np.array(losses, np.float64)


def main():
    ref = load_reference()
    torch.manual_seed(0)
    OUT.mkdir(parents=True, exist_ok=True)
    for name, case in U.CASES.items():
        seed = case["seed"]
        while True:
            gap, arrays = run_case(ref, case, seed)
            if gap >= MIN_ABS_PRE:
                break
            seed += 1000
        meta = dict(case, seed=seed, min_abs_pre=MIN_ABS_PRE, abs_range=U.ABS_RANGE)
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
        size = path.stat().st_size
        assert size <= MAX_BYTES, f"{path.name} is {size} bytes"
        print(f"  wrote {path.name}: {size / 1024:.1f} KiB  seed {seed}  min|pre| {gap:.3g}  loss {arrays['loss']:.6g}")
    arrays, meta = {}, dict(U.LOOP, abs_range=U.ABS_RANGE, cases={})
    for name, lc in U.LOOP_CASES.items():
        l32, l64 = run_loop(ref, name, lc, torch.float32), run_loop(ref, name, lc, torch.float64)
        gap = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
        bound = max(10.0 * gap, 1e-5)
        arrays[f"{name}.loss32"], arrays[f"{name}.loss64"] = l32, l64
        meta["cases"][name] = dict(lc, gap=gap, bound=bound)
        print(f"  loop {name}: loss {l32[0]:.4f} -> {l32[-1]:.4f}  fp32-vs-fp64 gap {gap:.3g}  bound {bound:.3g}")
    path = OUT / f"{U.LOOP_FIXTURE}.npz"
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"  wrote {path.name}: {path.stat().st_size / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
