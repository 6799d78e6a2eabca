#!/usr/bin/env python3
"""Generate tests/golden/train_ternary_*.npz by running the REFERENCE TernarySparseAutoencoder forward, loss.backward() and
STEWeights.init_mask / update_mask (container-only, CPU).

Weights and inputs come from the portable PRNG recipes of tests/train_ternary_util.py (quantizedsae_amd/synthetic.py), loaded
into the reference classes (tools/ref_loader.py).  Every recipe must make the reference itself unambiguous, which is checked
here and recorded in the fixture's meta: the smallest |encoder pre-activation| of the batch (the ReLU edge) must be > 0 (a
seed below 3e-5, ten times the worst rounding of a 64-term fp32 chain of O(1) terms, is advanced by 1000); for every
exactly-k selection the two keys either side of the boundary must differ, so that torch.topk's tie order cannot matter; a and delta are fed to the reference as one-row tensors, whose means are exact.
Only data is written: the recipe and seed, the reference's outputs, loss, gradients, masks (packed bits) and weights.
train_ternary_loop.npz holds the losses of 30 steps of the t_sae branch of training/trainer.py on a fixed batch, run once in
fp32 and once with the reference model in fp64, the largest relative gap between the two runs, the bound the GPU loop is held
to (ten times that gap, at least 1e-5), and the final mask.

Run:  python tools/gen_golden_train_ternary.py        (needs the reference checkout; CPU only, seconds)
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

import train_ternary_util as U  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
MIN_ABS_PRE = 3e-5
MAX_BYTES = 600 * 1024
MAX_LOOP_GAP = 1e-2


def build(ref, D: int, H: int, sd: dict, dtype=torch.float32):
    model = ref.TernarySparseAutoencoder(D, H)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(dtype)


def init_boundary(w: torch.Tensor, sparsity: float):
    """(n-th, n+1-th) smallest |w| keys."""
    n = int(w.numel() * sparsity)
    keys = torch.sort(U.abs_key(w)).values
    return int(keys[n - 1]), int(keys[n])


def checked_init_mask(model, sparsity: float) -> dict:
    """Runs the reference's init_mask, requires its boundary to be unambiguous and the restatement to reproduce it."""
    w0 = model.decoder.weight.detach().clone()
    lo, hi = init_boundary(w0, sparsity)
    assert lo != hi, "init_mask boundary is tied"
    model.decoder.init_mask(sparsity)
    w_ref, m_ref = U.init_mask_ref(w0, sparsity)
    assert torch.equal(m_ref, model.decoder.mask) and torch.equal(w_ref.view(torch.int32), model.decoder.weight.detach().view(torch.int32))
    return {"init_key": lo, "init_next_key": hi}


def save(name: str, meta: dict, arrays: dict):
    path = OUT / f"{name}.npz"
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    size = path.stat().st_size
    assert size <= MAX_BYTES, f"{path.name} is {size} bytes"
    return size


def run_case(ref, case: dict, seed: int):
    sd, x_np = U.case_inputs(case, seed)
    model = build(ref, case["D"], case["H"], sd)
    bounds = checked_init_mask(model, U.SPARSITY)
    x = torch.from_numpy(x_np).requires_grad_(True)
    with torch.no_grad():
        gap = float(model.encoder[0](x).abs().min())
    h, recon = model(x)
    loss = F.mse_loss(recon, x.detach())
    if case["l1"] > 0:
        loss = loss + case["l1"] * h.abs().mean()
    loss.backward()
    dec = model.decoder
    arrays = {"loss": np.float64(loss.item()), "min_abs_pre": np.float64(gap),
              "h": h.detach().numpy(), "recon": recon.detach().numpy(), "mask": U.pack_mask(dec.mask.numpy()),
              "a": dec.input_activations.mean(0).numpy(), "delta": dec.output_grad.mean(0).numpy(),
              "grad.x": x.grad.numpy()}
    for pname, p in model.named_parameters():
        arrays["grad." + pname] = p.grad.numpy().astype(np.float32)
    g_before = dec.weight.grad.clone()
    dec.mask_grad()
    assert torch.equal(g_before, dec.weight.grad), "the reference's autograd gradient is already masked"
    return gap, bounds, arrays


def run_mask_case(ref, case: dict):
    D, H, seed = case["D"], case["H"], case["seed"]
    w0, a, delta = U.mask_case_inputs(case, seed)
    dec = ref.STEWeights(H, D)
    with torch.no_grad():
        dec.weight.copy_(torch.from_numpy(w0))
    lo, hi = init_boundary(dec.weight.detach(), U.SPARSITY)
    assert lo != hi
    dec.init_mask(U.SPARSITY)
    w_i, m_i = U.init_mask_ref(torch.from_numpy(w0), U.SPARSITY)
    assert torch.equal(m_i, dec.mask) and torch.equal(w_i.view(torch.int32), dec.weight.detach().view(torch.int32))
    n = U.update_n(D * H, case["f_decay"])
    if case["ties"]:
        with torch.no_grad():
            dec.weight.copy_(U.plant_drop_ties(dec.weight.detach(), dec.mask, n))
    w1, m1 = dec.weight.detach().clone(), dec.mask.clone()
    if case["stats"]:
        dec.input_activations = torch.from_numpy(a)[None, :]
        dec.output_grad = torch.from_numpy(delta)[None, :]
    dec.update_mask(case["f_decay"], U.SPARSITY)
    w2, m2, info = U.update_mask_ref(w1, m1, None if a is None else torch.from_numpy(a),
                                     None if delta is None else torch.from_numpy(delta), n)
    assert torch.equal(m2, dec.mask), "the mask restatement differs from the reference"
    assert torch.equal(w2.view(torch.int32), dec.weight.detach().view(torch.int32))
    if "grow_key" in info:
        assert info["grow_key"] != info["grow_next_key"], "grow boundary is tied"
    if case["ties"]:
        assert int(info["dropped"].sum()) > n, "the planted ties did not reach the drop threshold"
    meta = dict(case, n=n, init_key=lo, init_next_key=hi, dropped=int(info["dropped"].sum()), grown=int(info["grown"].sum()),
                regrown=int((info["dropped"] & info["grown"]).sum()), active_after=int(m2.sum()),
                **{k: info[k] for k in ("drop_key", "drop_next_key", "grow_key", "grow_next_key") if k in info})
    arrays = {"mask_init": U.pack_mask(m1.numpy()), "mask_after": U.pack_mask(dec.mask.numpy()),
              "weight_before": w1.numpy(), "weight_after": dec.weight.detach().numpy()}
    return meta, arrays


def run_loop(ref, dtype):
    L = U.LOOP
    sd = U.S.ternary_sae_params(L["seed"], L["D"], L["H"])
    model = build(ref, L["D"], L["H"], sd)
    checked_init_mask(model, U.SPARSITY)
    model = model.to(dtype)
    x = torch.from_numpy(U.S.activations(L["seed"], L["B"], L["D"])).to(dtype)
    opt = torch.optim.Adam(model.parameters(), lr=L["lr"])
    losses = []
    for _ in range(L["steps"]):
        _, recon = model(x)
        loss = F.mse_loss(recon, x)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        model.decoder.mask_grad()
        opt.step()
        model.decoder.update_mask(L["f_decay"], U.SPARSITY)
        losses.append(float(loss.item()))
    return np.array(losses, np.float64), model.decoder.mask.detach().to(torch.float32)


def main():
    ref = load_reference()
    torch.manual_seed(0)
    OUT.mkdir(parents=True, exist_ok=True)
    for name, case in U.CASES.items():
        seed = case["seed"]
        while True:
            gap, bounds, arrays = run_case(ref, case, seed)
            if gap >= MIN_ABS_PRE:
                break
            seed += 1000
        size = save(name, dict(case, seed=seed, min_abs_pre=gap, sparsity=U.SPARSITY, **bounds), arrays)
        print(f"  wrote {name}.npz: {size / 1024:.1f} KiB  seed {seed}  min|pre| {gap:.3g}  loss {arrays['loss']:.6g}")
    for name, case in U.MASK_CASES.items():
        meta, arrays = run_mask_case(ref, case)
        size = save(name, meta, arrays)
        print(f"  wrote {name}.npz: {size / 1024:.1f} KiB  n {meta['n']}  dropped {meta['dropped']}  grown {meta['grown']}  "
              f"regrown {meta['regrown']}  active {meta['active_after']}")
    (l32, m32), (l64, m64) = run_loop(ref, torch.float32), run_loop(ref, torch.float64)
    gap = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
    assert gap <= MAX_LOOP_GAP, f"loop recipe unfit: fp32-to-fp64 gap {gap}"
    bound = max(10.0 * gap, 1e-5)
    meta = dict(U.LOOP, sparsity=U.SPARSITY, gap=gap, bound=bound, active_final=int(m32.sum()),
                mask_diff_fp32_fp64=int((m32 != m64).sum()))
    size = save(U.LOOP_FIXTURE, meta, {"loss32": l32, "loss64": l64, "mask_final": U.pack_mask(m32.numpy())})
    print(f"  wrote {U.LOOP_FIXTURE}.npz: {size / 1024:.1f} KiB  loss {l32[0]:.4f} -> {l32[-1]:.4f}  gap {gap:.3g}  bound {bound:.3g}  "
          f"active {meta['active_final']}  fp32/fp64 mask differences {meta['mask_diff_fp32_fp64']}")


if __name__ == "__main__":
    main()
