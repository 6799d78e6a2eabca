#!/usr/bin/env python3
"""Time one TernarySparseAutoencoder training step on the GPU -- forward_train, mse_loss, backward, mask_grad, Adam.step,
update_mask (the t_sae branch of trainer.py:157-164) -- against the same step in eager torch on the same card: the reference's
op sequence (ReLU encoder, straight-through ternary dictionary over weight * mask, autograd, the kthvalue / outer / topk mask
update) restated here with plain torch ops.  Also update_mask and init_mask alone against their torch sequences, and
forward_train / backward alone.

Every comparison is timed in one process, its sides alternating; a window is `steps` iterations between two device events
and ends in a synchronise; the figures are the median and the range over `repeats` windows.  One JSON line per case.

    python tools/bench_train_ternary.py [--batches 4096 8192] [--steps 10] [--warmup 2] [--repeats 5] [--hip-only]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from quantizedsae_amd import TernarySparseAutoencoder, synthetic as S  # noqa: E402

D, H, SPARSITY, F_DECAY = 512, 32768, 0.7, 0.3
DEV = "cuda:0"


def eager_init_mask(w, mask, sparsity):
    with torch.no_grad():
        n = int(w.numel() * sparsity)
        _, idx = torch.topk(w.abs().flatten(), n, largest=False)
        m = torch.ones_like(w).flatten()
        m[idx] = 0
        mask.copy_(m.view_as(w))
        w.mul_(mask)


def eager_update_mask(w, mask, a, delta, f_decay, sparsity_rate=SPARSITY):
    """sae/ternary.py:54-87 with a = input_activations.mean(0), delta = output_grad.mean(0) given (None: drop only)."""
    with torch.no_grad():
        flat = w.flatten()
        active = mask.flatten().bool()
        n = int(f_decay * (1 - sparsity_rate) * flat.size(0))
        if n > 0:
            thr = torch.kthvalue(flat[active].abs(), k=n)[0]
            active[(flat.abs() <= thr) & active] = False
        if n > 0 and a is not None:
            scores = torch.outer(delta.abs(), a.abs()).flatten()
            scores[active] = -float("inf")
            _, grow = torch.topk(scores, n)
            active[grow] = True
        mask.copy_(active.view_as(mask).float())
        w.mul_(mask)


def eager_step(params, mask, opt, x):
    """The reference's step restated in eager torch: dense latent, straight-through dictionary, autograd, RigL update."""
    W, b, w = params
    h = torch.relu(F.linear(x, W, b))
    with torch.no_grad():
        hard = torch.sign(w) * (w.abs() >= 0.5).float()
    mw = w * mask
    recon = F.linear(h, mw + (hard - mw).detach())
    recon.retain_grad()
    loss = F.mse_loss(recon, x)
    opt.zero_grad()
    loss.backward()
    w.grad.mul_(mask)
    opt.step()
    eager_update_mask(w, mask, h.detach().mean(0), recon.grad.mean(0), F_DECAY)
    return loss


def hip_step(model, opt, x):
    _, recon = model.forward_train(x)
    loss = F.mse_loss(recon, x)
    opt.zero_grad()
    loss.backward()
    model.decoder.mask_grad()
    opt.step()
    model.decoder.update_mask(F_DECAY, SPARSITY)
    return loss


def window_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def alternate(sides: dict, steps, warmup, repeats):
    """{name: fn} -> {name: (median ms, min ms, max ms)}: every side warmed up, then `repeats` rounds of one window each."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            got[name].append(window_ms(fn, steps))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def fmt(stat):
    return {"median_ms": round(stat[0], 4), "min_ms": round(stat[1], 4), "max_ms": round(stat[2], 4)}


def backward_alone_ms(model, x, n):
    out = []
    for _ in range(n):
        model.zero_grad(set_to_none=True)
        _, recon = model.forward_train(x)
        loss = F.mse_loss(recon, x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def make_model(sd):
    m = TernarySparseAutoencoder(D, H)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV)
    m.decoder.init_mask(SPARSITY)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="the HIP step alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_ternary.py needs cuda:0 (MI355X); nothing is timed without it")
    sd = S.ternary_sae_params(7, D, H)

    for B in args.batches:
        x = torch.from_numpy(S.activations(8, B, D)).to(DEV)
        out = {"what": "step", "B": B, "D": D, "H": H, "f_decay": F_DECAY, "steps": args.steps, "repeats": args.repeats}
        model = make_model(sd)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        sides = {}
        if not args.hip_only:
            params = [model.state_dict()[k].detach().clone().requires_grad_(True)
                      for k in ("encoder.0.weight", "encoder.0.bias", "decoder.weight")]
            rmask = model.decoder.mask.clone()
            ropt = torch.optim.Adam(params, lr=1e-4)
            sides["eager_reference_step"] = lambda: eager_step(params, rmask, ropt, x)
        sides["hip_step"] = lambda: hip_step(model, opt, x)
        for key, stat in alternate(sides, args.steps, args.warmup, args.repeats).items():
            out[key] = fmt(stat)
        out["active_positions"] = int(model.decoder.mask.sum())
        if not args.hip_only:
            out["hip_forward_train"] = fmt(alternate({"f": lambda: model.forward_train(x)}, args.steps, args.warmup,
                                                     args.repeats)["f"])
            out["hip_backward"] = fmt(backward_alone_ms(model, x, args.steps))
            with torch.no_grad():
                out["hip_forward"] = fmt(alternate({"f": lambda: model(x)}, args.steps, args.warmup, args.repeats)["f"])
            out["speedup"] = round(out["eager_reference_step"]["median_ms"] / out["hip_step"]["median_ms"], 2)
        print(json.dumps(out), flush=True)
        del model, opt, sides

    if args.hip_only:
        return
    # the mask updates alone: both sides restart from the same weights / mask / statistics in every iteration (the copies are
    # timed on both sides alike)
    model = make_model(sd)
    dec = model.decoder
    w0 = torch.from_numpy(sd["decoder.weight"]).to(DEV)
    w1, m1 = dec.weight.detach().clone(), dec.mask.clone()
    a = torch.from_numpy(S.normal(9, (H,), stream=5)).abs().to(DEV)
    delta = (torch.from_numpy(S.normal(9, (D,), stream=6)) * 1e-3).to(DEV)
    we, me = w1.clone(), m1.clone()

    def hip_update(stats):
        with torch.no_grad():
            dec.weight.copy_(w1)
            dec.mask.copy_(m1)
        dec.activation_mean, dec.output_grad_mean = (a, delta) if stats else (None, None)
        dec.update_mask(F_DECAY, SPARSITY)

    def eager_update(stats):
        we.copy_(w1)
        me.copy_(m1)
        eager_update_mask(we, me, a if stats else None, delta if stats else None, F_DECAY)

    def hip_init():
        with torch.no_grad():
            dec.weight.copy_(w0)
        dec.init_mask(SPARSITY)

    def eager_init():
        we.copy_(w0)
        eager_init_mask(we, me, SPARSITY)

    def copies():
        we.copy_(w1)
        me.copy_(m1)

    for what, sides in (("update_mask", {"eager": lambda: eager_update(True), "hip": lambda: hip_update(True)}),
                        ("update_mask_drop_only", {"eager": lambda: eager_update(False), "hip": lambda: hip_update(False)}),
                        ("init_mask", {"eager": eager_init, "hip": hip_init}),
                        ("restore_copies_alone", {"copies": copies})):
        out = {"what": what, "D": D, "H": H, "n": int(F_DECAY * (1 - SPARSITY) * D * H)}
        for key, stat in alternate(sides, args.steps, args.warmup, args.repeats).items():
            out[key] = fmt(stat)
        print(json.dumps(out), flush=True)
    eager_init()
    hip_init()
    print(json.dumps({"what": "init_mask_sides_differ_at", "positions": int((dec.mask != me).sum())}), flush=True)


if __name__ == "__main__":
    main()
