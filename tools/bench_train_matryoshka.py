#!/usr/bin/env python3
"""Time one QuantizedMatryoshkaSAE training step on the GPU -- forward_train, the q_sae loss, backward, apply_secant_grad,
Adam.step (the q_sae branch of trainer.py:88-112) -- against the same step in eager torch on the same card: the reference's op
sequence (sigmoid encoder, straight-through binarisation of latent and decoder logits, per-level scaled matmul on a detached
running reconstruction, autograd, the secant update, Adam) restated here with plain torch ops.  Sparse (~0.6 % of the units
fire) and 50 %-dense weights, decoder_grad_path "dense" against "lists", forward_train and backward alone, and with
--crossover the two decoder-gradient paths over a range of activation densities.

Every comparison is timed in one process, its sides alternating; a window is `steps` iterations between two device events
and ends in a synchronise; the figures are the median and the range over `repeats` windows.  One JSON line per case.

    python tools/bench_train_matryoshka.py [--batches 4096 8192] [--steps 20] [--warmup 3] [--repeats 5] [--crossover]
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

from quantizedsae_amd import QuantizedMatryoshkaSAE, synthetic as S  # noqa: E402
from quantizedsae_amd.sae.quantized_matryoshka import nested_sizes  # noqa: E402

D, H, N_BITS, ABS_RANGE, LAM = 512, 32768, 4, 1.5, 1.5e-3
DEV = "cuda:0"


def eager_step(params, opt, x):
    """The reference's step restated in eager torch: dense [B, H] latent, dense matmuls, autograd."""
    W, b, w, wm, bias = params
    B = x.shape[0]
    latent = torch.sigmoid(F.linear(x, W, b))
    quant_step = ABS_RANGE / 2 ** (N_BITS - 1)
    recon = torch.zeros_like(x)
    groups, recs, ctx, s = [], [], [], 0
    for i, size in enumerate(nested_sizes(H, N_BITS)):
        sw, swm = torch.sigmoid(w[s:s + size]), torch.sigmoid(wm[s:s + size])
        Bs = torch.where(sw >= 0.5, 1.0, -1.0)
        Bm = torch.where(swm >= 0.5, 1.0, -1.0)
        scale = (2 ** (N_BITS - i - 2) * quant_step) / (torch.norm(Bs + Bm, p=2, dim=1) + 1e-8)
        ste = ((Bs - sw).detach() + sw) + ((Bm - swm).detach() + swm)
        lat = latent[:, s:s + size]
        lat = ((lat > 0.5).to(lat.dtype) - lat).detach() + lat
        recon = recon.detach() + (scale * lat) @ ste
        if i == 0:
            recon = recon + bias
        groups.append(lat.sum(dim=-1).mean())
        recs.append(recon)
        ctx.append((s, size, scale, Bs, Bm, lat.sum(dim=0).detach(), sw.detach(), swm.detach()))
        s += size
    loss = sum(0.5 * F.mse_loss(r, x) for r in recs) + sum(groups) * LAM
    opt.zero_grad()
    loss.backward()
    with torch.no_grad():
        c = 1.0 / B / D
        for s, size, scale, Bs, Bm, cnt, sw, swm in ctx:
            coef = (c * cnt * scale ** 2)[:, None]
            w.grad[s:s + size].add_(-coef * Bs * sw * (1.0 - sw))
            wm.grad[s:s + size].add_(-coef * Bm * swm * (1.0 - swm))
    opt.step()
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


def make_model(sd, path):
    m = QuantizedMatryoshkaSAE(D, H, 32, abs_range=ABS_RANGE, n_bits=N_BITS)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.decoder_grad_path = path
    return m.to(DEV)


def q_loss(x, groups, levels):
    return sum(0.5 * F.mse_loss(r, x) for r in levels) + sum(groups) * LAM


def hip_step(model, opt, x):
    groups, levels = model.forward_train(x)
    loss = q_loss(x, groups, levels)
    opt.zero_grad()
    loss.backward()
    model.decoder.apply_secant_grad()
    opt.step()
    return loss


def backward_alone_ms(model, x, n):
    out = []
    for _ in range(n):
        model.zero_grad(set_to_none=True)
        groups, levels = model.forward_train(x)
        loss = q_loss(x, groups, levels)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--crossover", action="store_true", help="dense against lists over a range of activation densities")
    ap.add_argument("--hip-only", action="store_true", help="the HIP step alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_matryoshka.py needs cuda:0 (MI355X); nothing is timed without it")

    if args.crossover:
        B = max(args.batches)
        x = torch.from_numpy(S.activations(8, B, D)).to(DEV)
        for sigmas in (-2.5, -2.0, -1.75, -1.5, -1.25, -1.0, -0.5, 0.0):
            sd = S.matryoshka_sae_params(7, D, H, bias_std=0.1, enc_bias_sigmas=sigmas)
            models = {p: make_model(sd, p) for p in ("dense", "lists")}
            with torch.no_grad():
                frac = models["dense"].decoder.active_fraction(models["dense"].activation_bits(x, "dense"))
            steps = max(2, args.steps // 4)
            out = {"what": "crossover", "B": B, "sigmas": sigmas, "active_fraction": round(frac, 5)}
            for p, m in models.items():
                out[f"backward_{p}"] = fmt(backward_alone_ms(m, x, steps))
            print(json.dumps(out), flush=True)
            del models
        return

    for density, sigmas in (("sparse", -2.5), ("dense", 0.0)):
        sd = S.matryoshka_sae_params(7, D, H, bias_std=0.1, enc_bias_sigmas=sigmas)
        for B in args.batches:
            x = torch.from_numpy(S.activations(8, B, D)).to(DEV)
            out = {"what": "step", "weights": density, "B": B, "D": D, "H": H, "n_bits": N_BITS, "steps": args.steps,
                   "repeats": args.repeats}
            models = {p: make_model(sd, p) for p in ("dense", "lists")}
            opts = {p: torch.optim.Adam(m.parameters(), lr=1e-4) for p, m in models.items()}
            with torch.no_grad():
                out["active_fraction"] = round(models["dense"].decoder.active_fraction(
                    models["dense"].activation_bits(x, "dense")), 5)
            sides = {}
            if not args.hip_only:
                params = [torch.from_numpy(sd[k]).to(DEV).requires_grad_(True)
                          for k in ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.weight_mirror", "decoder.bias")]
                ropt = torch.optim.Adam(params, lr=1e-4)
                sides["eager_reference_step"] = lambda: eager_step(params, ropt, x)
            sides["hip_step_dense"] = lambda: hip_step(models["dense"], opts["dense"], x)
            if density == "sparse":                      # at 50 % the lists gather hundreds of GB: timed once below
                sides["hip_step_lists"] = lambda: hip_step(models["lists"], opts["lists"], x)
            for key, stat in alternate(sides, args.steps, args.warmup, args.repeats).items():
                out[key] = fmt(stat)
            if density == "dense" and not args.hip_only:
                out["hip_step_lists"] = fmt(alternate({"l": lambda: hip_step(models["lists"], opts["lists"], x)}, 2, 1, 3)["l"])
            if not args.hip_only:
                paths = ("dense", "lists") if density == "sparse" else ("dense",)
                for p in paths:
                    fw = alternate({"f": lambda p=p: models[p].forward_train(x)}, args.steps, args.warmup, args.repeats)["f"]
                    out[f"hip_forward_train_{p}"] = fmt(fw)
                    out[f"hip_backward_{p}"] = fmt(backward_alone_ms(models[p], x, args.steps))
                with torch.no_grad():
                    out["hip_forward"] = fmt(alternate({"f": lambda: models["dense"](x)}, args.steps, args.warmup,
                                                       args.repeats)["f"])
                ref = out["eager_reference_step"]["median_ms"]
                for p in ("dense", "lists"):
                    out[f"speedup_{p}"] = round(ref / out[f"hip_step_{p}"]["median_ms"], 2)
            print(json.dumps(out), flush=True)
            del models, opts, sides


if __name__ == "__main__":
    main()
