#!/usr/bin/env python3
"""Time the recipe around the Adam step (csrc/optim_recipe.hip) against the means the package had
before it, on the same card, with the protocol of tools/bench_optim.py: one process, the sides of a comparison alternating, a
window of `steps` iterations between two device events, median / min / max over `repeats` windows; a side counts as faster
only when its slowest window is below the other side's fastest.  One JSON line per case, at 512 -> 32768.

* every op alone, with its bytes and its share of the device-to-device copy rate measured here: grad_norm over the model's
  gradients, project_columns over the baseline decoder, adam_step_clipped with both streams over the decoder logits;
* the clipped training step: optim.Adam(max_grad_norm=) against torch.nn.utils.clip_grad_norm_(foreach=True) followed by
  optim.Adam(model=).step();
* the averaged training step: optim.Adam(ema_decay=) against the plain step followed by torch._foreach_lerp_;
* the projection: BaselineSparseAutoencoder.project_decoder_grad against its torch composition;
* the plain step with no option (--plain-only prints that alone: run it from two trees, alternating, to compare builds).

    python tools/bench_optim_recipe.py [--batches 4096 8192] [--steps 10] [--warmup 3] [--repeats 5]
                                       [--models binary baseline] [--plain-only]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_optim import D, DEV, H, LAM, LR, MIB, N_BITS, alternate, copy_rate, faster, fmt, make_model  # noqa: E402
from quantizedsae_amd import ops, synthetic as S  # noqa: E402
from quantizedsae_amd.optim import Adam  # noqa: E402

DECAY, CLIP = 0.999, 1e-3


def backward(kind, model, opt, x):
    opt.zero_grad(set_to_none=True)
    if kind == "binary":
        _, recon, pol = model.forward_train(x)
        (0.5 * F.mse_loss(recon, x) + LAM * pol).backward()
    else:
        _, recon = model.forward_train(x)
        F.mse_loss(recon, x).backward()


def finish(kind, model):
    if kind == "baseline":
        model.normalize_decoder_weights()


def with_rate(stat, nbytes, crate):
    rate = nbytes / (stat[0] * 1e-3)
    return dict(fmt(stat), traffic_MiB=round(nbytes / MIB, 1), GBps=round(rate / 1e9, 1), of_copy_rate=round(rate / crate, 3))


def bench_steps(kind, batches, args):
    names = ("plain", "hip_clip", "torch_clip", "hip_ema", "torch_ema")
    models = {w: make_model(kind) for w in names}
    opts = {"plain": Adam(models["plain"].parameters(), lr=LR, model=models["plain"]),
            "hip_clip": Adam(models["hip_clip"].parameters(), lr=LR, model=models["hip_clip"], max_grad_norm=CLIP),
            "torch_clip": Adam(models["torch_clip"].parameters(), lr=LR, model=models["torch_clip"]),
            "hip_ema": Adam(models["hip_ema"].parameters(), lr=LR, model=models["hip_ema"], ema_decay=DECAY),
            "torch_ema": Adam(models["torch_ema"].parameters(), lr=LR, model=models["torch_ema"])}
    params = {w: list(models[w].parameters()) for w in names}
    emas = [p.detach().clone() for p in params["torch_ema"]]

    def step(w, x):
        backward(kind, models[w], opts[w], x)
        if w == "torch_clip":
            torch.nn.utils.clip_grad_norm_(params[w], CLIP, foreach=True)
        opts[w].step()
        if w == "torch_ema":
            with torch.no_grad():
                torch._foreach_lerp_(emas, [p.detach() for p in params[w]], 1 - DECAY)
        finish(kind, models[w])

    for B in batches:
        x = torch.from_numpy(S.activations(8, B, D)).to(DEV)
        got = alternate({w: (lambda w=w: step(w, x)) for w in names}, args.steps, args.warmup, args.repeats)
        out = {"what": "train_step", "model": kind, "B": B, "D": D, "H": H, "steps": args.steps, "repeats": args.repeats}
        out.update({w: fmt(s) for w, s in got.items()})
        out["hip_clip_faster_than_torch_clip"] = faster(got["hip_clip"], got["torch_clip"])
        out["torch_clip_faster_than_hip_clip"] = faster(got["torch_clip"], got["hip_clip"])
        out["hip_ema_faster_than_torch_ema"] = faster(got["hip_ema"], got["torch_ema"])
        out["torch_ema_faster_than_hip_ema"] = faster(got["torch_ema"], got["hip_ema"])
        print(json.dumps(out), flush=True)

    # the ops alone, on the gradients the last step left
    model = models["plain"]
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    gbytes = sum(g.numel() for g in grads) * 4
    coef, report = ops.grad_norm(grads, CLIP)
    cstat, crate = copy_rate(gbytes // 2, args)
    got = alternate({"grad_norm": lambda: ops.grad_norm(grads, CLIP, coef, report),
                     "torch_get_total_norm": lambda: torch.nn.utils.get_total_norm(grads, foreach=True)},
                    args.steps, args.warmup, args.repeats)
    out = {"what": "grad_norm_alone", "model": kind, "tensors": len(grads), "copy_GBps": round(crate / 1e9, 1),
           "grad_norm": with_rate(got["grad_norm"], gbytes, crate), "torch_get_total_norm": fmt(got["torch_get_total_norm"])}
    print(json.dumps(out), flush=True)
    if kind == "baseline":
        w, g = model.decoder.weight, model.decoder.weight.grad
        mine = models["hip_clip"]
        mine.decoder.weight.grad = g.clone()

        def composition():
            dot = (g * w).sum(dim=0, keepdim=True)
            g.addcmul_(dot, w, value=-1)
        with torch.no_grad():
            got = alternate({"project_columns": mine.project_decoder_grad, "torch_composition": composition},
                            args.steps, args.warmup, args.repeats)
        nbytes = 3 * w.numel() * 4                                 # W and G read, G written (the second read of the strip: cache)
        cstat, crate = copy_rate(nbytes // 2, args)
        out = {"what": "project_columns", "D": D, "H": H, "copy_GBps": round(crate / 1e9, 1),
               "project_columns": with_rate(got["project_columns"], nbytes, crate), "torch_composition": fmt(got["torch_composition"]),
               "hip_faster": faster(got["project_columns"], got["torch_composition"]),
               "torch_faster": faster(got["torch_composition"], got["project_columns"])}
        print(json.dumps(out), flush=True)


def bench_flat(args):
    sc = (0.1, 0.999, 0.001, 0.0547, 1e-8, 1e-3)
    gen = torch.Generator(device=DEV).manual_seed(3)
    n = H * D * N_BITS                                             # the decoder logits: 67 M elements, 256 MiB
    p, g, m = (torch.randn((n,), device=DEV, generator=gen) for _ in range(3))
    v = torch.rand((n,), device=DEV, generator=gen) * 1e-3
    e, c = p.clone(), torch.full((1,), 0.5, device=DEV)
    got = alternate({"adam_step": lambda: ops.adam_step(p, g, m, v, *sc),
                     "adam_step_clipped_null": lambda: ops.adam_step_clipped(p, g, m, v, *sc),
                     "adam_step_clipped_coef": lambda: ops.adam_step_clipped(p, g, m, v, *sc, coef=c),
                     "adam_step_clipped_coef_ema": lambda: ops.adam_step_clipped(p, g, m, v, *sc, coef=c, ema=e,
                                                                                 one_minus_decay=1 - DECAY)},
                    args.steps, args.warmup, args.repeats)
    cstat, crate = copy_rate(9 * n * 4 // 2, args)
    out = {"what": "adam_step_clipped_decoder_logits", "n": n, "copy_GBps": round(crate / 1e9, 1)}
    for name, stat in got.items():
        out[name] = with_rate(stat, (9 if name.endswith("ema") else 7) * n * 4, crate)
    print(json.dumps(out), flush=True)


def plain_only(args):
    """The training step with no option: what a build before the recipe also runs."""
    for kind in args.models:
        model = make_model(kind)
        opt = Adam(model.parameters(), lr=LR, model=model)
        for B in args.batches:
            x = torch.from_numpy(S.activations(8, B, D)).to(DEV)

            def step():
                backward(kind, model, opt, x)
                opt.step()
                finish(kind, model)
            stat = alternate({"plain": step}, args.steps, args.warmup, args.repeats)["plain"]
            print(json.dumps({"what": "plain_train_step", "model": kind, "B": B, "plain": fmt(stat)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--models", nargs="*", default=["binary", "baseline"], choices=["binary", "baseline"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="the plain training step alone (to compare two trees)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_recipe.py needs cuda:0 (MI355X); nothing is timed without it")
    if args.plain_only:
        plain_only(args)
        return
    for kind in args.models:
        bench_steps(kind, args.batches, args)
        torch.cuda.empty_cache()
    bench_flat(args)


if __name__ == "__main__":
    main()
