#!/usr/bin/env python3
"""Time one BaselineSparseAutoencoder training step on the GPU -- forward_train, mse_loss, backward, Adam.step,
normalize_decoder_weights (the baseline_sae branch of trainer.py:166-173) -- against the reference's op sequence in eager
torch on the same card: dense F.linear, torch.topk, scatter_, dense F.linear, autograd, Adam.step and the three-op
normalisation (sae/baseline.py:17-51), restated here.  Also forward_train and loss.backward() alone, the step with
latent_path "prefilter" against "fused", and the normalisation kernel against the three torch ops.

Every comparison is timed in one process, its sides alternating; a window is `steps` iterations between two device events
and ends in a synchronise; the figures are the median and the range over `repeats` windows.  One JSON line per batch size.

    python tools/bench_train_baseline.py [--batches 4096 8192] [--steps 30] [--warmup 5] [--repeats 5]
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

from quantizedsae_amd import BaselineSparseAutoencoder, ops, synthetic as S  # noqa: E402

D, H, K = 512, 32768, 32
DEV = "cuda:0"


def eager_normalize(W_dec):
    """sae/baseline.py:42-51: norm, clamp, divide (three full passes and a fresh tensor)."""
    with torch.no_grad():
        w = W_dec.data
        W_dec.data = w / torch.clamp(torch.norm(w, dim=0, keepdim=True), min=1e-8)


def eager_reference_step(params, opt, x, k):
    """The reference's step in eager torch (dense [B, H] latent, dense GEMMs; sae/baseline.py:17-40, trainer.py:166-173)."""
    W, b, W_dec, b_dec = params
    h = F.linear(x, W, b)
    vals, ids = torch.topk(h, k, dim=1)
    h_sparse = torch.zeros_like(h)
    h_sparse.scatter_(1, ids, vals)
    recon = F.linear(h_sparse, W_dec, b_dec)
    loss = F.mse_loss(recon, x)
    opt.zero_grad()
    loss.backward()
    opt.step()
    eager_normalize(W_dec)
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
    m = BaselineSparseAutoencoder(D, H)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.topk = K
    m.latent_path = path
    return m.to(DEV)


def hip_step(model, opt, x, dense):
    latent, recon = model.forward_train(x, dense_latent=dense)
    loss = F.mse_loss(recon, x)
    opt.zero_grad()
    loss.backward()
    opt.step()
    model.normalize_decoder_weights()
    return loss


def backward_alone_ms(model, x, dense, n):
    out = []
    for _ in range(n):
        model.zero_grad(set_to_none=True)
        _, recon = model.forward_train(x, dense_latent=dense)
        loss = F.mse_loss(recon, x)
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_baseline.py needs cuda:0 (MI355X); nothing is timed without it")
    sd = S.baseline_sae_params(7, D, H, bias_std=0.1)

    # the normalisation alone: one pass in place + the transposed table, against norm / clamp / divide (+ the transpose the
    # next forward would make of the result)
    Wk = torch.from_numpy(sd["decoder.weight"]).to(DEV)
    We = torch.nn.Parameter(Wk.clone())
    norm = alternate({
        "hip_normalize_with_table": lambda: ops.normalize_columns_table(Wk, want_table=True),
        "hip_normalize_no_table": lambda: ops.normalize_columns_table(Wk, want_table=False),
        "eager_normalize_three_ops": lambda: eager_normalize(We),
        "eager_normalize_plus_transpose": lambda: (eager_normalize(We), We.data.t().contiguous()),
    }, 200, 20, args.repeats)
    print(json.dumps({"what": "normalize", "D": D, "H": H, **{k: fmt(v) for k, v in norm.items()}}), flush=True)
    del Wk, We

    for B in args.batches:
        x = torch.from_numpy(S.activations(8, B, D)).to(DEV)
        out = {"what": "step", "B": B, "D": D, "H": H, "k": K, "steps": args.steps, "repeats": args.repeats}
        models = {name: make_model(sd, path) for name, path in
                  (("auto", "auto"), ("prefilter", "prefilter"), ("fused", "fused"))}
        opts = {name: torch.optim.Adam(m.parameters(), lr=1e-4) for name, m in models.items()}
        params = [torch.from_numpy(sd[k]).to(DEV).requires_grad_(True)
                  for k in ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.bias")]
        ropt = torch.optim.Adam(params, lr=1e-4)
        sides = {"eager_reference_step": lambda: eager_reference_step(params, ropt, x, K)}
        for name in models:
            for dense in (True, False):
                sides[f"hip_step_{name}_dense{int(dense)}"] = \
                    (lambda n=name, d=dense: hip_step(models[n], opts[n], x, d))
        for key, stat in alternate(sides, args.steps, args.warmup, args.repeats).items():
            out[key] = fmt(stat)
        for name in ("auto", "fused"):
            for dense in (True, False):
                fw = alternate({"f": lambda n=name, d=dense: models[n].forward_train(x, dense_latent=d)},
                               args.steps, args.warmup, args.repeats)["f"]
                out[f"hip_forward_train_{name}_dense{int(dense)}"] = fmt(fw)
                out[f"hip_backward_{name}_dense{int(dense)}"] = fmt(backward_alone_ms(models[name], x, dense, args.steps))
        with torch.no_grad():
            out["hip_forward_auto"] = fmt(alternate({"f": lambda: models["auto"](x)}, args.steps, args.warmup,
                                                    args.repeats)["f"])
        ref = out["eager_reference_step"]["median_ms"]
        for name in models:
            for dense in (1, 0):
                out[f"speedup_{name}_dense{dense}"] = round(ref / out[f"hip_step_{name}_dense{dense}"]["median_ms"], 2)
        print(json.dumps(out), flush=True)
        del models, opts, params, ropt, sides


if __name__ == "__main__":
    main()
