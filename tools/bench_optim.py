#!/usr/bin/env python3
"""Time the optimizer step in HIP (quantizedsae_amd.optim.Adam, csrc/optim.hip) against torch.optim.Adam, default and
fused=True, on the same card: the full training step of tools/bench_train.py (BinarySAE 512 -> 32768, n_bits = 4) and of
tools/bench_train_baseline.py (BaselineSparseAutoencoder 512 -> 32768) with each of the three optimizers, the optimizer step
alone, and the kernels alone -- adam_step_prefilter against adam_step on the encoder pair followed by prefilter_pack_w, and
adam_step over the 256 MiB of decoder logits -- with a device-to-device copy of the same byte count as the yardstick.
The fused=True side calls model.invalidate_packed() after each step: torch's fused Adam does not move the parameters'
version counters, and without that call the model would go on selecting with the fp16 copy of the old weights.

Every comparison is timed in one process, its sides alternating; a window is `steps` iterations between two device events
and ends in a synchronise; the figures are the median and the range over `repeats` windows.  One JSON line per case.  A side
is "faster" when its slowest window beats the other side's fastest.

    python tools/bench_optim.py [--batches 4096 8192] [--steps 10] [--warmup 3] [--repeats 5] [--models binary baseline]
                                [--hip-only]      (--hip-only: the BinarySAE step with optim.Adam alone, for a kernel trace)
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

from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, ops, synthetic as S  # noqa: E402
from quantizedsae_amd.optim import Adam  # noqa: E402

D, H, N_BITS, GAMMA, LAM, LR = 512, 32768, 4, 4.0, 1e-2, 1e-4
DEV = "cuda:0"
MIB = 1 << 20


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


def faster(new, old):
    """the new side's slowest window below the old side's fastest"""
    return bool(new[2] < old[1])


def make_model(kind):
    if kind == "binary":
        m = BinarySAE(D, H, gamma=GAMMA, n_bits=N_BITS)
        sd = S.binary_sae_params(7, D, H, N_BITS, logit_std=1.0, dec_bias_std=0.1)
    else:
        m = BaselineSparseAutoencoder(D, H)
        sd = S.baseline_sae_params(7, D, H)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def make_optimizer(which, model):
    if which == "torch_adam":
        return torch.optim.Adam(model.parameters(), lr=LR)
    if which == "torch_adam_fused":
        return torch.optim.Adam(model.parameters(), lr=LR, fused=True)
    return Adam(model.parameters(), lr=LR, model=model)


def train_step(kind, model, opt, x, invalidate=False):
    """``invalidate``: torch.optim.Adam(fused=True) updates the parameters without moving their version counters, so the
    model's derived copies (the fp16 prefilter copy among them) would silently stay those of the old weights; a correct loop
    around it calls invalidate_packed() after every step, and that is the loop timed here."""
    opt.zero_grad(set_to_none=True)
    if kind == "binary":
        _, recon, pol = model.forward_train(x)
        (0.5 * F.mse_loss(recon, x) + LAM * pol).backward()
        opt.step()
        if invalidate:
            model.invalidate_packed()
    else:
        _, recon = model.forward_train(x)
        F.mse_loss(recon, x).backward()
        opt.step()
        if invalidate:
            model.invalidate_packed()
        model.normalize_decoder_weights()


SIDES = ("torch_adam", "torch_adam_fused", "hip_adam")


def bench_steps(kind, batches, args):
    models = {w: make_model(kind) for w in SIDES}
    opts = {w: make_optimizer(w, models[w]) for w in SIDES}
    for B in batches:
        x = torch.from_numpy(S.activations(8, B, D)).to(DEV)
        got = alternate({w: (lambda w=w: train_step(kind, models[w], opts[w], x, invalidate=(w == "torch_adam_fused")))
                         for w in SIDES}, args.steps, args.warmup, args.repeats)
        out = {"what": "train_step", "model": kind, "B": B, "D": D, "H": H, "steps": args.steps, "repeats": args.repeats}
        out.update({w: fmt(s) for w, s in got.items()})
        out["hip_faster_than_torch_adam"] = faster(got["hip_adam"], got["torch_adam"])
        out["hip_faster_than_torch_adam_fused"] = faster(got["hip_adam"], got["torch_adam_fused"])
        print(json.dumps(out), flush=True)
    # the optimizer step alone, on the gradients the last training step left (the fused route installs the fp16 copy; the
    # torch sides leave the next forward to rebuild it, which this comparison does not charge them for)
    got = alternate({w: opts[w].step for w in SIDES}, args.steps, args.warmup, args.repeats)
    out = {"what": "optimizer_step_alone", "model": kind, "parameter_MiB": round(sum(p.numel() for p in models["hip_adam"].parameters()) * 4 / MIB, 1)}
    out.update({w: fmt(s) for w, s in got.items()})
    print(json.dumps(out), flush=True)


def copy_rate(nbytes, args):
    """-> (stat of a device-to-device copy of nbytes, bytes/s moved (read + write) at its median)"""
    src = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    stat = alternate({"copy": lambda: dst.copy_(src)}, args.steps, args.warmup, args.repeats)["copy"]
    return stat, 2 * nbytes / (stat[0] * 1e-3)


def bench_kernels(args):
    sc = (0.1, 0.999, 0.001, 0.0547, 1e-8, 1e-3)
    gen = torch.Generator(device=DEV).manual_seed(3)
    W, gW, mW = (torch.randn((H, D), device=DEV, generator=gen) * 0.05 for _ in range(3))
    vW = torch.rand((H, D), device=DEV, generator=gen) * 1e-3
    b, gb, mb = (torch.randn((H,), device=DEV, generator=gen) * 0.05 for _ in range(3))
    vb = torch.rand((H,), device=DEV, generator=gen) * 1e-3
    Wq, meta = ops.prefilter_pack_w(W, b)

    def fused():
        ops.adam_step_prefilter(W, gW, mW, vW, b, gb, mb, vb, *sc, Wq=Wq, meta=meta)

    def separate():
        ops.adam_step(W, gW, mW, vW, *sc)
        ops.adam_step(b, gb, mb, vb, *sc)
        ops.prefilter_pack_w(W, b)

    def adam_pair():
        ops.adam_step(W, gW, mW, vW, *sc)
        ops.adam_step(b, gb, mb, vb, *sc)

    got = alternate({"adam_step_prefilter": fused, "adam_step_then_pack_w": separate, "adam_step_pair": adam_pair,
                     "prefilter_pack_w": lambda: ops.prefilter_pack_w(W, b)}, args.steps, args.warmup, args.repeats)
    wbytes = H * D * 4
    traffic = {"adam_step_prefilter": 8 * wbytes + wbytes // 2, "adam_step_pair": 7 * wbytes,
               "prefilter_pack_w": 3 * wbytes + wbytes // 2}
    cstat, crate = copy_rate((8 * wbytes + wbytes // 2) // 2, args)
    out = {"what": "encoder_pair_kernels", "H": H, "D": D, "copy_of_the_same_bytes": fmt(cstat), "copy_GBps": round(crate / 1e9, 1)}
    for name, stat in got.items():
        out[name] = fmt(stat)
        if name in traffic:
            rate = traffic[name] / (stat[0] * 1e-3)
            out[name].update(traffic_MiB=traffic[name] // MIB, GBps=round(rate / 1e9, 1), of_copy_rate=round(rate / crate, 3))
    out["fused_faster_than_separate"] = faster(got["adam_step_prefilter"], got["adam_step_then_pack_w"])
    print(json.dumps(out), flush=True)
    del W, gW, mW, vW, Wq

    n = H * D * N_BITS                                             # the decoder logits: 67 M elements, 256 MiB
    p, g, m = (torch.randn((n,), device=DEV, generator=gen) for _ in range(3))
    v = torch.rand((n,), device=DEV, generator=gen) * 1e-3
    views = tuple(t[1:] for t in (p, g, m, v))                     # off the 16-byte boundary: the element-wise variant
    got = alternate({"adam_step": lambda: ops.adam_step(p, g, m, v, *sc),
                     "adam_step_unaligned": lambda: ops.adam_step(*views, *sc)}, args.steps, args.warmup, args.repeats)
    cstat, crate = copy_rate(7 * n * 4 // 2, args)
    out = {"what": "adam_step_decoder_logits", "n": n, "traffic_MiB": 7 * n * 4 // MIB, "copy_of_the_same_bytes": fmt(cstat),
           "copy_GBps": round(crate / 1e9, 1)}
    for name, stat in got.items():
        rate = 7 * n * 4 / (stat[0] * 1e-3)
        out[name] = dict(fmt(stat), GBps=round(rate / 1e9, 1), of_copy_rate=round(rate / crate, 3))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--models", nargs="*", default=["binary", "baseline"], choices=["binary", "baseline"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="the BinarySAE step with optim.Adam alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs cuda:0 (MI355X); nothing is timed without it")
    if args.hip_only:
        model = make_model("binary")
        opt = make_optimizer("hip_adam", model)
        x = torch.from_numpy(S.activations(8, args.batches[0], D)).to(DEV)
        stat = alternate({"hip_adam": lambda: train_step("binary", model, opt, x)}, args.steps, args.warmup, args.repeats)
        print(json.dumps({"what": "train_step", "model": "binary", "B": args.batches[0], "hip_adam": fmt(stat["hip_adam"])}))
        return
    for kind in args.models:
        bench_steps(kind, args.batches, args)
        torch.cuda.empty_cache()
    bench_kernels(args)


if __name__ == "__main__":
    main()
