#!/usr/bin/env python3
"""The watch step timed on the device, on the headline BinarySAE (512 -> 32768, n_bits 4) after the backward of one training
step: every parameter and every gradient, about 670 MB of fp32.

  ModelWatch.collect()   one qsae_tensor_stats call over all tensors, one host copy, the parse
  kernels only           ops.tensor_stats on the same tensors, nothing read back
  wandb's recipe         the torch restatement of log_tensor_stats (tests/watch_util.py: isfinite().all(), min().item(),
                         max().item(), histc, tolist per tensor) on the same device tensors: the baseline
  device-to-device copy  of the same bytes, for the rate: the kernel reads every byte twice, the copy reads and writes once
  Gaussian / all zeros   the kernel on tensors of the same sizes filled with N(0, 1) and with zeros: every lane of a wave in
                         one bin is the worst case of the LDS histogram

Wall-clock time around each call with a synchronise before and after (the recipe's cost is its host round trips), median
(min / max) of --reps calls after --warmup, the candidates taken in turn inside every repetition.  "spread" is (max - min) /
median of the Gaussian run.  Nothing here asserts a ratio.

usage: python tools/bench_watch.py [--reps 30] [--warmup 5] [--out profiles/watch.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

DEV = "cuda:0"
D, H, N_BITS, B = 512, 32768, 4, 8192


def alternate(fns: dict, reps: int, warmup: int) -> dict:
    """-> name: (median, min, max) in ms; the candidates run in turn inside every repetition"""
    import torch
    ts = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f} / {t[2]:.3f}) ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import watch_util as U
    from quantizedsae_amd import BinarySAE, ops, synthetic as S
    from quantizedsae_amd.training import ModelWatch

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model = BinarySAE(D, H, gamma=4.0, n_bits=N_BITS).to(DEV)
    x = torch.from_numpy(S.activations(1, B, D)).to(DEV)
    _, recon, pol = model.forward_train(x, dense_latent=False)
    (torch.nn.functional.mse_loss(recon, x) + 1e-2 * pol).backward()
    watch = ModelWatch(model, log="all")
    keys, tensors = watch._tensors()
    nbytes = sum(t.numel() for t in tensors) * 4
    say(f"device {torch.cuda.get_device_name(0)}; BinarySAE {D} -> {H}, n_bits {N_BITS}, B {B}: {len(tensors)} tensors, "
        f"{nbytes / 1e6:.0f} MB; median (min / max) of {args.reps} calls after {args.warmup}")
    for k, t in zip(keys, tensors):
        say(f"  {k}: {t.numel()} elements, {int((t == 0).sum())} zeros")
    copies = [torch.empty_like(t) for t in tensors]
    gauss = [torch.randn_like(t) for t in tensors]
    zeros = [torch.zeros_like(t) for t in tensors]

    def recipe():
        return [U.wandb_recipe(t) for t in tensors]

    def copy():
        for c, t in zip(copies, tensors):
            c.copy_(t)

    got = alternate({"collect": watch.collect, "kernels": lambda: ops.tensor_stats(tensors, 64), "recipe": recipe, "copy": copy,
                     "gauss": lambda: ops.tensor_stats(gauss, 64), "zeros": lambda: ops.tensor_stats(zeros, 64)},
                    args.reps, args.warmup)
    crate = 2 * nbytes / (got["copy"][0] * 1e-3)
    say(f"ModelWatch.collect()   {fmt(got['collect'])}")
    say(f"kernels only           {fmt(got['kernels'])}  {2 * nbytes / (got['kernels'][0] * 1e-3) / 1e9:7.0f} GB/s read "
        f"= {2 * nbytes / (got['kernels'][0] * 1e-3) / crate:5.1%} of the copy's traffic rate")
    say(f"wandb's recipe (torch) {fmt(got['recipe'])}  x{got['recipe'][0] / got['collect'][0]:.2f} of collect()")
    say(f"device-to-device copy  {fmt(got['copy'])}  {crate / 1e9:7.0f} GB/s read + written")
    spread = (got["gauss"][2] - got["gauss"][1]) / got["gauss"][0]
    say(f"kernels, Gaussian data {fmt(got['gauss'])}  spread {spread:.1%}")
    say(f"kernels, all zeros     {fmt(got['zeros'])}  x{got['zeros'][0] / got['gauss'][0]:.3f} of Gaussian")
    say(f"collect() is {'faster' if got['collect'][0] < got['recipe'][0] else 'NOT faster'} than the recipe; all zeros is "
        f"{'not slower' if got['zeros'][0] <= got['gauss'][0] * (1 + spread) else 'SLOWER'} than Gaussian beyond the spread")
    # the two agree: counts of the recipe on the device against the kernel's (torch's GPU histc rounds the bin index its own
    # way: differences are counted, not asserted)
    mine = watch.collect()
    diff = total = 0
    for k, r in zip(keys, recipe()):
        if r is not None and k in mine:
            diff += sum(abs(int(a) - int(b)) for a, b in zip(r[0], mine[k].counts.tolist())) // 2
            total += sum(int(a) for a in r[0])
    say(f"elements the device recipe bins elsewhere than the kernel (= torch.histc on the CPU): {diff} of {total}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
