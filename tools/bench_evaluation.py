#!/usr/bin/env python3
"""The evaluation reports timed on the device: qsae_quantization_error on logits 32768 x 512 x {4, 8} and
qsae_dataset_moments_add on B = 65536, D = 512 (fp32 and bf16 rows, with and without reconstructions), each next to the
torch formulation of the reference's own function on the same card, in the same process.

  quantization error  ours: ops.quantization_error (two kernels, nothing read back) and quantization_error(model) (the
                      same plus the one 384-byte copy and the Python arithmetic).
                      torch: sigmoid -> [H, D, n] view -> weighted sum for W_float, (sigmoid > 0.5) the same way for
                      W_quant, then the reference's reductions, each with its .item(): mean of squares, mean and max of
                      |diff|, norm; mean / std / min / max / norm of both matrices; the flat argmax.
  dataset moments     ours: one DatasetMoments.add of all rows and finish().
                      torch: per 1024 rows .float(), isnan().any() (a host decision), .sum().item(), (b ** 2).sum().item()
                      (and ((r - b) ** 2).sum().item() with reconstructions).

"GB/s" is the bytes the algorithm must read (the logits; the rows and the reconstructions) over the median time, next to
the 6.29 TB/s a float4 copy reaches on this card and the 8 TB/s of the data sheet.  Median (min / max) of `--reps` calls
after `--warmup`, device events around each call and a synchronise after it.  Nothing here asserts a ratio.

usage: python tools/bench_evaluation.py [--reps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

DEV = "cuda:0"
H, D = 32768, 512
B = 65536
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f} / {t[2]:.3f}) ms"


def rate(nbytes, t):
    r = nbytes / (t[0] * 1e-3)
    return f"{r / 1e9:7.0f} GB/s = {r / HBM_MEASURED:5.1%} of the measured copy rate, {r / HBM_SPEC:5.1%} of the data sheet"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    from quantizedsae_amd import BinarySAE, ops
    from quantizedsae_amd.inference import DatasetMoments, quantization_error

    print(f"device {torch.cuda.get_device_name(0)}; median (min / max) of {args.reps} calls after {args.warmup}")
    gen = torch.Generator(device=DEV).manual_seed(1)

    def torch_quant(w, n, step):
        p = torch.sigmoid(w).view(H, -1, n)
        bw = torch.pow(torch.tensor(2.0, device=DEV), torch.arange(n, device=DEV, dtype=torch.float32))
        bw[-1] *= -1
        wf = step * (p * bw).sum(dim=-1)
        wq = step * ((p > 0.5).to(w.dtype) * bw).sum(dim=-1)
        diff = wq - wf
        out = [diff.pow(2).mean().item(), diff.abs().mean().item(), diff.abs().max().item(), diff.norm().item()]
        for m in (wf, wq):
            out += [m.mean().item(), m.std(unbiased=False).item(), m.min().item(), m.max().item(), m.norm().item()]
        val, idx = (wq - wf).abs().view(-1).max(0)
        return out + [val.item(), int(idx.item())]

    for n in (4, 8):
        model = BinarySAE(D, H, gamma=4.0, n_bits=n).to(DEV).eval()
        with torch.no_grad():
            model.decoder.weight.copy_(torch.randn((H, D * n), device=DEV, generator=gen) * 2.0)
        w = model.decoder.weight.detach()
        step = model.decoder.quantization_step
        nbytes = w.numel() * 4
        tk = timed(lambda: ops.quantization_error(w, D, n, step, math.log(3.0)), args.reps, args.warmup)
        ta = timed(lambda: quantization_error(model), args.reps, args.warmup)
        tt = timed(lambda: torch_quant(w, n, step), max(3, args.reps // 4), 1)
        r, ref = quantization_error(model), torch_quant(w, n, step)
        print(f"quantization error {H} x {D} x {n} ({nbytes / 2 ** 20:.0f} MiB of logits)")
        print(f"  kernels only        {fmt(tk)}  {rate(nbytes, tk)}")
        print(f"  quantization_error  {fmt(ta)}  {rate(nbytes, ta)}")
        print(f"  torch formulation   {fmt(tt)}  x{tt[0] / ta[0]:.2f} of quantization_error")
        print(f"  mse {r['mse']:.9e} / torch {ref[0]:.9e}; max |diff| {r['max_abs']:.9e} at {r['row_index'] * D + r['col_index']} / "
              f"torch {ref[14]:.9e} at {ref[15]}", flush=True)
        del model, w

    def torch_moments(x, recon):
        n, s1, s2, s3 = 0, 0.0, 0.0, 0.0
        for a in range(0, x.shape[0], 1024):
            b = x[a:a + 1024].float()
            if torch.isnan(b).any():
                continue
            s1 += b.sum().item()
            s2 += (b ** 2).sum().item()
            if recon is not None:
                s3 += ((recon[a:a + 1024] - b) ** 2).sum().item()
            n += b.numel()
        return s1 / n, s2 / n - (s1 / n) ** 2, s3 / n

    def ours_moments(x, recon):
        m = DatasetMoments(D, 1024, DEV)
        m.add(x, recon)
        return m.finish()

    x32 = torch.randn((B, D), device=DEV, generator=gen) * 3.0 + 0.25
    recon = x32 * 0.75 + 0.125
    for name, x in (("fp32", x32), ("bf16", x32.to(torch.bfloat16))):
        for with_recon in (False, True):
            r = recon if with_recon else None
            nbytes = x.numel() * x.element_size() + (recon.numel() * 4 if with_recon else 0)
            to = timed(lambda: ours_moments(x, r), args.reps, args.warmup)
            tt = timed(lambda: torch_moments(x, r), max(3, args.reps // 4), 1)
            o, t = ours_moments(x, r), torch_moments(x, r)
            print(f"dataset moments {B} x {D} {name}{' with reconstructions' if with_recon else ''} ({nbytes / 2 ** 20:.0f} MiB)")
            print(f"  DatasetMoments      {fmt(to)}  {rate(nbytes, to)}")
            print(f"  torch formulation   {fmt(tt)}  x{tt[0] / to[0]:.2f} of DatasetMoments")
            print(f"  variance {o['variance']:.12f} / torch {t[1]:.12f}" + (f"; mse {o['mse']:.12f} / torch {t[2]:.12f}" if with_recon else ""),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
