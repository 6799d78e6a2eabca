#!/usr/bin/env python3
"""k-means over dictionary atoms: qsae_kmeans_assign_f32 (exact-fp32 MFMA, one key per atom, no [N, C] matrix) and
qsae_kmeans_update_f32 (fp64 means in a fixed order) timed in one process at the registry shape N = 32768, D = 512,
C in {16, 256, 4096}, both metrics.

Atoms are Gaussian, drawn on the device; the centers are C distinct atoms (kmeans_atoms' initialisation); the update is
timed on the labels of the assign.  Timed in the same run, on the same card:
  (a) what the library could already do: ops.nearest_atoms_f32(atoms, centers, 1) for the labels (cosine only: that is
      the metric it knows), then index_add_ / bincount and a division for the means;
  (b) the kmeans_pytorch formulation in torch on the device: normalise (cosine) or expand the square (euclidean), fp32
      matmul over 4096-row slices, argmin, and a per-cluster mean loop (one boolean mask and one mean per cluster, as
      kmeans_pytorch's update does).  At C = 4096 that loop is 4096 small launches with a host decision each.
Neither is code under test.  Median / min / max of `--reps` timed calls after `--warmup`, device events around each
call.  "TFLOP/s" counts the useful 2 N C D operations of the assign against the fp32 MFMA peak of 157.3 TFLOP/s.
"iteration" is one assign, the key decode and one update, as kmeans_atoms runs them, without the host read.

usage: python tools/bench_kmeans.py [--reps 5] [--warmup 1]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

DEV = "cuda:0"
N, D = 32768, 512
CLUSTERS = (16, 256, 4096)
PEAK_F32_MFMA = 157.3e12
MARGIN = 1.05                      # run-to-run spread of event timing on a shared machine


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
    return f"{t[0]:9.3f} ({t[1]:.3f} / {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    from quantizedsae_amd import ops
    from quantizedsae_amd.inference.dictionary import _decode_keys

    gen = torch.Generator(device=DEV).manual_seed(1)
    a = torch.randn((N, D), device=DEV, generator=gen)
    perm = torch.randperm(N, device=DEV, generator=gen)

    def ours(c, metric):
        labels = _decode_keys(ops.kmeans_assign(a, c, metric))[1]
        return ops.kmeans_update(a, labels, c)

    def existing(c):                                          # (a)
        labels = _decode_keys(ops.nearest_atoms_f32(a, c, 1))[1][:, 0]
        sums = torch.zeros_like(c).index_add_(0, labels, a)
        counts = torch.bincount(labels, minlength=c.shape[0])
        return torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], c), counts

    def formulation_assign(c, metric, rows=4096):             # (b), the assign
        out = []
        if metric == "cosine":
            an, cn = torch.nn.functional.normalize(a, dim=1), torch.nn.functional.normalize(c, dim=1)
            for r in range(0, N, rows):
                out.append(torch.argmin(1.0 - an[r:r + rows] @ cn.T, dim=1))
        else:
            c2 = (c * c).sum(1)
            for r in range(0, N, rows):
                x = a[r:r + rows]
                out.append(torch.argmin((x * x).sum(1, keepdim=True) - 2.0 * (x @ c.T) + c2[None, :], dim=1))
        return torch.cat(out)

    def formulation(c, metric):                               # (b), the whole iteration
        labels = formulation_assign(c, metric)
        new = c.clone()
        for j in range(c.shape[0]):
            sel = a[labels == j]
            if sel.shape[0]:
                new[j] = sel.mean(dim=0)
        return new

    print(f"device {torch.cuda.get_device_name(0)}; N = {N}, D = {D}, Gaussian atoms; median (min / max) ms; "
          f"{args.reps} calls after {args.warmup}")
    verdict = None
    for C in CLUSTERS:
        c = a[perm[:C]].clone()
        for metric in ("cosine", "euclidean"):
            labels = _decode_keys(ops.kmeans_assign(a, c, metric))[1]
            ta = timed(lambda: ops.kmeans_assign(a, c, metric), args.reps, args.warmup)
            tu = timed(lambda: ops.kmeans_update(a, labels, c), args.reps, args.warmup)
            ti = timed(lambda: ours(c, metric), args.reps, args.warmup)
            tfa = timed(lambda: formulation_assign(c, metric), args.reps, args.warmup)
            tf = timed(lambda: formulation(c, metric), 1 if C > 256 else args.reps, 0 if C > 256 else args.warmup)
            flops = 2.0 * N * C * D / (ta[0] * 1e-3)
            agree = float((formulation_assign(c, metric) == labels).double().mean())
            print(f"C {C:4d} {metric:9s}: assign {fmt(ta)}  {flops / 1e12:6.1f} TFLOP/s = {flops / PEAK_F32_MFMA:5.1%} of "
                  f"the fp32 MFMA peak | update {fmt(tu)} | iteration {fmt(ti)}", flush=True)
            print(f"{'':17s}(b) torch formulation: assign {fmt(tfa)}, iteration {fmt(tf)}"
                  f"{' (one call, no warm-up)' if C > 256 else ''}  x{tf[0] / ti[0]:.2f} of ours; labels agree on {agree:.4%}",
                  flush=True)
            if metric == "cosine":
                te = timed(lambda: existing(c), args.reps, args.warmup)
                same = bool(torch.equal(_decode_keys(ops.nearest_atoms_f32(a, c, 1))[1][:, 0], labels))
                print(f"{'':17s}(a) nearest_atoms_f32(k = 1) + index_add_ / bincount: iteration {fmt(te)}  "
                      f"x{te[0] / ti[0]:.2f} of ours; labels identical: {same}", flush=True)
                if C == 4096:
                    verdict = (ti[0], te[0])
    ti, te = verdict
    ok = ti <= MARGIN * te
    print(f"acceptance (C = 4096, cosine): iteration {ti:.3f} ms against (a) {te:.3f} ms, margin {MARGIN:.2f}: "
          f"{'not slower' if ok else 'SLOWER'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
