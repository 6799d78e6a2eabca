#!/usr/bin/env python3
"""Nearest atoms of an fp32 dictionary: qsae_nearest_atoms_f32 (exact-fp32 MFMA, per-query top-k lists in LDS, no [N, N]
matrix) timed in one process at the registry shape N = 32768, D = 512, self mode, k in {10, 64}.

Dictionaries, drawn on the device:
  baseline    U(+-1 / sqrt(N)) per component: a baseline SAE's decoder.weight at its initialisation
  matryoshka  weight + weight_mirror of a matryoshka decoder: two U(+-1) logit tables pushed away from 0 by 1e-3
Timed in the same run:
  (a) the reference's formulation on the same card (analyze_sae.py:59-69 and a top-k) -- F.normalize, fp32 matmul over
      2048-row slices, torch.topk(k) -- which is not code under test; "agree" compares the neighbour sets on the rows
      whose yardstick cosines around the k-th place are more than 2e-5 apart;
  (b) cosine_compare in cross mode, stats only: the same contraction with a one-key epilogue, the floor for the loop.
Median / min / max of `--reps` timed calls after `--warmup`, device events around each call.  "TFLOP/s" counts the
useful 2 N^2 D operations; "ns per product" is the whole call over N^2.

A rocprofv3 --kernel-trace --stats pass over a child process (the kernel call only, no counters) gives the split
between the norm pass, the main kernel and the merge; its summary is printed last.

usage: python tools/bench_dictionary_neighbors_f32.py [--reps 5] [--warmup 1] [--out DIR] [--no-trace]
"""
from __future__ import annotations

import argparse
import csv
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

DEV = "cuda:0"
N, D = 32768, 512


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


def dictionaries(which=("baseline", "matryoshka")):
    import torch
    g = torch.Generator(device=DEV).manual_seed(1)
    out = {}

    def u(lo, hi):
        return lo + (hi - lo) * torch.rand((N, D), device=DEV, generator=g)

    def away(t, m=1e-3):
        return torch.where(t.abs() < m, torch.where(t < 0, -m, m), t)
    if "baseline" in which:
        b = 1.0 / N ** 0.5
        out["baseline"] = u(-b, b)
    if "matryoshka" in which:
        out["matryoshka"] = away(u(-1.0, 1.0)) + away(u(-1.0, 1.0))
    return out


def yardstick(a, k, rows=2048):
    """F.normalize rows, fp32 matmul on row slices, topk"""
    import torch
    f = torch.nn.functional.normalize(a, dim=1)
    vals, idx = [], []
    for r in range(0, a.shape[0], rows):
        v, i = torch.topk(f[r:r + rows] @ f.T, k + 1, dim=1)
        vals.append(v)
        idx.append(i)
    return torch.cat(vals), torch.cat(idx)


def child():
    """what the trace pass runs: the kernel call alone, three times per k on the baseline dictionary"""
    import torch
    from quantizedsae_amd import ops
    a = dictionaries(("baseline",))["baseline"]
    for k in (10, 64):
        for _ in range(3):
            ops.nearest_atoms_f32(a, None, k)
    torch.cuda.synchronize()


def trace(out: Path):
    exe = shutil.which("rocprofv3")
    if exe is None:
        print("rocprofv3 not found: no kernel trace")
        return
    out.mkdir(parents=True, exist_ok=True)
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--", sys.executable,
           str(Path(__file__).resolve()), "--child"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(f"rocprofv3 pass failed ({r.returncode}):\n{r.stderr[-2000:]}")
        return
    print(f"kernel trace (rocprofv3 --kernel-trace --stats; baseline, N = {N}, D = {D}, 3 calls each at k = 10 and k = 64):")
    for f in sorted(out.rglob("*kernel_stats.csv")):
        for row in csv.DictReader(f.open()):
            if any(s in row["Name"] for s in ("EpiNeighbors", "atom_inv_norms", "topk_lists_merge")):
                name = "gemm_nt_f32_kernel<.., EpiNeighbors, ..>" if "EpiNeighbors" in row["Name"] else row["Name"].split("(")[0]
                print(f"  {name:50s} calls {row['Calls']:>3s}  avg {float(row['AverageNs']) / 1e6:9.3f} ms  "
                      f"min {float(row['MinNs']) / 1e6:9.3f}  max {float(row['MaxNs']) / 1e6:9.3f}  {float(row['Percentage']):5.1f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=Path, default=None, help="directory of the rocprofv3 output (default: a temporary one)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()

    import torch
    from quantizedsae_amd import ops
    from quantizedsae_amd.inference.dictionary import _decode_keys

    print(f"device {torch.cuda.get_device_name(0)}; N = {N}, D = {D}, self mode; median (min / max) ms; "
          f"{args.reps} calls after {args.warmup}")
    ok = True
    for label, a in dictionaries().items():
        tc = timed(lambda: ops.cosine_compare(a, a.clone()), args.reps, args.warmup)
        print(f"{label:10s} (b) cosine_compare cross, stats only: {tc[0]:9.2f} ({tc[1]:.2f} / {tc[2]:.2f})", flush=True)
        for k in (10, 64):
            t = timed(lambda: ops.nearest_atoms_f32(a, None, k), args.reps, args.warmup)
            flops = 2.0 * N * N * D / (t[0] * 1e-3)
            ty = timed(lambda: yardstick(a, k), args.reps, args.warmup)
            vals, yidx = yardstick(a, k)
            _, idx = _decode_keys(ops.nearest_atoms_f32(a, None, k))
            clear = ((vals[:, :-1] - vals[:, 1:]) > 2e-5).all(1)
            agree = bool((idx[clear] == yidx[clear][:, :k]).all())
            ok &= agree
            print(f"{label:10s} k {k:2d}: call {t[0]:9.2f} ({t[1]:.2f} / {t[2]:.2f})  {flops / 1e12:6.1f} TFLOP/s, "
                  f"{t[0] * 1e6 / (N * N):.4f} ns per product, x{t[0] / tc[0]:.2f} of (b) | (a) yardstick {ty[0]:8.2f} "
                  f"({ty[1]:.2f} / {ty[2]:.2f})  x{ty[0] / t[0]:.2f} | agree on {int(clear.sum())} clear rows: {agree}",
                  flush=True)
            del vals, yidx
        del a
        torch.cuda.empty_cache()
    print(f"neighbours agree wherever the yardstick is clear: {ok}")
    if not args.no_trace:
        if args.out is not None:
            trace(args.out)
        else:
            with tempfile.TemporaryDirectory() as d:
                trace(Path(d))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
