#!/usr/bin/env python3
"""Nearest atoms of an int8 dictionary: qsae_nearest_atoms_i8 (int8 MFMA, per-row top-k lists in LDS, no [N, N] matrix)
timed in one process at the registry shape N = 32768, D = 512, self mode with duplicates, k in {10, 64}.

Dictionaries, drawn on the device:
  ternary    {-1, 0, +1} at the density of a kaiming-initialised STEWeights: w ~ N(0, 2 / H) per the reference's init is
             all zeros at threshold 0.5, so the density of the trained dictionaries the project's fixtures use is taken
             instead: P(|w| >= 0.5) for w ~ N(0, 0.5^2) = 31.7 %
  4-bit      uniform two's-complement values in [-8, 7]
  identical  one atom repeated: every product passes the filter in every round and every pair is a duplicate hit --
             the worst case of the epilogue
Yardstick on the same card: the reference's formulation (inspector.py:47-58) without the host -- F.normalize, fp32
matmul over 2048-row slices, torch.topk(k) -- which is not code under test; "agree" compares the neighbour sets on the
rows whose k-th and (k+1)-th yardstick cosines are more than 2e-6 apart.
Median / min / max of `--reps` timed calls after `--warmup`, device events around each call.  "TOP/s" counts the useful
int8 operations 2 N^2 D against the 5.03 POP/s peak DESIGN.md 4.14 quotes; "ns per product" is the whole call over N^2.

A rocprofv3 --kernel-trace --stats pass over a child process (the kernel call only, no counters) gives the split
between the norm pass, the main kernel and the merge; its summary is printed last.

usage: python tools/bench_dictionary_neighbors.py [--reps 5] [--warmup 1] [--out DIR] [--no-trace] [--skip-identical]
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
PEAK_INT8 = 5.03e15
TERNARY_DENSITY = 0.317


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


def dictionaries(which=("ternary", "4-bit", "identical")):
    import torch
    g = torch.Generator(device=DEV).manual_seed(1)
    out = {}
    if "ternary" in which:
        u = torch.rand((N, D), device=DEV, generator=g)
        out["ternary"] = torch.where(u < TERNARY_DENSITY / 2, -1, torch.where(u < TERNARY_DENSITY, 1, 0)).to(torch.int8)
    if "4-bit" in which:
        out["4-bit"] = torch.randint(-8, 8, (N, D), device=DEV, generator=g, dtype=torch.int8)
    if "identical" in which:
        u = torch.rand((1, D), device=DEV, generator=g)
        out["identical"] = torch.where(u < 0.16, -1, torch.where(u < 0.32, 1, 0)).to(torch.int8).repeat(N, 1)
    return out


def baseline(a, k, rows=2048):
    """F.normalize rows, fp32 matmul on row slices, topk"""
    import torch
    f = torch.nn.functional.normalize(a.float(), dim=1)
    vals, idx = [], []
    for r in range(0, a.shape[0], rows):
        v, i = torch.topk(f[r:r + rows] @ f.T, k + 1, dim=1)
        vals.append(v)
        idx.append(i)
    return torch.cat(vals), torch.cat(idx)


def child():
    """what the trace pass runs: the kernel call alone, three times per k on the ternary dictionary"""
    import torch
    from quantizedsae_amd import ops
    a = dictionaries(("ternary",))["ternary"]
    for k in (10, 64):
        for _ in range(3):
            ops.nearest_atoms_i8(a, None, k, want_duplicates=True)
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
    print(f"kernel trace (rocprofv3 --kernel-trace --stats; ternary, N = {N}, D = {D}, 3 calls each at k = 10 and k = 64):")
    for f in sorted(out.rglob("*kernel_stats.csv")):
        for row in csv.DictReader(f.open()):
            if any(s in row["Name"] for s in ("nearest_atoms", "nbr_norm", "topk_lists_merge")):
                name = row["Name"].split("(")[0]
                print(f"  {name:50s} calls {row['Calls']:>3s}  avg {float(row['AverageNs']) / 1e6:9.3f} ms  "
                      f"min {float(row['MinNs']) / 1e6:9.3f}  max {float(row['MaxNs']) / 1e6:9.3f}  {float(row['Percentage']):5.1f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=Path, default=None, help="directory of the rocprofv3 output (default: a temporary one)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--skip-identical", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()

    import torch
    from quantizedsae_amd import ops
    from quantizedsae_amd.inference.dictionary import _decode_keys

    print(f"device {torch.cuda.get_device_name(0)}; N = {N}, D = {D}, self mode with duplicate_of; median (min / max) ms; "
          f"{args.reps} calls after {args.warmup}")
    which = ("ternary", "4-bit") + (() if args.skip_identical else ("identical",))
    ok = True
    for label, a in dictionaries(which).items():
        for k in (10, 64):
            reps, warm = (args.reps, args.warmup) if label != "identical" else (1, 0)
            t = timed(lambda: ops.nearest_atoms_i8(a, None, k, want_duplicates=True), reps, warm)
            tops = 2.0 * N * N * D / (t[0] * 1e-3)
            line = (f"{label:10s} k {k:2d}: call {t[0]:9.2f} ({t[1]:.2f} / {t[2]:.2f})  {tops / 1e12:7.1f} TOP/s = "
                    f"{100 * tops / PEAK_INT8:5.2f} % of the int8 peak, {t[0] * 1e6 / (N * N):.4f} ns per product")
            if label != "identical":
                tb = timed(lambda: baseline(a, k), 2, 1)
                vals, bidx = baseline(a, k)
                keys, _ = ops.nearest_atoms_i8(a, None, k)
                _, idx = _decode_keys(keys)
                clear = (vals[:, k - 1] - vals[:, k]) > 2e-6
                same = (torch.sort(idx, 1).values == torch.sort(bidx[:, :k], 1).values).all(1)
                agree = bool(same[clear].all())
                ok &= agree
                line += (f" | yardstick {tb[0]:8.2f} ({tb[1]:.2f} / {tb[2]:.2f})  x{tb[0] / t[0]:.2f} | agree on "
                         f"{int(clear.sum())} clear rows: {agree}")
            print(line, flush=True)
        del a
        torch.cuda.empty_cache()
    print(f"neighbour sets agree wherever the yardstick is clear: {ok}")
    if not args.no_trace:
        if args.out is not None:
            trace(args.out)
        else:
            with tempfile.TemporaryDirectory() as d:
                trace(Path(d))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
