#!/usr/bin/env python3
"""Time the decoder-dictionary comparison at full size (32768 x 32768 atoms, D = 512) on one GPU.

Rows: the kernel route (compare_decoders: cross stats-only, self stats-only, cross with the [Na, Nb] matrix stored)
and the reference's torch route on the same card (F.normalize, the fp32 matmul, max(1), max(0), mean).  Atoms are a
BinarySAE 512->32768 (n_bits 4) dictionary against a baseline one, from the synthetic recipes.  Median of `--reps`
timed calls after `--warmup`, CUDA events around each call (host-side result decoding included for the kernel route).

usage: python tools/bench_dictionary.py [--reps 5] [--warmup 2]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import quantizedsae_amd as Q  # noqa: E402
import dictionary_util as U  # noqa: E402
from quantizedsae_amd.inference import compare_decoders, decoder_atoms  # noqa: E402


def timed(fn, reps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = "cuda:0"
    a = decoder_atoms(U.build(Q, {"variant": "binary", "seed": 72}, 512, 32768).to(dev))
    b = decoder_atoms(U.build(Q, {"variant": "baseline", "seed": 71}, 512, 32768).to(dev))
    flop = 2.0 * a.shape[0] * b.shape[0] * a.shape[1]
    print(f"device {torch.cuda.get_device_name(0)}; atoms {tuple(a.shape)} x {tuple(b.shape)}; "
          f"{flop / 1e12:.2f} TFLOP per cross product; median / min / max of {args.reps} ms")

    def torch_route():
        m = F.normalize(a, dim=1) @ F.normalize(b, dim=1).t()
        return m.max(1), m.max(0), m.mean()

    rows = [
        ("cross stats-only (compare_decoders(A, B))", lambda: compare_decoders(a, b), flop),
        ("self stats-only (compare_decoders(B))", lambda: compare_decoders(b), flop / 2),
        ("cross + matrix (return_matrix=True)", lambda: compare_decoders(a, b, return_matrix=True), flop),
        ("torch: normalize, fp32 matmul, max(1), max(0), mean", torch_route, flop),
    ]
    for name, fn, fl in rows:
        med, lo, hi = timed(fn, args.reps, args.warmup)
        print(f"{name:55s} {med:8.2f} ms  ({lo:.2f} / {hi:.2f})  {fl / med / 1e9:6.1f} TFLOP/s", flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
