#!/usr/bin/env python3
"""Token-overlap histogram between two SAEs: qsae_token_overlap_hist (int8 MFMA over packed bitsets, LDS histogram)
and the whole `jaccard_histogram`, timed in one process at the registry shape Na = Nb = 32768, k = 100.

Nothing computed this before, and the reference's Python double loop cannot run at this size, so the yardstick is the
straightforward device formulation on the same sets: 0/1 membership matrices in fp16 (exact: sums of at most 128 ones,
fp32 accumulation), `torch` matmul on slices of 2048 rows, `bincount` of (inter, union).  It is a yardstick, not code
under test; "equal" compares the two tables.

Data, drawn on the device:
  zipf      400 tokens per feature, id = floor(V u^3): the top-100 sets are mostly full and share the frequent tokens
            (3 % of the features never fire); also run through the vocabulary compaction of jaccard_histogram
  uniform   100 distinct uniform tokens per feature: every set full, almost every pair in the bins (0, 200), (1, 199):
            the most same-address LDS atomics the epilogue can meet
  spread    uniform tokens, set sizes uniform in 1..100: the pairs spread over ~10^4 bins, the fewest collisions
Median / min / max of `--reps` timed calls after `--warmup`, device events around each call.  "POP/s executed" counts
what the kernel runs, 2 * (256-feature tiles)^2 * (256-token chunks), against the 5.03 POP/s int8 peak DESIGN.md 4.14
uses.  The fixed part of a call (re-tiling aside, the epilogue) comes from timing V and V / 2 on the same sizes and
solving t = per_chunk * chunks + fixed.

A rocprofv3 --kernel-trace --stats pass over a child process (the kernel call only, no counters) gives the split
between the re-tiling pass and the MFMA kernel; its summary is printed last.

usage: python tools/bench_token_overlap.py [--reps 5] [--warmup 1] [--baseline-reps 2] [--out DIR] [--no-trace]
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
N, V, K = 32768, 50304, 100
PEAK_INT8 = 5.03e15


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


def zipf_stats(seed, draws=400):
    """stats dict with an on-device CSR pair: `draws` tokens per feature, Zipf-like ids, 3 % never-active features"""
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    tokens = (V * torch.rand(N * draws, device=DEV, generator=g) ** 3).long().clamp_(max=V - 1)
    offsets = torch.arange(N + 1, device=DEV, dtype=torch.int64) * draws
    counts = torch.full((N,), draws, device=DEV, dtype=torch.int64)
    counts[torch.rand(N, device=DEV, generator=g) < 0.03] = 0
    return {"tokens_per_feature": (offsets, tokens), "activation_counts": counts}


def uniform_sets(seed, spread):
    """padded sets [N, K] of distinct uniform tokens; `spread`: sizes uniform in 1..K, else all K"""
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    sets = torch.empty((N, K), dtype=torch.int64, device=DEV)
    for r in range(0, N, 4096):
        sets[r:r + 4096] = torch.rand((4096, V), device=DEV, generator=g).topk(K, dim=1).indices
    if spread:
        size = torch.randint(1, K + 1, (N,), device=DEV, generator=g)
        sets[torch.arange(K, device=DEV)[None, :] >= size[:, None]] = -1
    return sets


def packed(sets, v):
    """(bitsets over the tokens below v, true set sizes): tokens at or past v are dropped from the bits only"""
    import torch
    from quantizedsae_amd.inference.token_overlap import _pack
    return _pack(torch.where(sets < v, sets, torch.full_like(sets, -1)), (v + 31) // 32), (sets >= 0).sum(1).int()


def baseline(pa, asize, pb, bsize, v, rows=2048):
    """membership matrices in fp16, matmul on row slices, bincount of (inter, union)"""
    import torch
    shifts = torch.arange(32, device=DEV, dtype=torch.int32)

    def member(p):
        return ((p[:, :(v + 31) // 32, None] >> shifts) & 1).view(p.shape[0], -1)[:, :v].half()

    Mb = member(pb)
    sb = bsize.long()[None, :]
    hist = torch.zeros((K + 1) * (2 * K + 1), dtype=torch.int64, device=DEV)
    for r in range(0, pa.shape[0], rows):
        inter = (member(pa[r:r + rows]) @ Mb.T).long()
        sa = asize[r:r + rows].long()[:, None]
        ok = (sa > 0) & (sb > 0)
        hist += torch.bincount((inter * (2 * K + 1) + sa + sb - inter)[ok], minlength=hist.numel())
    return hist.view(K + 1, 2 * K + 1)


def child():
    """what the trace pass runs: the kernel call alone, three times on the zipf sets at the full vocabulary"""
    import torch
    from quantizedsae_amd import ops
    from quantizedsae_amd.inference import top_token_sets
    sides = []
    for seed in (1, 2):
        s = zipf_stats(seed)
        sides.append(packed(top_token_sets(s["tokens_per_feature"], s["activation_counts"], K).tokens, V))
    for _ in range(3):
        ops.token_overlap_hist(*sides[0], *sides[1], V, K)
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
    print(f"kernel trace (rocprofv3 --kernel-trace --stats; zipf sets, Na = Nb = {N}, V = {V}, k = {K}, 3 calls):")
    for f in sorted(out.rglob("*kernel_stats.csv")):
        for row in csv.DictReader(f.open()):
            if "token_overlap" in row["Name"]:
                name = row["Name"].split("(")[0]
                print(f"  {name:45s} calls {row['Calls']:>3s}  avg {float(row['AverageNs']) / 1e6:9.3f} ms  "
                      f"min {float(row['MinNs']) / 1e6:9.3f}  max {float(row['MaxNs']) / 1e6:9.3f}  {float(row['Percentage']):5.1f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--out", type=Path, default=None, help="directory of the rocprofv3 output (default: a temporary one)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()

    import torch
    from quantizedsae_amd import ops
    from quantizedsae_amd.inference import jaccard_histogram, top_token_sets

    print(f"device {torch.cuda.get_device_name(0)}; Na = Nb = {N}, k = {K}; median (min / max) ms; kernel: {args.reps} calls "
          f"after {args.warmup}, baseline: {args.baseline_reps} after 1")
    stats = [zipf_stats(1), zipf_stats(2)]
    zipf = [top_token_sets(s["tokens_per_feature"], s["activation_counts"], K).tokens for s in stats]
    data = {"zipf": zipf, "uniform": [uniform_sets(3, False), uniform_sets(4, False)],
            "spread": [uniform_sets(5, True), uniform_sets(6, True)]}
    all_equal = True

    def run(label, sets, v, with_baseline):
        nonlocal all_equal
        (pa, asize), (pb, bsize) = (packed(s, v) for s in sets)
        hist = torch.zeros((K + 1, 2 * K + 1), dtype=torch.int64, device=DEV)
        t = timed(lambda: ops.token_overlap_hist(pa, asize, pb, bsize, v, K, hist), args.reps, args.warmup)
        chunks = (v + 255) // 256
        pops = 2.0 * N * N * chunks * 256 / (t[0] * 1e-3)
        line = (f"{label:30s} V {v:6d}: kernel call {t[0]:8.2f} ({t[1]:.2f} / {t[2]:.2f})  {pops / 1e12:7.1f} TOP/s executed, "
                f"{100 * pops / PEAK_INT8:4.1f} % of the int8 peak; nonzero bins {int((hist > 0).sum())}, largest share "
                f"{float(hist.max()) / float(hist.sum()):.3f}")
        if with_baseline:
            tb = timed(lambda: baseline(pa, asize, pb, bsize, v), args.baseline_reps, 1)
            same = bool(torch.equal(baseline(pa, asize, pb, bsize, v) * (args.reps + args.warmup), hist))
            all_equal &= same
            line += f" | baseline {tb[0]:9.2f} ({tb[1]:.2f} / {tb[2]:.2f})  x{tb[0] / t[0]:.1f} | equal {same}"
        print(line, flush=True)
        torch.cuda.empty_cache()
        return t[0], chunks

    for label, sets in data.items():
        full, chunks = run(label, sets, V, True)
        half, hchunks = run(label + " (first half of V)", sets, V // 2, False)
        per_chunk = (full - half) / (chunks - hchunks)
        fixed = full - per_chunk * chunks
        print(f"{'':30s} per chunk {per_chunk * 1e3:.1f} us, fixed part {fixed:.2f} ms = {100 * fixed / full:.1f} % of the call "
              f"at V = {V}", flush=True)

    # the vocabulary compaction of jaccard_histogram, and the whole of it from on-device CSR input
    present = [torch.unique(t[t >= 0]) for t in zipf]
    both, seen = torch.unique(torch.cat(present), return_counts=True)
    common = both[seen == 2]
    remap = torch.full((V,), -1, dtype=torch.int64, device=DEV)
    remap[common] = torch.arange(common.numel(), device=DEV)
    compacted = [torch.where(t >= 0, remap[t.clamp(min=0)], t) for t in zipf]
    sizes = [(t >= 0).sum(1).int() for t in zipf]
    vc = int(common.numel())
    (pa, _), (pb, _) = (packed(s, vc) for s in compacted)
    hist = torch.zeros((K + 1, 2 * K + 1), dtype=torch.int64, device=DEV)
    t = timed(lambda: ops.token_overlap_hist(pa, sizes[0], pb, sizes[1], vc, K, hist), args.reps, args.warmup)
    print(f"{'zipf, compacted vocabulary':30s} V {vc:6d}: kernel call {t[0]:8.2f} ({t[1]:.2f} / {t[2]:.2f})", flush=True)
    t = timed(lambda: jaccard_histogram(stats[0], stats[1], K), args.reps, args.warmup)
    print(f"{'jaccard_histogram, CSR input':30s} {N * 400} tokens per side: {t[0]:8.2f} ({t[1]:.2f} / {t[2]:.2f}) "
          f"(sets, compaction, packing, kernel, copy of the table to the host)", flush=True)
    s = jaccard_histogram(stats[0], stats[1], K).summary()
    print(f"  n_pairs {s['n_pairs']}  mean {s['mean']:.6f}  top means {s['top']}")
    print(f"equal results wherever the baseline ran: {all_equal}")
    if not args.no_trace:
        if args.out is not None:
            trace(args.out)
        else:
            with tempfile.TemporaryDirectory() as d:
                trace(Path(d))
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
