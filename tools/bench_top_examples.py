#!/usr/bin/env python3
"""Strongest activations per feature: the streaming top-n update (qsae_top_examples_*) against the same update written in
torch on the same card, and next to the forward that produces its input.

Per batch of ``--rows`` x 65 at H = 32768 (bench.py's BinarySAE with k = 65, standard-normal inputs), n in {8, 64}:
  (a) ``TopExamples.add_compact``: on the first batch (empty state) and in steady state (the 10th batch of the stream, the
      state holding the first nine);
  (b) the same update in torch: keep val > 0, one sort of the composite key feature << 48 | value bits << 16 | ~row, the
      first n of every feature's segment, and a row-wise sort that joins them with the old state -- results are compared
      for equality with (a);
  (c) ``forward_compact`` of the model for that batch, of which (a) is reported as a share.
Dense form: ``add_dense`` of a ReLU latent [8192, 32768] against ``torch.topk(latent.T, n)`` (which keeps no state).
Device events around each call, median (min / max) of ``--reps`` after one warm-up; whatever a call mutates is cloned
outside the timed region.

usage: python tools/bench_top_examples.py [--reps 5] [--rows 65536] [--batches 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
DEV = "cuda:0"
D, H, K = 512, 32768, 65
SIGN = -(2 ** 63)


def timed(fn, reps, setup=None):
    """(median, min, max) ms of fn(setup()) by device events; one untimed warm-up call first"""
    import torch
    times = []
    out = None
    for i in range(reps + 1):
        arg = setup() if setup is not None else None
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        out = fn(arg)
        e.record()
        torch.cuda.synchronize()
        if i:
            times.append(s.elapsed_time(e))
    return (statistics.median(times), min(times), max(times)), out


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f} / {t[2]:.3f}) ms"


def torch_update(idx, val, base, state, n):
    """The update in torch.  ``state`` int64 [H, n] holds the u64 keys with the top bit flipped (so that int64 order is the
    keys' order and 'none' is the smallest value); returns the new state."""
    import torch
    B, k = idx.shape
    on = val > 0
    rows = torch.arange(B, device=idx.device).unsqueeze(1).expand(B, k)[on]
    feat = idx[on].long()
    bits = val[on].view(torch.int32).long() & 0xFFFFFFFF
    mono = bits | 0x80000000                                    # val > 0: the order-preserving map sets the top bit
    comp = (feat << 48) | ((mono & 0x7FFFFFFF) << 16) | (0xFFFF - rows)     # needs B <= 65536; bit 31 of mono is constant
    order = torch.sort(comp, descending=True).indices
    feat, mono, rows = feat[order], mono[order], rows[order]
    first = torch.ones_like(feat, dtype=torch.bool)
    first[1:] = feat[1:] != feat[:-1]
    pos = torch.arange(feat.numel(), device=feat.device)
    start = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values
    rank = pos - start
    keep = rank < n
    key = ((mono[keep] << 32) | (0xFFFFFFFF - (rows[keep] + base))) ^ SIGN
    both = torch.full((state.shape[0], 2 * n), SIGN, dtype=torch.int64, device=state.device)
    both[:, :n] = state
    both[feat[keep], n + rank[keep]] = key
    return torch.sort(both, dim=1, descending=True).values[:, :n].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--dense-rows", type=int, default=8192)
    ap.add_argument("--out", type=Path, default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import bench
    from quantizedsae_amd.inference import TopExamples
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    B = args.rows
    assert B <= 65536, "the torch form packs the row into 16 bits"
    emit(f"device {torch.cuda.get_device_name(0)}; device events, median (min / max) of {args.reps} calls after one warm-up; "
         f"H {H}, D {D}, k {K}, {B} rows per batch")
    model = bench.build_model(DEV)
    model.k = K / H
    g = torch.Generator(device=DEV).manual_seed(11)
    stream = []
    with torch.no_grad():
        for _ in range(args.batches):
            x = torch.randn((B, D), device=DEV, generator=g)
            idx, val, _ = model.forward_compact(x)
            stream.append((idx, val))
        t_fwd, _ = timed(lambda _a: model.forward_compact(x), args.reps)
    emit(f"(c) forward_compact of one batch:                 {fmt(t_fwd)}")
    last = args.batches - 1
    for n in (8, 64):
        def fresh():
            return TopExamples(H, n, DEV)

        def update(b, te):
            te.add_compact(stream[b][0], stream[b][1], b * B)
            return te
        t_first, _ = timed(lambda te: update(0, te), args.reps, fresh)
        te = fresh()
        for b in range(last):
            update(b, te)
        steady = te.keys.clone()

        def warm():
            w = fresh()
            w.keys.copy_(steady)
            return w
        t_steady, te_end = timed(lambda w: update(last, w), args.reps, warm)
        emit(f"n = {n}")
        emit(f"  (a) add_compact, first batch:                   {fmt(t_first)}")
        emit(f"  (a) add_compact, batch {last + 1} of the stream:          {fmt(t_steady)}  "
             f"= {100 * t_steady[0] / t_fwd[0]:.1f} % of (c)")
        empty = torch.full((H, n), SIGN, dtype=torch.int64, device=DEV)
        tt_first, _ = timed(lambda st: torch_update(*stream[0], 0, st, n), args.reps, lambda: empty)
        st = empty
        for b in range(last):
            st = torch_update(*stream[b], b * B, st, n)
        tt_steady, st_end = timed(lambda s9: torch_update(*stream[last], last * B, s9, n), args.reps, lambda: st)
        same = bool(torch.equal(st_end ^ SIGN, te_end.keys))
        emit(f"  (b) torch (sort + first n per segment), first:  {fmt(tt_first)}")
        emit(f"  (b) torch, batch {last + 1} of the stream:                {fmt(tt_steady)}  equal keys: {same}")
        emit(f"  steady state (a) / (b) = {t_steady[0] / tt_steady[0]:.3f}  (aim: not above 1.05)")
        del st, st_end, empty
        torch.cuda.empty_cache()
    stream.clear()
    torch.cuda.empty_cache()
    Bd = args.dense_rows
    lat = torch.relu(torch.randn((Bd, H), device=DEV, generator=g))
    emit(f"dense form, latent [{Bd}, {H}] ({lat.numel() * 4 / 1e9:.2f} GB read once)")
    for n in (8, 64):
        t_dense, te = timed(lambda w: (w.add_dense(lat, 0), w)[1], args.reps, lambda: TopExamples(H, n, DEV))
        t_topk, tk = timed(lambda _a: torch.topk(lat.T, n), args.reps)
        vals = te.finish()["values"]
        emit(f"  n = {n}: add_dense {fmt(t_dense)} = {lat.numel() * 4 / t_dense[0] / 1e6:.0f} GB/s;  torch.topk(latent.T, n) "
             f"{fmt(t_topk)};  equal values: {bool(torch.equal(vals, tk.values))}")
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
