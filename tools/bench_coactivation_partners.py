#!/usr/bin/env python3
"""Co-activation partner sets (one bit per pair) against the int32 co-activation counts, timed in one process on the
same inputs.

Threshold models: at the six shapes of tools/bench_coactivation_bits.py (H = 32768 at B = 65536 and 8192, bit densities
0.6 % and 50 %, and the residual model's four stages with their index map), ``coactivation_partners_bits`` plus
``coactivation_partner_counts`` against ``coactivation_bits`` plus ``coactivation_partner_counts_dense`` on the same packed
bits.  Both update calls share the bit transpose and the int8-MFMA main loop; they differ in the epilogue (one stored
word per 32 pairs, no index lookup, against a read-modify-write of the [H, H] int32 matrix) and in the state the count
reads (128 MiB against 4 GiB).  "equal" compares the two partner counts (OR-accumulation is idempotent, so the number
of calls does not matter).

Top-k models: H = 32768, k = 65, B = 65536, ``coactivation_partners_sparse`` against ``coactivation_sparse``, on the
first batch (zeroed state) and on a fifth batch after four others, for units drawn uniformly and for a skewed draw
(unit = H u^4, u uniform: a few features fire often, as trained SAEs do) -- the second shows whether the load before
the atomic pays once pairs repeat.

Median / min / max of `--reps` timed calls after `--warmup`, device events around each call.  The exit status is 1
when the partners update is slower than ``coactivation_bits`` at a shape by more than the run-to-run spread (the two
calls' max - min), or the counts differ; 0 otherwise.

usage: python tools/bench_coactivation_partners.py [--reps 5] [--warmup 1]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_coactivation_bits import DEV, SHAPES, packed_bits, timed  # noqa: E402


def fmt(t):
    return f"{t[0]:8.2f} ({t[1]:.2f} / {t[2]:.2f})"


def timed_from(fn, prepare, reps, warmup):
    """like timed(), with `prepare` (untimed) before every call"""
    import torch
    ts = []
    for i in range(warmup + reps):
        prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def bits_shapes(args):
    import torch
    from quantizedsae_amd import ops
    ok = True
    for label, H, B, density, stages in SHAPES:
        Hs = H // stages
        ws = Hs // 32 + (1 if stages > 1 else 0)                # words per stage: one word of pad slots per stage
        z = packed_bits(B, stages * ws * 32, density, seed=B + stages)
        index = None
        if stages > 1:
            g = torch.Generator().manual_seed(7)
            local = torch.full((ws * 32,), -1, dtype=torch.int64)
            local[torch.randperm(ws * 32, generator=g)[:Hs]] = torch.randperm(Hs, generator=g)
            local = local.to(DEV)
            index = torch.cat([torch.where(local >= 0, local + s * Hs, local) for s in range(stages)]).to(torch.int32)
        P = z.shape[1] * 32
        partners = torch.zeros((P, P // 32), dtype=torch.int32, device=DEV)
        coact = torch.zeros((H, H), dtype=torch.int32, device=DEV)
        t_part = timed(lambda: ops.coactivation_partners_bits(z, index, partners), args.reps, args.warmup)
        t_cnt = timed(lambda: ops.coactivation_bits(z, H, index, coact), args.reps, args.warmup)
        t_pc = timed(lambda: ops.coactivation_partner_counts(partners, H, index), args.reps, args.warmup)
        t_dc = timed(lambda: ops.coactivation_partner_counts_dense(coact), args.reps, args.warmup)
        a, b = ops.coactivation_partner_counts(partners, H, index), ops.coactivation_partner_counts_dense(coact)
        same = bool(torch.equal(a, b)) and int(a.max()) > 0
        spread = (t_part[2] - t_part[1]) + (t_cnt[2] - t_cnt[1])
        not_slower = t_part[0] <= t_cnt[0] + spread
        ok &= same and not_slower
        print(f"{label:18s} H {H} B {B:5d} density {density:5.3f}: partners_bits {fmt(t_part)} | coactivation_bits {fmt(t_cnt)} "
              f"| ratio {t_part[0] / t_cnt[0]:.3f} {'ok' if not_slower else 'SLOWER'} | partner_counts {fmt(t_pc)} | "
              f"counts_dense {fmt(t_dc)} | update + count {t_part[0] + t_pc[0]:.2f} vs {t_cnt[0] + t_dc[0]:.2f} "
              f"x{(t_cnt[0] + t_dc[0]) / (t_part[0] + t_pc[0]):.2f} | equal {same} | mean partners {float(a.float().mean()):.1f}",
              flush=True)
        del z, partners, coact
        torch.cuda.empty_cache()
    return ok


def sparse_shape(args):
    import torch
    from quantizedsae_amd import ops
    H, k, B = 32768, 65, 65536
    ok = True
    for draw in ("uniform", "skewed"):
        g = torch.Generator(device=DEV)
        g.manual_seed(11)
        batches = []
        for _ in range(5):
            u = torch.rand((B, k), device=DEV, generator=g)
            u = u ** 4 if draw == "skewed" else u
            batches.append((u * H).to(torch.int32).clamp_(max=H - 1))
        partners = torch.zeros((H, H // 32), dtype=torch.int32, device=DEV)
        coact = torch.zeros((H, H), dtype=torch.int32, device=DEV)
        first_p = timed_from(lambda: ops.coactivation_partners_sparse(batches[0], None, H, partners), partners.zero_,
                             args.reps, args.warmup)
        first_c = timed_from(lambda: ops.coactivation_sparse(batches[0], None, H, coact), coact.zero_, args.reps, args.warmup)
        for idx in batches[1:4]:
            ops.coactivation_partners_sparse(idx, None, H, partners)
            ops.coactivation_sparse(idx, None, H, coact)
        fifth_p = timed(lambda: ops.coactivation_partners_sparse(batches[4], None, H, partners), args.reps, args.warmup)
        fifth_c = timed(lambda: ops.coactivation_sparse(batches[4], None, H, coact), args.reps, args.warmup)
        a, b = ops.coactivation_partner_counts(partners, H), ops.coactivation_partner_counts_dense(coact)
        same = bool(torch.equal(a, b)) and int(a.max()) > 0
        ok &= same
        print(f"top-k {draw:7s} H {H} k {k} B {B}: first batch partners_sparse {fmt(first_p)} | coactivation_sparse {fmt(first_c)} "
              f"| ratio {first_p[0] / first_c[0]:.3f} || fifth batch partners_sparse {fmt(fifth_p)} | coactivation_sparse "
              f"{fmt(fifth_c)} | ratio {fifth_p[0] / fifth_c[0]:.3f} | equal {same} | mean partners {float(a.float().mean()):.1f}",
              flush=True)
        del partners, coact, batches
        torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    print(f"device {torch.cuda.get_device_name(0)}; median (min / max) ms of {args.reps} calls after {args.warmup}")
    ok = bits_shapes(args)
    ok &= sparse_shape(args)
    print(f"partners update not slower than coactivation_bits at every shape, equal partner counts everywhere: {ok}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
