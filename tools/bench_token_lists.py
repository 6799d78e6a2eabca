#!/usr/bin/env python3
"""Tokens per feature of one batch: ``compute_activation_stats(with_tokens="csr")`` (ordered CSR lists built on the
device, qsae_token_lists_*) against ``with_tokens=True`` (the reference's Python lists: nonzero, stable sort, host copy,
H list extensions), timed in one process on the same model and the same batch, plus the token-list calls on their own.

One batch of 32768 rows at H = 32768, D = 512, standard-normal inputs (bench.py's batch):
  b_sae   BinarySAE(512, 32768, gamma 4, n_bits 4) with k = 65, bench.py's synthetic weights
  q_sae   QuantizedMatryoshkaSAE(512, 32768, top_k 32, abs_range 4, n_bits 4) with the encoder bias at -0.44 (-2.5 sigma
          of the latent, about 200 active units per row): bench.py's config 4

Both modes also compute the counts and the co-activation matrix, so ``with_tokens=False`` is timed too and the
difference to it is what the tokens per feature cost in either form.  "alone" times add_compact / add_bits + finish() on
the model's (idx, val) or packed bits: the count, the host read of the entry count and the fill.  The two forms are
compared for equality (token_lists_to_python of the CSR pair == the Python lists).  Median / min / max of ``--reps``
timed calls after ``--warmup``, a host clock around work that ends in a device synchronise (the list mode is host work
for the most part).  Calls are alternated between the modes.

``--parent DIR``: a checkout of the parent commit, already built; its ``with_tokens=True`` and ``False`` are timed in a
child process of this run on the same inputs (same seeds), after this tree's.

usage: python tools/bench_token_lists.py [--reps 3] [--warmup 1] [--rows 32768] [--parent DIR] [--out FILE]
"""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

DEV = "cuda:0"
D, H, K = 512, 32768, 65
TPC = 128


def models(root: Path):
    sys.path.insert(0, str(root))
    import torch
    import bench
    from quantizedsae_amd import QuantizedMatryoshkaSAE
    from quantizedsae_amd.inference import framework as F
    b = bench.build_model(DEV)
    b.k = K / H
    with torch.no_grad():
        q = QuantizedMatryoshkaSAE(D, H, top_k=32, abs_range=4, n_bits=4)
        q.encoder[0].bias.fill_(-0.44)
        g = torch.Generator().manual_seed(4)
        q.decoder.weight.copy_(torch.rand(q.decoder.weight.shape, generator=g) * 2 - 1)
        q.decoder.weight_mirror.copy_(torch.rand(q.decoder.weight_mirror.shape, generator=g) * 2 - 1)
    q = q.to(DEV).eval()
    return {"b_sae": F.SAEWrapper(F.SAE_REGISTRY["b_sae"], b, DEV), "q_sae": F.SAEWrapper(F.SAE_REGISTRY["q_sae"], q, DEV)}


def inputs(rows: int):
    import torch
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((rows, D), device=DEV, generator=g)
    contexts = (rows + TPC - 1) // TPC
    token_ids = torch.randint(0, 50257, (contexts, TPC), generator=torch.Generator().manual_seed(12))
    return x, token_ids


def clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(fns, reps, warmup):
    """{name: (median, min, max) ms} and the last result of each; the calls of one round run one after the other"""
    times = {name: [] for name in fns}
    last = {}
    for i in range(warmup + reps):
        for name, fn in fns.items():
            ms, last[name] = clock(fn)
            if i >= warmup:
                times[name].append(ms)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}, last


def fmt(t):
    return f"{t[0]:10.2f} ({t[1]:.2f} / {t[2]:.2f})"


def run(root: Path, rows: int, reps: int, warmup: int, modes, emit):
    import torch
    saes = models(root)
    from quantizedsae_amd.inference import analysis as A
    x, token_ids = inputs(rows)
    for name, sae in saes.items():
        def stats(mode):
            st = A.compute_activation_stats(sae, [x], token_ids=token_ids, tokens_per_context=TPC, with_tokens=mode)
            del st["coactivation"]                           # 4 GiB on the host per result: not kept
            return st
        fns = {repr(mode): (lambda mode=mode: stats(mode)) for mode in modes}
        t, last = alternate(fns, reps, warmup)
        n = int(last[repr(False)]["activation_counts"].sum())
        emit(f"{name}: {rows} rows, {n} activations ({n / rows:.1f} per row)")
        for mode in modes:
            emit(f"  compute_activation_stats(with_tokens={mode!r:6}) {fmt(t[repr(mode)])} ms")
        for mode in modes:
            if mode is not False:
                extra = t[repr(mode)][0] - t[repr(False)][0]
                emit(f"  tokens per feature, with_tokens={mode!r:6}: {extra:10.2f} ms over with_tokens=False")
        if "csr" in modes:
            from quantizedsae_amd.inference import TokenLists, token_lists_to_python
            emit(f"  \"csr\" is x{(t[repr(True)][0] - t[repr(False)][0]) / max(t[repr('csr')][0] - t[repr(False)][0], 1e-3):.1f} "
                 f"cheaper than True in that difference, x{t[repr(True)][0] / t[repr('csr')][0]:.1f} over the whole call")
            offsets, tokens = last[repr("csr")]["tokens_per_feature"]
            ms, as_lists = clock(lambda: token_lists_to_python(offsets, tokens))
            emit(f"  token_lists_to_python of the result: {ms:10.2f} ms; equal to the lists of with_tokens=True: "
                 f"{as_lists == last[repr(True)]['tokens_per_feature']}")
            del as_lists
            row_tok = token_ids.reshape(-1)[:rows]
            with torch.no_grad():
                if name == "b_sae":
                    idx, val = A.activation_indices(sae, x)

                    def alone():
                        lists = TokenLists(H, DEV)
                        lists.add_compact(idx, val, row_tok)
                        return lists.finish()
                else:
                    zb, index = A._packed_bits(sae.model, x)

                    def alone():
                        lists = TokenLists(H, DEV)
                        lists.add_bits(zb, index, row_tok)
                        return lists.finish()
                ta, _ = alternate({"alone": alone}, max(reps, 5), warmup)
            emit(f"  TokenLists alone (count, host read, fill): {fmt(ta['alone'])} ms; "
                 f"results {4 * n / 1e6:.1f} MB + bitmap {H * ((rows + 63) // 64) * 8 / 1e6:.1f} MB")
        last.clear()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--parent", type=Path, default=None, help="a built checkout of the parent commit to time as well")
    ap.add_argument("--out", type=Path, default=None, help="also write the report to this file")
    ap.add_argument("--child-root", type=Path, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    if args.child_root is not None:
        run(args.child_root.resolve(), args.rows, args.reps, args.warmup, (False, True), emit)
        return 0
    import torch
    emit(f"device {torch.cuda.get_device_name(0)}; median (min / max) ms of {args.reps} calls after {args.warmup}, modes alternated; "
         f"H {H}, D {D}, tokens_per_context {TPC}")
    run(Path(__file__).resolve().parents[1], args.rows, args.reps, args.warmup, (False, "csr", True), emit)
    if args.parent is not None:
        emit(f"parent commit ({args.parent}), its own build, child process, same inputs:")
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child-root", str(args.parent), "--rows", str(args.rows),
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        for line in r.stdout.splitlines():
            emit("  " + line)
        if r.returncode != 0:
            emit(f"  parent run failed ({r.returncode}): {r.stderr[-1500:]}")
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
