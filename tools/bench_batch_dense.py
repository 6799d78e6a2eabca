#!/usr/bin/env python3
"""Time the dense BatchTopK encoder (csrc/batch_dense.hip) against the capped path it stands next to, at
H = 32768, D = 512, 8192 rows on one card, at the list widths K = 256 (k = 65) and K = 64 (k = 16: a controller takes k <= K,
and K = 4 k is its default relation).

* (a) select: ``ops.encode_batch_topk`` under a floor of ``ratio * m`` (m: the batch's smallest selected value; what a training
  step leaves behind) against the capped path's two calls: the model's top-K selection ``_select_cap`` at K plus
  ``ops.batch_select``.  A second line times the same call under a floor of 2 m, which fails the certificate, so that the second
  attempt runs.
* (b) the whole step: ``Trainer._step`` with ``batch_topk=True, batch_topk_dense=True`` against ``batch_topk=True`` alone, the
  same cap, both with the HIP Adam; plain and with ``batch_topk_nested_bounds="default"``.
* (c) how often the second attempt runs: ``--rate-steps`` training steps over the batches in turn at every ``--ratios`` value,
  the count kept on the device (``BatchTopK.second_attempts``) and read once at the end, with the candidates per row of the
  last step.

The capped side is the code of the parent commit, untouched by this feature, and runs in the same process.  The two sides'
outputs are compared before anything is timed: the counts, the report's four words, and the lists over every row's first
counts[r] places.

The method is tools/bench_trainer.py's: the sides alternating; a window is ``steps`` iterations between two device events and
ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its slowest window beats the
other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

    python tools/bench_batch_dense.py [--batch 8192] [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_activity import CONFIG, verdict  # noqa: E402
from bench_nested import D, DEV, H, K, make_model  # noqa: E402
from bench_optim import alternate, fmt  # noqa: E402
from quantizedsae_amd import ops, synthetic as S  # noqa: E402
from quantizedsae_amd.optim import Adam  # noqa: E402
from quantizedsae_amd.training import BatchTopK, Trainer  # noqa: E402

CAPS, BATCHES, RATIOS = (256, 64), 4, (0.99, 0.97, 0.95, 0.9, 0.8)
K_AT = {256: K, 64: 16}                                       # the k of a list width


def model_at(sae_type, cap):
    """make_model with the top-k of the list width"""
    model = make_model(sae_type)
    k = K_AT.get(cap, max(1, cap // 4))
    if hasattr(model, "topk"):
        model.topk = k
    else:
        model.k = (k + 0.5) / H
        assert model.top_k == k
    return model, k


def line(what, sae_type, B, cap, got, new, old, **more):
    out = {"what": what, "sae_type": sae_type, "B": B, "D": D, "H": H, "k": K_AT.get(cap, max(1, cap // 4)), "cap": cap,
           new: fmt(got[new]), old: fmt(got[old]),
           f"{new}_is": verdict(got[new], got[old]), "median_ratio": round(got[new][0] / got[old][0], 4)}
    out.update(more)
    print(json.dumps(out), flush=True)


def same_prefixes(a, b, counts):
    """the two [B, K] lists agree over every row's first counts[r] places"""
    inside = torch.arange(a.shape[1], device=a.device)[None, :] < counts[:, None]
    return bool(torch.equal(torch.where(inside, a, torch.zeros_like(a)), torch.where(inside, b, torch.zeros_like(b))))


def bench_ops(sae_type, model, x, cap, ratio, args):
    B = x.shape[0]
    n_select = B * K_AT.get(cap, max(1, cap // 4))
    with torch.no_grad():
        lin = model.encoder.linear
        W, b = lin.weight.detach(), lin.bias.detach()

        def capped():
            idx, val = model._select_cap(x, cap, "bench")
            return (idx,) + tuple(ops.batch_select(val, n_select))

        c = capped()
        m = float(c[3][3:4].to(torch.int32).view(torch.float32))

        def dense(floor=ratio * m):
            return ops.encode_batch_topk(x, W, b, n_select, cap, floor, 1.0)

        def second():
            return ops.encode_batch_topk(x, W, b, n_select, cap, 2.0 * m, 1.0)
        for name, fn in (("certified", dense), ("second attempt", second)):
            d = fn()
            same = bool(torch.equal(c[1], d[2]) and torch.equal(c[3], d[3][:4])) and same_prefixes(c[0], d[0], c[1]) and \
                same_prefixes(c[2].view(torch.int32), d[1].view(torch.int32), c[1])
            rep = d[3].tolist()
            more = dict(same_outputs=same, n_select=n_select, floor=ratio * m if fn is dense else 2.0 * m, smallest_selected=m,
                        candidates_per_row=rep[4] / B, rows_over_cap=rep[6], second_attempt=rep[5], saturated_rows=rep[1])
            if fn is dense:
                got = alternate({"encode_batch_topk": fn, "select_cap_batch_select": capped}, args.steps, args.warmup, args.repeats)
                line("select", sae_type, B, cap, got, "encode_batch_topk", "select_cap_batch_select", floor_ratio=ratio, **more)
            else:
                got = alternate({"encode_batch_topk_second_attempt": fn, "select_cap_batch_select": capped}, 2, 1, 3)
                line("select_second_attempt", sae_type, B, cap, got, "encode_batch_topk_second_attempt", "select_cap_batch_select",
                     **more)


def make_trainer(sae_type, cap, tmp, dense, nested, ratio):
    return Trainer(CONFIG, sae_type, False, True, model=model_at(sae_type, cap)[0], dataset_dir=tmp, save_dir=tmp, batch_topk=True,
                   batch_topk_cap=cap, batch_topk_dense=dense, batch_topk_nested_bounds="default" if nested else None,
                   **({"batch_topk_floor_ratio": ratio} if dense else {}))


def bench_steps(sae_type, batches, cap, nested, ratio, tmp, args):
    sides, trainers = {}, {}
    for name, dense in (("dense", True), ("capped", False)):
        t = trainers[name] = make_trainer(sae_type, cap, tmp, dense, nested, ratio)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    e = trainers["dense"].batch_topk.dense_summary()
    line("train_step_nested" if nested else "train_step", sae_type, batches[0].shape[0], cap, got, "dense", "capped", steps=args.steps,
         repeats=args.repeats, floor_ratio=ratio, dense_selections=e["dense_selections"], second_attempts=e["second_attempts"],
         candidates_per_row=e["candidates_per_row"])


def second_attempt_rate(sae_type, batches, cap, tmp, args):
    for ratio in args.ratios:
        t = make_trainer(sae_type, cap, tmp, True, False, ratio)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        for i in range(args.rate_steps):
            t._step(opt, batches[i % len(batches)], False)
        e = t.batch_topk.dense_summary()
        print(json.dumps({"what": "second_attempt_rate", "sae_type": sae_type, "B": batches[0].shape[0], "cap": cap, "floor_ratio": ratio,
                          "steps": args.rate_steps, "dense_selections": e["dense_selections"], "second_attempts": e["second_attempts"],
                          "candidates_per_row_last": e["candidates_per_row"], "rows_over_cap_last": e["rows_over_cap"],
                          "lr": CONFIG["lr"], "distinct_batches": len(batches)}), flush=True)
        del t, opt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--caps", nargs="*", type=int, default=list(CAPS))
    ap.add_argument("--ratios", nargs="*", type=float, default=list(RATIOS))
    ap.add_argument("--ratio", type=float, default=BatchTopK.DEFAULT_FLOOR_RATIO, help="the floor ratio of the timed cases")
    ap.add_argument("--rate-steps", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-rate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_dense.py needs cuda:0 (MI355X); nothing is timed without it")
    assert (CONFIG["input_dim"], CONFIG["hidden_dim"]) == (D, H)
    batches = [torch.from_numpy(S.activations(5 + i, args.batch, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            for cap in args.caps:
                if not args.skip_rate and cap == max(args.caps):
                    second_attempt_rate(sae_type, batches, cap, tmp, args)
                model, _ = model_at(sae_type, cap)
                bench_ops(sae_type, model, batches[0], cap, args.ratio, args)
                del model
                torch.cuda.empty_cache()
                for nested in (False, True):
                    bench_steps(sae_type, batches, cap, nested, args.ratio, tmp, args)
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
