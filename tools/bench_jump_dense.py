#!/usr/bin/env python3
"""Time the dense JumpReLU encoder (csrc/jump_dense.hip) against the capped path it stands next to, at
H = 32768, D = 512, 8192 rows on one card, thresholds calibrated at k = 65 on the first batch, at the list widths K = 256 and 64.

* (a) select: ``ops.encode_jump`` (the thresholds in the epilogue of the encoder's contraction, both lists, l0, the report)
  against the capped path's two calls: the model's top-K selection ``_select_cap`` at K plus ``ops.jump_select``.
* (b) the whole step: ``Trainer._step`` with ``jumprelu=True, jumprelu_dense=True`` against ``jumprelu=True`` alone, the same
  cap, both with the HIP Adam.

The capped side is the code of the parent commit, untouched by this feature, and runs in the same process.  The two sides'
outputs are compared before anything is timed: the counts, and the lists over every row's first counts[r] places (they are the
same lists where the capped path certifies a row and no row holds more than K firing units; the lines say how many rows are
uncertified, saturated or truncated).

The method is tools/bench_trainer.py's: the sides alternating; a window is ``steps`` iterations between two device events and
ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its slowest window beats the
other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

    python tools/bench_jump_dense.py [--batch 8192] [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae]
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
from quantizedsae_amd.training import JumpReLU, Trainer  # noqa: E402

CAPS, BATCHES, L0_COEF = (256, 64), 4, 1e-3


def line(what, sae_type, B, cap, got, new, old, **more):
    out = {"what": what, "sae_type": sae_type, "B": B, "D": D, "H": H, "k": K, "cap": cap, new: fmt(got[new]), old: fmt(got[old]),
           f"{new}_is": verdict(got[new], got[old]), "median_ratio": round(got[new][0] / got[old][0], 4)}
    out.update(more)
    print(json.dumps(out), flush=True)


def same_prefixes(a, b, counts):
    """the two [B, K] lists agree over every row's first counts[r] places"""
    inside = torch.arange(a.shape[1], device=a.device)[None, :] < counts[:, None]
    return bool(torch.equal(torch.where(inside, a, torch.zeros_like(a)), torch.where(inside, b, torch.zeros_like(b))))


def calibrated(model, x):
    """log-thresholds calibrated at k on the batch from the top-256 lists, whatever cap the timed side then runs at"""
    jr = JumpReLU(model, cap=256)
    jr.calibrate(x, K)
    return jr.log_threshold.detach().clone(), jr.bandwidth


def bench_ops(sae_type, model, x, cap, args):
    B = x.shape[0]
    with torch.no_grad():
        log_theta, eps = calibrated(model, x)
        theta = log_theta.exp()
        lin = model.encoder.linear
        W, b = lin.weight.detach(), lin.bias.detach()

        def capped():
            idx, val = model._select_cap(x, cap, "bench")
            return ops.jump_select(idx, val, theta, eps)

        def dense():
            return ops.encode_jump(x, W, b, theta, cap, eps)
        c, d = capped(), dense()
        same_counts = bool(torch.equal(c[2], d[2]) and torch.equal(c[4], d[4]))
        same_lists = same_counts and same_prefixes(c[0], d[0], c[2]) and same_prefixes(c[1].view(torch.int32), d[1].view(torch.int32), c[2]) \
            and same_prefixes(c[3], d[3], c[4])
        got = alternate({"encode_jump": dense, "select_cap_jump_select": capped}, args.steps, args.warmup, args.repeats)
        rc, rd = c[6].tolist(), d[6].tolist()
        line("select", sae_type, B, cap, got, "encode_jump", "select_cap_jump_select", same_counts=same_counts, same_lists=same_lists,
             l0_dense=float(d[5]), l0_capped=float(c[5]), band_entries=rd[1], truncated_rows=rd[2], empty_rows=rd[3],
             capped_saturated_rows=rc[2], capped_uncertified_rows=rc[4], max_count=int(d[2].max()))


def bench_steps(sae_type, batches, cap, tmp, args):
    sides = {}
    for name, dense in (("dense", True), ("capped", False)):
        t = Trainer(CONFIG, sae_type, False, True, model=make_model(sae_type), dataset_dir=tmp, save_dir=tmp, jumprelu=True,
                    jumprelu_l0_coef=L0_COEF, jumprelu_cap=cap, jumprelu_dense=dense)
        with torch.no_grad():
            t.jumprelu.log_threshold.copy_(calibrated(t.model, batches[0])[0])
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        opt.add_param_group({"params": [t.jumprelu.log_threshold]})
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    line("train_step", sae_type, batches[0].shape[0], cap, got, "dense", "capped", steps=args.steps, repeats=args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--caps", nargs="*", type=int, default=list(CAPS))
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jump_dense.py needs cuda:0 (MI355X); nothing is timed without it")
    assert (CONFIG["input_dim"], CONFIG["hidden_dim"]) == (D, H)
    batches = [torch.from_numpy(S.activations(5 + i, args.batch, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            for cap in args.caps:
                model = make_model(sae_type)
                bench_ops(sae_type, model, batches[0], cap, args)
                del model
                torch.cuda.empty_cache()
                bench_steps(sae_type, batches, cap, tmp, args)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
