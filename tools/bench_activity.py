#!/usr/bin/env python3
"""Time what ``Trainer(..., activity_window=W)`` adds to a training step (csrc/activity.hip,
quantizedsae_amd/training/activity.py), at the reference's config (B = 8192, D = 512, H = 32768) on one card:

* ``Trainer._step`` with and without ``activity_window`` for the six ``sae_type``s.  The side without is this same tree with
  the option off: not one line of that path differs from a tree without the feature.
* ``add_dense`` on the [8192, 32768] latent against ``ops.train_col_sum`` on the same tensor: both read it once.
* the summary (one kernel call and one host copy), with and without the dead list, as a logging step pays it.

The method is tools/bench_trainer.py's: one process, the sides alternating; a window is ``steps`` iterations between two
device events and ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its
slowest window beats the other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

    python tools/bench_activity.py [--steps 10] [--warmup 3] [--repeats 5] [--types ...]
                                   [--kernels-only]   (ten launches of each kernel at the bench shapes and of train_col_sum,
                                                       for a kernel trace)
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_optim import alternate, faster, fmt  # noqa: E402
from quantizedsae_amd import ops, synthetic as S  # noqa: E402
from quantizedsae_amd.optim import Adam  # noqa: E402
from quantizedsae_amd.sae.quantized_matryoshka import nested_sizes  # noqa: E402
from quantizedsae_amd.training import FeatureActivity, SAE_TYPES, Trainer  # noqa: E402
from quantizedsae_amd.training.trainer import _build_model  # noqa: E402

D, H, B, N_BITS, BATCHES = 512, 32768, 8192, 4, 4
CONFIG = {"input_dim": D, "n_bits": N_BITS, "hidden_dim": H, "gamma": 1.5, "epochs": 1, "lr": 1e-4, "top_k": 32,
          "sparsity_lambda": 1.5e-3, "polarize_lambda": 1e-2, "batch_size": B}
DEV = "cuda:0"
WINDOW = 1_000_000


def verdict(new, old):
    if faster(new, old):
        return "faster"
    if faster(old, new):
        return "slower"
    return "not distinguishable"


def params(sae_type):
    if sae_type == "b_sae":
        return S.binary_sae_params(7, D, H, 8, logit_std=1.0, dec_bias_std=0.1)       # 8 bits: the reference's constructor call
    if sae_type == "baseline_sae":
        return S.baseline_sae_params(7, D, H)
    if sae_type == "t_sae":
        return S.ternary_sae_params(7, D, H)
    if sae_type == "bl_sae":
        return {"encoder.0.weight": S.xavier_uniform(7, H, D, stream=1), "encoder.0.bias": S.normal(7, (H,), stream=2, std=0.05),
                "decoder.weight": S.uniform(7, (D, H), -1.0 / np.sqrt(H), 1.0 / np.sqrt(H), stream=3),
                "decoder.bias": S.normal(7, (D,), stream=4, std=0.1)}
    if sae_type == "q_sae":
        return S.matryoshka_sae_params(7, D, H, bias_std=0.1, enc_bias_sigmas=-2.5)
    sd = {}
    for i, h in enumerate(nested_sizes(H, N_BITS)):
        for k, v in S.matryoshka_sae_params(7, D, h, bias_std=0.1, stream0=16 * i, enc_bias_sigmas=-2.5).items():
            sd[f"saes.{i}.{k}"] = v
    return sd


def make_trainer(sae_type, sd, tmp, window):
    model = _build_model(sae_type, CONFIG)
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys, res
    model = model.to(DEV)
    if sae_type == "t_sae":
        model.decoder.init_mask(0.7)
    t = Trainer(CONFIG, sae_type, sae_type == "t_sae", True, model=model, dataset_dir=tmp, save_dir=tmp, activity_window=window)
    t.f_decay = 0.3
    return t


def bench_steps(sae_type, batches, tmp, args):
    sd = params(sae_type)
    sides, trainers = {}, {}
    for name, window in (("with_activity", WINDOW), ("without", None)):
        t = trainers[name] = make_trainer(sae_type, sd, tmp, window)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    act = trainers["with_activity"].activity
    s = act.summary(WINDOW)
    out = {"what": "train_step", "sae_type": sae_type, "B": B, "D": D, "H": H, "steps": args.steps, "repeats": args.repeats}
    out.update({w: fmt(v) for w, v in got.items()})
    out["with_activity_is"] = verdict(got["with_activity"], got["without"])
    out["median_ratio"] = round(got["with_activity"][0] / got["without"][0], 4)
    out["rows_seen"], out["mean_l0"], out["never_fired"] = act.rows_seen, round(s.mean_l0, 2), s.never
    print(json.dumps(out), flush=True)


def dense_latent():
    gen = torch.Generator(device=DEV).manual_seed(3)
    return torch.relu(torch.randn((B, H), device=DEV, generator=gen))


def bench_dense(args):
    h = dense_latent()
    t = FeatureActivity(H, DEV)
    got = alternate({"add_dense": lambda: t.add_dense(h), "train_col_sum": lambda: ops.train_col_sum(h)},
                    args.steps, args.warmup, args.repeats)
    assert torch.equal(t.fired, (h > 0).sum(0) * (t.rows_seen // B))
    ratio = got["add_dense"][0] / got["train_col_sum"][0]
    out = {"what": "add_dense_vs_train_col_sum", "B": B, "H": H, "MiB_read": B * H * 4 >> 20, "add_dense": fmt(got["add_dense"]),
           "train_col_sum": fmt(got["train_col_sum"]), "median_ratio": round(ratio, 3), "within_1.5x": bool(ratio <= 1.5),
           "add_dense_GBps": round(B * H * 4 / (got["add_dense"][0] * 1e-3) / 1e9, 1)}
    print(json.dumps(out), flush=True)


def activity_state():
    t = FeatureActivity(H, DEV, nested_sizes(H, N_BITS))
    gen = torch.Generator(device=DEV).manual_seed(5)
    idx = torch.randint(0, H // 2, (B, 65), device=DEV, generator=gen, dtype=torch.int32)     # half of the units never fire
    t.add_compact(idx, None)
    return t, idx


def bench_summary(args):
    t, _ = activity_state()
    got = alternate({"summary": lambda: t.summary(B, advance=False), "summary_with_dead_list": lambda: t.summary(B, dead_list=True, advance=False)},
                    args.steps, args.warmup, args.repeats)
    s = t.summary(B, dead_list=True, advance=False)
    out = {"what": "summary", "H": H, "levels": len(t.level_sizes), "dead": s.dead, "summary": fmt(got["summary"]),
           "summary_with_dead_list": fmt(got["summary_with_dead_list"])}
    print(json.dumps(out), flush=True)


def trace_kernels(runs=10):
    """For a kernel trace: ten launches of each kernel at the bench shapes -- compact 8192 x 65, bits 8192 x 32768 at about
    4 % density through a permutation, dense 8192 x 32768 -- of the summary with its dead list, and of train_col_sum on the
    same dense tensor."""
    t, idx = activity_state()
    gen = torch.Generator(device=DEV).manual_seed(9)
    val = torch.randn((B, 65), device=DEV, generator=gen)
    z = (torch.rand((B, H // 32, 32), device=DEV, generator=gen) < 0.04).to(torch.int64)
    z = (z << torch.arange(32, device=DEV)).sum(-1).to(torch.int32)
    index = torch.randperm(H, device=DEV, generator=gen).to(torch.int32)
    h = dense_latent()
    for _ in range(runs):
        t.add_compact(idx, val)
        t.add_bits(z, index)
        t.add_dense(h)
        ops.train_col_sum(h)
        t.summary(B, dead_list=True, advance=False)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=list(SAE_TYPES), choices=list(SAE_TYPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="ten launches of each kernel (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_activity.py needs cuda:0 (MI355X); nothing is timed without it")
    if args.kernels_only:
        trace_kernels()
        return
    bench_dense(args)
    bench_summary(args)
    batches = [torch.from_numpy(S.activations(5 + i, B, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            bench_steps(sae_type, batches, tmp, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
