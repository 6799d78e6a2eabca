#!/usr/bin/env python3
"""Time the per-row top-k over hidden slabs (include/qsae_wide.h, ``latent_path = "slabs"``) on one card, D = 512:

* the selection alone (compact lists, no dense latent), ``ops.encode_topk_wide`` with the fp16 prefilter copy, against
  - at H = 65536 the one-piece ``ops.encode_topk_prefilter`` (the parent's path; the bits are compared first), and
  - at every H the same result composed from existing ops: ``ops.encode_topk_prefilter`` on every slab's row range,
    ``torch.cat``, ``torch.topk``, two gathers (values compared first; torch.topk orders ties its own way);
* the training step of a BaselineSparseAutoencoder with ``topk = k`` -- forward_train(dense_latent=False), the loss, backward,
  optim.Adam(model=...), normalize -- under ``"slabs"``, and at H = 65536 under ``"auto"`` as well.

Protocol of tools/bench_trainer.py: one process, the sides of a comparison alternating, a window of `steps` iterations between
two device events, median [min .. max] over `repeats` windows; a side is "faster" only when its slowest window beats the other
side's fastest.  One JSON line per case.

    python tools/bench_wide.py [--steps 5] [--warmup 2] [--repeats 5] [--H 65536 131072 262144] [--B 8192 65536] [--k 65 256]
                               [--no-train]
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

from bench_optim import alternate, faster, fmt  # noqa: E402
from quantizedsae_amd import BaselineSparseAutoencoder, ops  # noqa: E402
from quantizedsae_amd.training import Trainer  # noqa: E402

D, DEV = 512, "cuda:0"


def verdict(new, old):
    return "faster" if faster(new, old) else ("slower" if faster(old, new) else "not distinguishable")


def operands(B, H):
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((B, D), device=DEV, generator=g)
    bound = (6.0 / (D + H)) ** 0.5
    W = (torch.rand((H, D), device=DEV, generator=g) * 2 - 1) * bound
    b = torch.randn((H,), device=DEV, generator=g) * 0.05
    return x, W, b


def bench_selection(B, H, k, args):
    x, W, b = operands(B, H)
    Wq, meta = ops.prefilter_pack_w(W, b)
    starts = ops.wide_plan(H, k)
    info = {}

    def slabs():
        return ops.encode_topk_wide(x, W, b, k, Wq=Wq, meta=meta, want_dense=False, info=info)

    def composed():
        vals, idxs = [], []
        for h0, h1 in zip(starts, starts[1:]):
            i, v, _ = ops.encode_topk_prefilter(x, W[h0:h1], b[h0:h1], Wq[h0:h1], meta, k, want_dense=False)
            vals.append(v)
            idxs.append(i + h0)
        v, pos = torch.topk(torch.cat(vals, dim=1), k, dim=1)
        return torch.gather(torch.cat(idxs, dim=1), 1, pos), v

    idx, val, _ = slabs()
    ci, cv = composed()
    assert torch.equal(cv, val), "the composition's values differ"
    sides = {"slabs": slabs, "composed_from_existing_ops": composed}
    if ops.prefilter_supported(B, D, H, k):
        def one_piece():
            return ops.encode_topk_prefilter(x, W, b, Wq, meta, k, want_dense=False)
        oi, ov, _ = one_piece()
        assert torch.equal(oi, idx) and torch.equal(ov.view(torch.int32), val.view(torch.int32)), "slabs differ from the one-piece path"
        sides["one_piece"] = one_piece
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    out = {"what": "selection", "B": B, "D": D, "H": H, "k": k, "slabs": len(starts) - 1, "flagged_rows": info["flagged_rows"]}
    out.update({name: fmt(stat) for name, stat in got.items()})
    out["slabs_vs_composed"] = verdict(got["slabs"], got["composed_from_existing_ops"])
    if "one_piece" in got:
        out["slabs_vs_one_piece"] = verdict(got["slabs"], got["one_piece"])
    print(json.dumps(out), flush=True)


def bench_step(B, H, k, args, tmp):
    config = {"input_dim": D, "n_bits": 4, "hidden_dim": H, "gamma": 1.5, "epochs": 1, "lr": 1e-4, "top_k": k,
              "sparsity_lambda": 1.5e-3, "polarize_lambda": 1e-2, "batch_size": B}
    x, W, b = operands(B, H)
    sides = {}
    for path in ("slabs", "auto"):
        if path == "auto" and not ops.prefilter_supported(B, D, H, k):
            continue
        with torch.device(DEV):
            m = BaselineSparseAutoencoder(D, H)
        with torch.no_grad():
            m.encoder.linear.weight.copy_(W)
            m.encoder.linear.bias.copy_(b)
        m.topk, m.latent_path = k, path
        trainer = Trainer(config, "baseline_sae", False, True, model=m, dataset_dir=tmp, save_dir=tmp)
        opt = trainer._make_optimizer()
        sides[f"trainer_step_{path}"] = (lambda t=trainer, o=opt: t._step(o, x, False))
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    out = {"what": "training_step", "model": "baseline", "B": B, "D": D, "H": H, "k": k}
    out.update({name: fmt(stat) for name, stat in got.items()})
    if "trainer_step_auto" in got:
        out["slabs_vs_auto"] = verdict(got["trainer_step_slabs"], got["trainer_step_auto"])
    print(json.dumps(out), flush=True)
    del sides
    ops.release_workspaces()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--H", type=int, nargs="+", default=[65536, 131072, 262144])
    ap.add_argument("--B", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--k", type=int, nargs="+", default=[65, 256])
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        for H in args.H:
            for B in args.B:
                for k in args.k:
                    bench_selection(B, H, k, args)
                    ops.release_workspaces()
                    torch.cuda.empty_cache()
                    if not args.no_train:
                        bench_step(B, H, k, args, tmp)


if __name__ == "__main__":
    main()
