#!/usr/bin/env python3
"""Time the AuxK pieces (csrc/auxk.hip, quantizedsae_amd/training/auxk.py) at the reference's config
(B = 8192, D = 512, H = 32768) on one card:

* (a) ``ops.encode_topk_units`` (k = 64) against the composition of existing ops it replaces -- ``index_select`` of the listed
  rows of W and bias, ``ops.encode_topk`` on the copy, the positions mapped back through the list -- for lists of 1024, 8192
  and 16384 units.  The two sides' outputs are compared before anything is timed.
* (b) ``ops.auxk_loss`` against the same arithmetic in torch ops (fp32, torch's own summation order).
* (c) ``Trainer._step`` for ``b_sae`` and ``baseline_sae`` with ``aux_k=64`` over a fixed list of that many units against the
  same Trainer with ``aux_k=None`` (not one line of that path differs from a tree without the feature), and the pieces of the
  auxiliary term on their own: its forward (subset top-k, sparse decode, loss), the kernels of its backward (which write
  dense [H, D] and decoder-shaped gradients), and the additions with which autograd accumulates those into ``.grad``.

The method is tools/bench_trainer.py's: one process, the sides alternating; a window is ``steps`` iterations between two
device events and ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its
slowest window beats the other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

    python tools/bench_auxk.py [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae] [--lists 1024 8192 16384]
                               [--skip-steps]
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

from bench_activity import CONFIG, params, verdict  # noqa: E402
from bench_optim import alternate, fmt  # noqa: E402
from quantizedsae_amd import ops, synthetic as S  # noqa: E402
from quantizedsae_amd.optim import Adam  # noqa: E402
from quantizedsae_amd.sae.topk import sparse_backward  # noqa: E402
from quantizedsae_amd.training import Trainer  # noqa: E402
from quantizedsae_amd.training.trainer import _build_model  # noqa: E402

D, H, B, K_AUX, COEF, BATCHES = 512, 32768, 8192, 64, 1 / 32, 4
DEV = "cuda:0"
WINDOW = 1_000_000


def unit_list(n: int) -> torch.Tensor:
    """n distinct units in ascending order, spread over the dictionary by a seeded permutation"""
    gen = torch.Generator(device=DEV).manual_seed(11)
    return torch.randperm(H, device=DEV, generator=gen)[:n].sort().values.to(torch.int32)


def composed(x, W, bias, units, k):
    n = units.numel()
    assert n % 4 == 0
    sel = units.long()
    pos, val = ops.encode_topk(x, W.index_select(0, sel), bias.index_select(0, sel), k)
    return units[pos.long()], val


def bench_topk(args):
    x = torch.from_numpy(S.activations(5, B, D)).to(DEV)
    sd = S.baseline_sae_params(7, D, H)
    W, bias = torch.from_numpy(sd["encoder.0.weight"]).to(DEV), torch.from_numpy(sd["encoder.0.bias"]).to(DEV)
    for n in args.lists:
        units = unit_list(n)
        a, b = ops.encode_topk_units(x, W, bias, units, K_AUX), composed(x, W, bias, units, K_AUX)
        equal = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
        got = alternate({"kernel": lambda: ops.encode_topk_units(x, W, bias, units, K_AUX),
                         "composition": lambda: composed(x, W, bias, units, K_AUX)}, args.steps, args.warmup, args.repeats)
        out = {"what": "encode_topk_units_vs_composition", "B": B, "D": D, "H": H, "n_units": n, "k": K_AUX, "same_bits": equal,
               "kernel": fmt(got["kernel"]), "composition": fmt(got["composition"]), "kernel_is": verdict(got["kernel"], got["composition"]),
               "median_ratio": round(got["kernel"][0] / got["composition"][0], 4),
               "kernel_TFLOPs": round(2.0 * B * n * D / (got["kernel"][0] * 1e-3) / 1e12, 2)}
        print(json.dumps(out), flush=True)


def torch_loss(x, recon, aux, coef):
    e = x - recon
    q = aux - e
    Dn = ((e - e.mean(0)) ** 2).sum()
    return coef * (q * q).sum() / Dn, (2 * coef / Dn) * q


def bench_loss(args):
    x, recon, aux = (torch.from_numpy(S.activations(21 + i, B, D)).to(DEV) for i in range(3))
    a, b = ops.auxk_loss(x, recon, aux, COEF), torch_loss(x, recon, aux, COEF)
    rel = abs(a[0].item() - b[0].item()) / abs(b[0].item())
    got = alternate({"kernel": lambda: ops.auxk_loss(x, recon, aux, COEF), "torch_ops": lambda: torch_loss(x, recon, aux, COEF)},
                    args.steps, args.warmup, args.repeats)
    # what the algorithm moves: x, recon twice, aux once; grad written twice and read once
    moved = 8 * B * D * 4
    out = {"what": "auxk_loss_vs_torch_ops", "B": B, "D": D, "loss_rel_diff": float(f"{rel:.3g}"), "kernel": fmt(got["kernel"]),
           "torch_ops": fmt(got["torch_ops"]), "kernel_is": verdict(got["kernel"], got["torch_ops"]),
           "median_ratio": round(got["kernel"][0] / got["torch_ops"][0], 4),
           "kernel_GBps": round(moved / (got["kernel"][0] * 1e-3) / 1e9, 1)}
    print(json.dumps(out), flush=True)


def make_trainer(sae_type, sd, tmp, units):
    model = _build_model(sae_type, CONFIG)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    t = Trainer(CONFIG, sae_type, False, True, model=model.to(DEV), dataset_dir=tmp, save_dir=tmp, activity_window=WINDOW,
                aux_k=K_AUX if units is not None else None, aux_coef=COEF, aux_refresh=1 << 40)
    if units is not None:
        t._aux_units, t._aux_steps = units, 1                 # a fixed list: no refresh inside the timed windows
    return t


def bench_steps(sae_type, n, batches, tmp, args):
    sd = params(sae_type)
    units = unit_list(n)
    sides = {}
    for name, u in (("with_aux_k", units), ("without", None)):
        t = make_trainer(sae_type, sd, tmp, u)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
        if u is not None:
            model = t.model
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    # the pieces of the auxiliary term, on the model of the "with" side
    x = batches[0]
    recon = torch.from_numpy(S.activations(31, B, D)).to(DEV)
    lin = model.encoder.linear
    dec_param, table, step_size = model._aux_decoder()
    idx, val = ops.encode_topk_units(x, lin.weight.detach(), lin.bias.detach(), units, K_AUX)
    g = torch.from_numpy(S.activations(32, B, D)).to(DEV)

    def forward():
        with torch.no_grad():
            i, v = ops.encode_topk_units(x, lin.weight.detach(), lin.bias.detach(), units, K_AUX)
            ops.auxk_loss(x, recon, ops.decode_table_sparse(i, v, table, step_size, None), COEF)

    def backward_kernels():
        return sparse_backward(idx, table, step_size, g, None, lin.weight, None, (False, True, True, True, False), x.dtype,
                               lambda off, ent, gv: model._aux_unit_grad(off, ent, val, gv, x, g, True, True))
    grads = [t_ for t_ in backward_kernels() if t_ is not None]
    sums = [torch.zeros_like(t_) for t_ in grads]

    def accumulate():
        for s_, g_ in zip(sums, grads):
            s_.add_(g_)
    parts = alternate({"forward": forward, "backward_kernels": backward_kernels, "accumulate": accumulate}, args.steps, args.warmup,
                      args.repeats)
    full = got["with_aux_k"][0]
    out = {"what": "train_step", "sae_type": sae_type, "B": B, "D": D, "H": H, "aux_k": K_AUX, "n_units": n, "steps": args.steps,
           "repeats": args.repeats, "with_aux_k": fmt(got["with_aux_k"]), "without": fmt(got["without"]),
           "with_aux_k_is": verdict(got["with_aux_k"], got["without"]), "median_ratio": round(full / got["without"][0], 4),
           "aux_forward": fmt(parts["forward"]), "aux_backward_kernels": fmt(parts["backward_kernels"]),
           "aux_grad_accumulate": fmt(parts["accumulate"]), "dense_grad_MiB": sum(t_.numel() for t_ in grads) * 4 >> 20,
           "share_of_step_backward_kernels": round(parts["backward_kernels"][0] / full, 4),
           "share_of_step_accumulate": round(parts["accumulate"][0] / full, 4)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--lists", nargs="*", type=int, default=[1024, 8192, 16384])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true", help="parts (a) and (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_auxk.py needs cuda:0 (MI355X); nothing is timed without it")
    bench_topk(args)
    bench_loss(args)
    if args.skip_steps:
        return
    batches = [torch.from_numpy(S.activations(5 + i, B, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            for n in args.lists:
                bench_steps(sae_type, n, batches, tmp, args)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
