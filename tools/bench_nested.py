#!/usr/bin/env python3
"""Time the nested-dictionary objective of the top-k SAEs (csrc/nested.hip, quantizedsae_amd/training/nested.py; DESIGN.md
section 4.31) at H = 32768, D = 512, k = 65, L = 4 levels ``[H/8, H/4, H/2, H]`` on one card, against what the same objective
costs with the ops the library had before:

* (a) decode: ``ops.decode_nested_*`` (one walk per row) against L calls of ``ops.decode_*_sparse`` on lists whose removed
  entries carry a value of 0 -- for the soft table (what training decodes from) and for the packed dictionary.  The two sides'
  outputs are compared before anything is timed.
* (b) backward: ``train_row_grad_nested`` + ``train_csr`` + ``train_*unit_grad_nested`` + ``train_col_sum`` against L calls of
  ``train_row_grad`` and of ``train_*unit_grad`` (one per level with g_recon = G[level], the results merged by level) + the
  same ``train_csr`` and ``train_col_sum``.
* (c) the whole step: ``Trainer._step`` with ``nested_bounds="default"`` against the same Trainer without it (the plain
  ``forward_train`` step, whose objective has one level).

The method is tools/bench_trainer.py's: one process, the sides alternating; a window is ``steps`` iterations between two
device events and ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its
slowest window beats the other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

    python tools/bench_nested.py [--batch 8192] [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae]
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
from quantizedsae_amd.sae import BinarySAE  # noqa: E402
from quantizedsae_amd.training import Trainer, default_nested_bounds  # noqa: E402
from quantizedsae_amd.training.trainer import _build_model  # noqa: E402

D, H, K, LEVELS, BATCHES = 512, 32768, 65, 4, 4
DEV = "cuda:0"


def make_model(sae_type):
    model = _build_model(sae_type, CONFIG)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params(sae_type).items()})
    if isinstance(model, BinarySAE):
        assert model.top_k == K
    else:
        model.topk = K
    return model.to(DEV)


def line(what, sae_type, B, got, new, old, **more):
    out = {"what": what, "sae_type": sae_type, "B": B, "D": D, "H": H, "k": K, "levels": LEVELS, new: fmt(got[new]),
           old: fmt(got[old]), f"{new}_is": verdict(got[new], got[old]), "median_ratio": round(got[new][0] / got[old][0], 4)}
    out.update(more)
    print(json.dumps(out), flush=True)


def bench_decode(sae_type, model, x, bounds, args):
    B = x.shape[0]
    with torch.no_grad():
        idx, val, _ = model._nested_select(x, False)
        table, step, _ = model._nested_train_decoder()
        bias = model.decoder.bias.detach()
        forms = [("table", lambda: ops.decode_nested_table(idx, val, table, step, bias, bounds),
                  lambda v: ops.decode_table_sparse(idx, v, table, step, bias))]
        if isinstance(model, BinarySAE):
            dec = model.decoder
            packed = dec.packed()["packed"]
            forms.append(("packed", lambda: ops.decode_nested_binary(idx, val, packed, D, dec.n_bits, step, bias, bounds),
                          lambda v: ops.decode_binary_sparse(idx, v, packed, D, dec.n_bits, step, bias)))
        masked = [torch.where(idx < b, val, torch.zeros_like(val)) for b in bounds]
        for form, nested, plain in forms:
            def per_level(plain=plain):
                return [plain(v) for v in masked]
            equal = all(torch.equal(a, b) for a, b in zip(nested(), per_level()))
            got = alternate({"nested": nested, "per_level": per_level}, args.steps, args.warmup, args.repeats)
            line("decode", sae_type, B, got, "nested", "per_level", form=form, same_bits=bool(equal))
    return idx, val, table, step


def bench_backward(sae_type, model, x, bounds, idx, val, table, step, args):
    B = x.shape[0]
    W = model.encoder.linear.weight.detach()
    g = [torch.from_numpy(S.activations(40 + l, B, D)).to(DEV) * (1.0 / (B * D)) for l in range(LEVELS)]
    binary = isinstance(model, BinarySAE)
    logits = model.decoder.weight.detach()
    unit_levels = torch.bucketize(torch.arange(H, device=DEV), torch.tensor(bounds, device=DEV), right=True)
    entry_levels = torch.bucketize(idx.long(), torch.tensor(bounds, device=DEV), right=True)

    def nested():
        G, gv, _ = ops.train_row_grad_nested(idx, table, step, g, bounds, None, None)
        offsets, entries = ops.train_csr(idx, H)
        if binary:
            out = ops.train_unit_grad_nested(offsets, entries, val, gv, x, G, bounds, logits, model.decoder.n_bits, step, None)
        else:
            out = ops.train_table_unit_grad_nested(offsets, entries, val, gv, x, G, bounds)
        return out + (ops.train_col_sum(G[0]),)

    def per_level():
        G = [g[-1]]
        for l in range(LEVELS - 2, -1, -1):
            G.insert(0, g[l] + G[0])
        gv = None
        for l in range(LEVELS):
            gv_l, _ = ops.train_row_grad(idx, table, step, G[l], None, None)
            gv = gv_l if gv is None else torch.where(entry_levels == l, gv_l, gv)
        offsets, entries = ops.train_csr(idx, H)
        ddec = None
        for l in range(LEVELS):
            if binary:
                dW, db, dd = ops.train_unit_grad(offsets, entries, val, gv, x, G[l], logits, model.decoder.n_bits, step, None,
                                                 want_encoder=l == 0)
                mine = (unit_levels == l)[:, None]
            else:
                dW, db, dd = ops.train_table_unit_grad(offsets, entries, val, gv, x, G[l], want_encoder=l == 0)
                mine = (unit_levels == l)[None, :]
            if l == 0:
                keep = (dW, db)
            ddec = dd if ddec is None else torch.where(mine, dd, ddec)
        return keep + (ddec, ops.train_col_sum(G[0]))
    with torch.no_grad():
        equal = all(torch.equal(a, b) for a, b in zip(nested(), per_level()))
        got = alternate({"nested": nested, "per_level": per_level}, args.steps, args.warmup, args.repeats)
    line("backward", sae_type, B, got, "nested", "per_level", same_bits=bool(equal))


def bench_steps(sae_type, batches, tmp, args):
    sides = {}
    for name, nb in (("nested", "default"), ("plain", None)):
        t = Trainer(CONFIG, sae_type, False, True, model=make_model(sae_type), dataset_dir=tmp, save_dir=tmp, nested_bounds=nb)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    line("train_step", sae_type, batches[0].shape[0], got, "nested", "plain", steps=args.steps, repeats=args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nested.py needs cuda:0 (MI355X); nothing is timed without it")
    assert (CONFIG["input_dim"], CONFIG["hidden_dim"]) == (D, H)
    bounds = default_nested_bounds(H, LEVELS)
    batches = [torch.from_numpy(S.activations(5 + i, args.batch, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            model = make_model(sae_type)
            idx, val, table, step = bench_decode(sae_type, model, batches[0], bounds, args)
            bench_backward(sae_type, model, batches[0], bounds, idx, val, table, step, args)
            del model
            torch.cuda.empty_cache()
            bench_steps(sae_type, batches, tmp, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
