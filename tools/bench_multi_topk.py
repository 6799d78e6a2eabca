#!/usr/bin/env python3
"""Time the Multi-TopK objective of the top-k SAEs (csrc/multi_topk.hip, quantizedsae_amd/training/multi_topk.py; DESIGN.md
section 4.34) at H = 32768, D = 512, k = 65, ``ks = [65, 256]`` on one card, against what the same objective costs with the ops
the library had before:

* (a) decode: ``ops.decode_multik_*`` (every dictionary row gathered once) against one call of ``ops.decode_*_sparse`` per
  point on truncated copies of the lists -- for the soft table (what training decodes from) and for the packed dictionary.
  The two sides' outputs are compared bit for bit before anything is timed.
* (b) backward: ``train_row_grad_multik`` + ``train_csr`` + ``train_*unit_grad_multik`` + ``train_col_sum`` against one
  ``train_row_grad`` + ``train_csr`` + ``train_*unit_grad`` pass per point on the truncated lists, the gradients added (the sums
  run in another order, so the two sides agree to rounding, not in bits; the largest relative difference is printed).
* (c) the whole step: ``Trainer._step`` with ``multi_topk=[65, 256]`` against the plain step at ``top_k = 65`` and against the
  plain step at ``top_k = 256`` (the selection the Multi-TopK step pays for).

The method is tools/bench_trainer.py's: one process, the sides alternating; a window is ``steps`` iterations between two
device events and ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its
slowest window beats the other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

    python tools/bench_multi_topk.py [--batch 8192] [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae]
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
from quantizedsae_amd.training import Trainer  # noqa: E402
from quantizedsae_amd.training.trainer import _build_model  # noqa: E402

D, H, K, KS, BATCHES = 512, 32768, 65, [65, 256], 4
DEV = "cuda:0"


def make_model(sae_type, top_k=K):
    model = _build_model(sae_type, CONFIG)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params(sae_type).items()})
    if isinstance(model, BinarySAE):
        model.k = (top_k + 0.5) / H
        assert model.top_k == top_k
    else:
        model.topk = top_k
    return model.to(DEV)


def line(what, sae_type, B, got, new, old, **more):
    out = {"what": what, "sae_type": sae_type, "B": B, "D": D, "H": H, "k": K, "ks": KS, new: fmt(got[new]),
           old: fmt(got[old]), f"{new}_is": verdict(got[new], got[old]), "median_ratio": round(got[new][0] / got[old][0], 4)}
    out.update(more)
    print(json.dumps(out), flush=True)


def bench_decode(sae_type, model, x, args):
    B = x.shape[0]
    with torch.no_grad():
        idx, val, _ = model._select(x, KS[-1], model._select_path(B, KS[-1], "bench_multi_topk"), False)
        table, step, _ = model._nested_train_decoder()
        bias = model.decoder.bias.detach()
        cut = [(idx[:, :k].contiguous(), val[:, :k].contiguous()) for k in KS]
        forms = [("table", lambda: ops.decode_multik_table(idx, val, table, step, bias, KS),
                  lambda i, v: ops.decode_table_sparse(i, v, table, step, bias))]
        if isinstance(model, BinarySAE):
            dec = model.decoder
            packed = dec.packed()["packed"]
            forms.append(("packed", lambda: ops.decode_multik_binary(idx, val, packed, D, dec.n_bits, step, bias, KS),
                          lambda i, v: ops.decode_binary_sparse(i, v, packed, D, dec.n_bits, step, bias)))
        for form, multik, plain in forms:
            def per_point(plain=plain):
                return [plain(i, v) for i, v in cut]
            equal = all(torch.equal(a, b) for a, b in zip(multik(), per_point()))
            got = alternate({"multik": multik, "per_point": per_point}, args.steps, args.warmup, args.repeats)
            line("decode", sae_type, B, got, "multik", "per_point", form=form, same_bits=bool(equal))
    return idx, val, cut, table, step


def bench_backward(sae_type, model, x, idx, val, cut, table, step, args):
    B = x.shape[0]
    g = [torch.from_numpy(S.activations(40 + p, B, D)).to(DEV) * (1.0 / (B * D)) for p in range(len(KS))]
    binary = isinstance(model, BinarySAE)
    logits = model.decoder.weight.detach()

    def multik():
        G, gv, _ = ops.train_row_grad_multik(idx, table, step, g, KS, None, None)
        offsets, entries = ops.train_csr(idx, H)
        if binary:
            out = ops.train_unit_grad_multik(offsets, entries, val, gv, x, G, KS, logits, model.decoder.n_bits, step, None)
        else:
            out = ops.train_table_unit_grad_multik(offsets, entries, val, gv, x, G, KS)
        return out + (ops.train_col_sum(G[0]),)

    def per_point():
        total = None
        for p, (i, v) in enumerate(cut):
            gv, _ = ops.train_row_grad(i, table, step, g[p], None, None)
            offsets, entries = ops.train_csr(i, H)
            if binary:
                out = ops.train_unit_grad(offsets, entries, v, gv, x, g[p], logits, model.decoder.n_bits, step, None)
            else:
                out = ops.train_table_unit_grad(offsets, entries, v, gv, x, g[p])
            out = out + (ops.train_col_sum(g[p]),)
            total = out if total is None else tuple(a.add_(b) for a, b in zip(total, out))
        return total
    with torch.no_grad():
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(multik(), per_point()))
        got = alternate({"multik": multik, "per_point": per_point}, args.steps, args.warmup, args.repeats)
    line("backward", sae_type, B, got, "multik", "per_point", max_rel_diff=diff)


def bench_steps(sae_type, batches, tmp, args):
    sides = {}
    for name, top_k, mk in (("multik", K, KS), ("plain_k65", K, None), ("plain_k256", KS[-1], None)):
        t = Trainer(CONFIG, sae_type, False, True, model=make_model(sae_type, top_k), dataset_dir=tmp, save_dir=tmp, multi_topk=mk)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    for old in ("plain_k65", "plain_k256"):
        line("train_step", sae_type, batches[0].shape[0], got, "multik", old, steps=args.steps, repeats=args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_topk.py needs cuda:0 (MI355X); nothing is timed without it")
    assert (CONFIG["input_dim"], CONFIG["hidden_dim"]) == (D, H)
    batches = [torch.from_numpy(S.activations(5 + i, args.batch, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            model = make_model(sae_type)
            idx, val, cut, table, step = bench_decode(sae_type, model, batches[0], args)
            bench_backward(sae_type, model, batches[0], idx, val, cut, table, step, args)
            del model, idx, val, cut, table
            torch.cuda.empty_cache()
            bench_steps(sae_type, batches, tmp, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
