#!/usr/bin/env python3
"""Time the nested levels over ragged rows (csrc/nested_ragged.hip, include/qsae_nested_batch.h) at
H = 32768, D = 512, k = 65, cap K = 256, four default levels on one card, against the masked composition that was the only
route before: the nested ops of (idx, val_sel) at the full width K, with +0 behind every prefix.

* (a) decode: ``ops.decode_nested_ragged_*`` against ``ops.decode_nested_*`` of (idx, val_sel) at width K -- the soft table and,
  for b_sae, the packed dictionary; same bits on a finite dictionary, checked before anything is timed.
* (b) backward: ``train_row_grad_nested_ragged`` + ``train_csr_ragged`` + the nested unit-gradient op + ``train_col_sum(G[0])``
  against ``train_row_grad_nested`` at width K + a mask on gv + ``train_csr`` + the same unit-gradient op and column sum.
* (c) the whole step: ``Trainer._step`` with ``batch_topk=True, batch_topk_nested_bounds="default"`` against the step with
  ``batch_topk=True`` alone, for the cost of the levels.

The baselines are ops that exist without this feature.  The method is tools/bench_trainer.py's: one process, the sides
alternating; a window is ``steps`` iterations between two device events and ends in a synchronise; median / min / max over
``repeats`` windows.  A side is "faster" only when its slowest window beats the other side's fastest; overlapping windows are
"not distinguishable".  One JSON line per case.

    python tools/bench_nested_batch_topk.py [--batch 8192] [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae]
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
from quantizedsae_amd.sae import BinarySAE  # noqa: E402
from quantizedsae_amd.sae.topk import TopKCore  # noqa: E402
from quantizedsae_amd.training import BatchTopK, Trainer  # noqa: E402

CAP, BATCHES = 256, 4
BOUNDS = TopKCore.default_nested_bounds(H)


def line(what, sae_type, B, got, new, old, **more):
    out = {"what": what, "sae_type": sae_type, "B": B, "D": D, "H": H, "k": K, "cap": CAP, "bounds": BOUNDS, new: fmt(got[new]),
           old: fmt(got[old]), f"{new}_is": verdict(got[new], got[old]), "median_ratio": round(got[new][0] / got[old][0], 4)}
    out.update(more)
    print(json.dumps(out), flush=True)


def bench_ops(sae_type, model, x, args):
    B = x.shape[0]
    binary = isinstance(model, BinarySAE)
    with torch.no_grad():
        logits = model.decoder.weight.detach()
        table, step, _ = model._nested_train_decoder()
        bias = model.decoder.bias.detach()
        idx, val = model._select_cap(x, CAP, "bench")
        counts, val_sel, report = ops.batch_select(val, B * K)
        mask = (torch.arange(CAP, device=DEV)[None, :] < counts[:, None]).to(torch.float32)

        forms = [("table", lambda: ops.decode_nested_ragged_table(idx, val_sel, counts, table, step, bias, BOUNDS)[0],
                  lambda: ops.decode_nested_table(idx, val_sel, table, step, bias, BOUNDS))]
        if binary:
            dec = model.decoder
            packed = dec.packed()["packed"]
            forms.append(("packed",
                          lambda: ops.decode_nested_ragged_binary(idx, val_sel, counts, packed, D, dec.n_bits, step, bias, BOUNDS)[0],
                          lambda: ops.decode_nested_binary(idx, val_sel, packed, D, dec.n_bits, step, bias, BOUNDS)))
        for form, ragged, masked in forms:
            same_bits = bool(torch.equal(ragged(), masked()))
            got = alternate({"ragged": ragged, "masked": masked}, args.steps, args.warmup, args.repeats)
            line("nested_decode", sae_type, B, got, "ragged", "masked", form=form, same_bits=same_bits,
                 saturated_rows=int(report[1]), empty_rows=int(report[2]), max_count=int(counts.max()))

        g = [torch.from_numpy(S.activations(40 + l, B, D)).to(DEV) * (1.0 / (B * D)) for l in range(len(BOUNDS))]

        def unit(offsets, entries, gv, G):
            if binary:
                return ops.train_unit_grad_nested(offsets, entries, val_sel, gv, x, G, BOUNDS, logits, model.decoder.n_bits, step, None)
            return ops.train_table_unit_grad_nested(offsets, entries, val_sel, gv, x, G, BOUNDS)

        def ragged_backward():
            G, gv, _ = ops.train_row_grad_nested_ragged(idx, counts, table, step, g, BOUNDS, None, None)
            offsets, entries = ops.train_csr_ragged(idx, counts, H)
            return unit(offsets, entries, gv, G) + (ops.train_col_sum(G[0]),)

        def masked_backward():
            G, gv, _ = ops.train_row_grad_nested(idx, table, step, g, BOUNDS, None, None)
            offsets, entries = ops.train_csr(idx, H)
            return unit(offsets, entries, gv * mask, G) + (ops.train_col_sum(G[0]),)
        close = all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(ragged_backward(), masked_backward()))
        got = alternate({"ragged": ragged_backward, "masked": masked_backward}, args.steps, args.warmup, args.repeats)
        line("nested_backward", sae_type, B, got, "ragged", "masked", close=bool(close))


def bench_steps(sae_type, batches, tmp, args):
    sides = {}
    for name, bounds in (("batch_topk_nested", "default"), ("batch_topk", None)):
        t = Trainer(CONFIG, sae_type, False, True, model=make_model(sae_type), dataset_dir=tmp, save_dir=tmp, batch_topk=True,
                    batch_topk_cap=CAP, batch_topk_nested_bounds=bounds)
        assert t.nested_bounds == (BOUNDS if bounds else None)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    line("train_step", sae_type, batches[0].shape[0], got, "batch_topk_nested", "batch_topk", steps=args.steps, repeats=args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nested_batch_topk.py needs cuda:0 (MI355X); nothing is timed without it")
    assert (CONFIG["input_dim"], CONFIG["hidden_dim"]) == (D, H)
    batches = [torch.from_numpy(S.activations(5 + i, args.batch, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            model = make_model(sae_type)
            assert BatchTopK(model, cap=CAP).k == K
            bench_ops(sae_type, model, batches[0], args)
            del model
            torch.cuda.empty_cache()
            bench_steps(sae_type, batches, tmp, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
