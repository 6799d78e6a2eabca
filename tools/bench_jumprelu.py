#!/usr/bin/env python3
"""Time JumpReLU for the top-k SAEs (csrc/jumprelu.hip, quantizedsae_amd/training/jumprelu.py) at
H = 32768, D = 512, k = 65, cap K = 256 on one card, thresholds calibrated at k on the first batch.

* (a) select: ``ops.jump_select`` (both partitions, l0 and the report) against the torch composition -- gather the thresholds,
  mask ``val > theta[idx]``, a stable argsort of the mask and two gathers for the partition, a row sum for the counts.  Same
  lists, checked before anything is timed.
* (b) decode and backward on the compacted ragged lists (``decode_ragged_table``; ``train_row_grad_ragged`` +
  ``train_csr_ragged`` + the unit-gradient op + ``train_col_sum``) against the existing ops on the masked lists at width K
  (``decode_table_sparse``; ``train_row_grad`` + a mask on gv + ``train_csr`` + the same unit-gradient op).
* (c) the threshold-gradient chain on its own: ``train_row_grad_ragged`` on the band lists without dx, ``train_csr_ragged``,
  ``jump_threshold_grad``; at the paper's bandwidth and at a hundred times that.  Nothing to compare with: the line says what
  it costs.
* (d) the whole step: ``Trainer._step`` with ``jumprelu=True`` against ``batch_topk=True`` at the same cap.

The method is tools/bench_trainer.py's: one process, the sides alternating; a window is ``steps`` iterations between two
device events and ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its
slowest window beats the other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

    python tools/bench_jumprelu.py [--batch 8192] [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae]
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
from quantizedsae_amd.training import JumpReLU, Trainer  # noqa: E402

CAP, BATCHES, L0_COEF = 256, 4, 1e-3


def line(what, sae_type, B, got, new, old=None, **more):
    out = {"what": what, "sae_type": sae_type, "B": B, "D": D, "H": H, "k": K, "cap": CAP, new: fmt(got[new])}
    if old is not None:
        out.update({old: fmt(got[old]), f"{new}_is": verdict(got[new], got[old]),
                    "median_ratio": round(got[new][0] / got[old][0], 4)})
    out.update(more)
    print(json.dumps(out), flush=True)


def torch_select(idx, val, theta):
    """the composition: mask, stable partition by argsort, counts"""
    mask = val > theta[idx.long()]
    order = torch.argsort((~mask).to(torch.int8), dim=1, stable=True)
    idx_sel = torch.gather(idx, 1, order)
    val_sel = torch.gather(val * mask, 1, order)
    return idx_sel, val_sel, mask.sum(1, dtype=torch.int32), mask


def bench_ops(sae_type, model, x, args):
    B = x.shape[0]
    binary = isinstance(model, BinarySAE)
    with torch.no_grad():
        jr = JumpReLU(model, cap=CAP)
        jr.calibrate(x, K)
        theta = jr.thresholds()
        logits = model.decoder.weight.detach()
        table, step, _ = model._nested_train_decoder()
        bias = model.decoder.bias.detach()
        idx, val = model._select_cap(x, CAP, "bench")
        eps = jr.bandwidth
        idx_sel, val_sel, counts, idx_band, counts_band, l0, report = ops.jump_select(idx, val, theta, eps)
        t_idx, t_val, t_counts, mask = torch_select(idx, val, theta)
        same = bool(torch.equal(idx_sel, t_idx) and torch.equal(val_sel, t_val) and torch.equal(counts, t_counts))
        got = alternate({"jump_select": lambda: ops.jump_select(idx, val, theta, eps),
                         "torch_mask_argsort": lambda: torch_select(idx, val, theta)}, args.steps, args.warmup, args.repeats)
        rep = report.tolist()
        line("select", sae_type, B, got, "jump_select", "torch_mask_argsort", same_lists=same, l0=float(l0), band_entries=rep[1],
             saturated_rows=rep[2], empty_rows=rep[3], uncertified_rows=rep[4], max_count=int(counts.max()))

        masked = val * mask
        ragged = lambda: ops.decode_ragged_table(idx_sel, val_sel, counts, table, step, bias)     # noqa: E731
        plain = lambda: ops.decode_table_sparse(idx, masked, table, step, bias)                    # noqa: E731
        got = alternate({"ragged": ragged, "masked": plain}, args.steps, args.warmup, args.repeats)
        line("decode", sae_type, B, got, "ragged", "masked", form="table", same_bits=bool(torch.equal(ragged(), plain())))

        g = torch.from_numpy(S.activations(40, B, D)).to(DEV) * (1.0 / (B * D))

        def unit(offsets, entries, v, gv):
            if binary:
                return ops.train_unit_grad(offsets, entries, v, gv, x, g, logits, model.decoder.n_bits, step, None)
            return ops.train_table_unit_grad(offsets, entries, v, gv, x, g)

        def ragged_backward():
            gv, _ = ops.train_row_grad_ragged(idx_sel, counts, table, step, g, None, None)
            offsets, entries = ops.train_csr_ragged(idx_sel, counts, H)
            return unit(offsets, entries, val_sel, gv) + (ops.train_col_sum(g),)

        def masked_backward():
            gv, _ = ops.train_row_grad(idx, table, step, g, None, None)
            offsets, entries = ops.train_csr(idx, H)
            return unit(offsets, entries, masked, gv * mask) + (ops.train_col_sum(g),)
        close = all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(ragged_backward(), masked_backward()))
        got = alternate({"ragged": ragged_backward, "masked": masked_backward}, args.steps, args.warmup, args.repeats)
        line("backward", sae_type, B, got, "ragged", "masked", close=bool(close))

        g_l0 = torch.full((1,), L0_COEF, device=DEV)
        for width in (eps, 100 * eps):
            _, _, _, ib, cb, _, rb = ops.jump_select(idx, val, theta, width)

            def chain(ib=ib, cb=cb, width=width):
                gv, _ = ops.train_row_grad_ragged(ib, cb, table, step, g, None, None)
                offsets, entries = ops.train_csr_ragged(ib, cb, H)
                return ops.jump_threshold_grad(offsets, entries, gv, theta, g_l0, B, CAP, width)
            got = alternate({"threshold_grad_chain": chain}, args.steps, args.warmup, args.repeats)
            line("threshold_gradient", sae_type, B, got, "threshold_grad_chain", bandwidth=width, band_entries=int(rb[1]))


def bench_steps(sae_type, batches, tmp, args):
    sides = {}
    for name, kw in (("jumprelu", dict(jumprelu=True, jumprelu_l0_coef=L0_COEF, jumprelu_cap=CAP, jumprelu_init="calibrate")),
                     ("batch_topk", dict(batch_topk=True, batch_topk_cap=CAP))):
        t = Trainer(CONFIG, sae_type, False, True, model=make_model(sae_type), dataset_dir=tmp, save_dir=tmp, **kw)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        if t.jumprelu is not None:
            opt.add_param_group({"params": [t.jumprelu.log_threshold]})
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    line("train_step", sae_type, batches[0].shape[0], got, "jumprelu", "batch_topk", steps=args.steps, repeats=args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jumprelu.py needs cuda:0 (MI355X); nothing is timed without it")
    assert (CONFIG["input_dim"], CONFIG["hidden_dim"]) == (D, H)
    batches = [torch.from_numpy(S.activations(5 + i, args.batch, D)).to(DEV) for i in range(BATCHES)]
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            model = make_model(sae_type)
            bench_ops(sae_type, model, batches[0], args)
            del model
            torch.cuda.empty_cache()
            bench_steps(sae_type, batches, tmp, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
