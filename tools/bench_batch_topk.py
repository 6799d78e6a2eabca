#!/usr/bin/env python3
"""Time BatchTopK for the top-k SAEs (csrc/batch_topk.hip, csrc/batch_topk_decode.hip, quantizedsae_amd/training/batch_topk.py;
DESIGN.md section 4.32) at H = 32768, D = 512, k = 65, cap K = 256 on one card, against the composition the library offered
before: select per row at K, let torch pick the ``B k`` largest of the flattened ``[B, K]`` values and mask the lists, then
decode and differentiate the masked lists at their full width K.

* (a) select: ``ops.batch_select`` against ``torch.topk`` over the flattened values plus the scatter of a mask.  (torch breaks
  ties as it likes; on distinct values both sides select the same set, which is checked before anything is timed.)
* (b) decode: ``ops.decode_ragged_*`` against ``ops.decode_*_sparse`` of the masked lists -- the soft table and the packed
  dictionary; same bits.
* (c) backward: ``train_row_grad_ragged`` + ``train_csr_ragged`` + the unit-gradient op + ``train_col_sum`` against
  ``train_row_grad`` + a mask on gv + ``train_csr`` + the same unit-gradient op + ``train_col_sum`` at width K.
* (d) forward and backward of one batch from the ops: selection at K, (a), (b) and (c) on each side.
* (e) the whole step: ``Trainer._step`` with ``batch_topk=True`` against the plain top-k step at k, for context; and the
  encoder's selection at K = 256 against k = 65 as a line of its own, because that cost is inherent to a cap.

The method is tools/bench_trainer.py's: one process, the sides alternating; a window is ``steps`` iterations between two
device events and ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its
slowest window beats the other side's fastest; overlapping windows are "not distinguishable".  One JSON line per case.

With --profile one ``rocprofv3 --kernel-trace --stats`` run of the new ops alone (--ops-only) follows in a fresh child process.

    python tools/bench_batch_topk.py [--batch 8192] [--steps 10] [--warmup 3] [--repeats 5] [--types b_sae baseline_sae] [--profile]
"""
from __future__ import annotations

import argparse
import csv
import json
import shutil
import subprocess
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
from quantizedsae_amd.training import BatchTopK, Trainer  # noqa: E402

CAP, BATCHES = 256, 4


def line(what, sae_type, B, got, new, old, **more):
    out = {"what": what, "sae_type": sae_type, "B": B, "D": D, "H": H, "k": K, "cap": CAP, new: fmt(got[new]),
           old: fmt(got[old]), f"{new}_is": verdict(got[new], got[old]), "median_ratio": round(got[new][0] / got[old][0], 4)}
    out.update(more)
    print(json.dumps(out), flush=True)


def torch_select(val, n):
    """the composition: the n largest of the flattened values, as a mask on the lists"""
    top = torch.topk(val.reshape(-1), n, sorted=False)
    mask = torch.zeros(val.numel(), dtype=val.dtype, device=val.device)
    mask[top.indices] = 1.0
    mask = mask.view_as(val)
    return mask, val * mask


def bench_ops(sae_type, model, x, args):
    B = x.shape[0]
    binary = isinstance(model, BinarySAE)
    with torch.no_grad():
        W, logits = model.encoder.linear.weight.detach(), model.decoder.weight.detach()
        table, step, _ = model._nested_train_decoder()
        bias = model.decoder.bias.detach()
        select_cap = lambda: model._select_cap(x, CAP, "bench")   # noqa: E731
        idx, val = select_cap()
        n = B * K
        counts, val_sel, report = ops.batch_select(val, n)
        mask, masked = torch_select(val, n)
        same_set = bool(torch.equal(masked, val_sel))
        got = alternate({"batch_select": lambda: ops.batch_select(val, n), "torch_topk_mask": lambda: torch_select(val, n)},
                        args.steps, args.warmup, args.repeats)
        line("select", sae_type, B, got, "batch_select", "torch_topk_mask", same_set=same_set,
             saturated_rows=int(report[1]), empty_rows=int(report[2]), max_count=int(counts.max()))

        forms = [("table", lambda: ops.decode_ragged_table(idx, val_sel, counts, table, step, bias),
                  lambda: ops.decode_table_sparse(idx, masked, table, step, bias))]
        if binary:
            dec = model.decoder
            packed = dec.packed()["packed"]
            forms.append(("packed", lambda: ops.decode_ragged_binary(idx, val_sel, counts, packed, D, dec.n_bits, step, bias),
                          lambda: ops.decode_binary_sparse(idx, masked, packed, D, dec.n_bits, step, bias)))
        for form, ragged, plain in forms:
            got = alternate({"ragged": ragged, "masked": plain}, args.steps, args.warmup, args.repeats)
            line("decode", sae_type, B, got, "ragged", "masked", form=form, same_bits=bool(torch.equal(ragged(), plain())))

        g = torch.from_numpy(S.activations(40, B, D)).to(DEV) * (1.0 / (B * D))

        def unit(offsets, entries, v, gv):
            if binary:
                return ops.train_unit_grad(offsets, entries, v, gv, x, g, logits, model.decoder.n_bits, step, None)
            return ops.train_table_unit_grad(offsets, entries, v, gv, x, g)

        def ragged_backward(counts=counts, val_sel=val_sel):
            gv, _ = ops.train_row_grad_ragged(idx, counts, table, step, g, None, None)
            offsets, entries = ops.train_csr_ragged(idx, counts, H)
            return unit(offsets, entries, val_sel, gv) + (ops.train_col_sum(g),)

        def masked_backward(mask=mask, masked=masked):
            gv, _ = ops.train_row_grad(idx, table, step, g, None, None)
            offsets, entries = ops.train_csr(idx, H)
            return unit(offsets, entries, masked, gv * mask) + (ops.train_col_sum(g),)
        close = all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(ragged_backward(), masked_backward()))
        got = alternate({"ragged": ragged_backward, "masked": masked_backward}, args.steps, args.warmup, args.repeats)
        line("backward", sae_type, B, got, "ragged", "masked", close=bool(close))

        def ragged_all():
            i, v = select_cap()
            c, vs, _ = ops.batch_select(v, n)
            ops.decode_ragged_table(i, vs, c, table, step, bias)
            return ragged_backward(c, vs)

        def masked_all():
            i, v = select_cap()
            m, mv = torch_select(v, n)
            ops.decode_table_sparse(i, mv, table, step, bias)
            return masked_backward(m, mv)
        got = alternate({"ragged": ragged_all, "masked": masked_all}, args.steps, args.warmup, args.repeats)
        line("forward_backward_ops", sae_type, B, got, "ragged", "masked")

        k_own = lambda: model._nested_select(x, False)        # noqa: E731
        got = alternate({"select_at_cap": select_cap, "select_at_k": k_own}, args.steps, args.warmup, args.repeats)
        line("encoder_selection", sae_type, B, got, "select_at_cap", "select_at_k")


def ops_only(x, steps: int = 5) -> None:
    """what the kernel trace runs: the selection at the cap, batch_select, the ragged table decode and the ragged backward of
    b_sae, ``steps`` times"""
    model = make_model("b_sae")
    with torch.no_grad():
        table, step, _ = model._nested_train_decoder()
        bias, logits = model.decoder.bias.detach(), model.decoder.weight.detach()
        g = torch.from_numpy(S.activations(40, x.shape[0], D)).to(DEV) * (1.0 / (x.shape[0] * D))
        for _ in range(steps):
            idx, val = model._select_cap(x, CAP, "bench")
            counts, val_sel, _ = ops.batch_select(val, x.shape[0] * K)
            ops.decode_ragged_table(idx, val_sel, counts, table, step, bias)
            gv, _ = ops.train_row_grad_ragged(idx, counts, table, step, g, None, None)
            offsets, entries = ops.train_csr_ragged(idx, counts, H)
            ops.train_unit_grad(offsets, entries, val_sel, gv, x, g, logits, model.decoder.n_bits, step, None)
        torch.cuda.synchronize()


def kernel_table(batch: int) -> None:
    """One rocprofv3 --kernel-trace --stats run of ops_only in a fresh child process; prints its kernel table."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        print("== rocprofv3 not found: no kernel table")
        return
    with tempfile.TemporaryDirectory(prefix="qsae_batch_topk_prof_") as tmp:
        child = [sys.executable, str(Path(__file__).resolve()), "--ops-only", "--batch", str(batch)]
        print(f"== rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_batch_topk.py --ops-only --batch {batch}")
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + child,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(f"   rocprofv3 exited with {r.returncode}: {r.stderr[-400:]}")
            return
        files = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not files:
            print("   no kernel_stats.csv was written")
            return
        with open(files[0], newline="") as f:
            rows = list(csv.DictReader(f))
    print("   (5 steps of b_sae; kernels above 0.1 % of the GPU time; name, calls, average us, percentage)")
    for row in rows:
        pct = float(row.get("Percentage", 0) or 0)
        if pct >= 0.1:
            print(f"   {row.get('Name', '')[:90]:90s} {row.get('Calls', '')!s:>5} {float(row.get('AverageNs', 0) or 0) / 1e3:10.1f} {pct:6.2f}", flush=True)


def bench_steps(sae_type, batches, tmp, args):
    sides = {}
    for name, on in (("batch_topk", True), ("plain_topk", False)):
        t = Trainer(CONFIG, sae_type, False, True, model=make_model(sae_type), dataset_dir=tmp, save_dir=tmp, batch_topk=on,
                    batch_topk_cap=CAP if on else None)
        opt = Adam(t.model.parameters(), lr=CONFIG["lr"], model=t.model)
        pos = [0]

        def step(t=t, opt=opt, pos=pos):
            t._step(opt, batches[pos[0] % len(batches)], False)
            pos[0] += 1
        sides[name] = step
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    line("train_step", sae_type, batches[0].shape[0], got, "batch_topk", "plain_topk", steps=args.steps, repeats=args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["b_sae", "baseline_sae"], choices=["b_sae", "baseline_sae"])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ops-only", action="store_true", help="the new ops alone, five times (what the kernel trace runs)")
    ap.add_argument("--profile", action="store_true", help="after the timings: one rocprofv3 --kernel-trace --stats run of --ops-only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_topk.py needs cuda:0 (MI355X); nothing is timed without it")
    assert (CONFIG["input_dim"], CONFIG["hidden_dim"]) == (D, H)
    batches = [torch.from_numpy(S.activations(5 + i, args.batch, D)).to(DEV) for i in range(BATCHES)]
    if args.ops_only:
        ops_only(batches[0])
        return
    with tempfile.TemporaryDirectory() as tmp:
        for sae_type in args.types:
            model = make_model(sae_type)
            assert BatchTopK(model, cap=CAP).k == K
            bench_ops(sae_type, model, batches[0], args)
            del model
            torch.cuda.empty_cache()
            bench_steps(sae_type, batches, tmp, args)
            torch.cuda.empty_cache()
    if args.profile:
        del batches
        torch.cuda.empty_cache()
        kernel_table(args.batch)


if __name__ == "__main__":
    main()
