#!/usr/bin/env python3
"""Time one BinaryLatentSAE training step on the GPU -- forward_train, F.mse_loss, backward, Adam.step (the bl_sae of
training/trainer.py) -- against the same step in eager torch on the same card: the reference's op sequence (sigmoid encoder,
straight-through binary latent, dense decoder, autograd) restated here with plain torch ops.  Also forward_train, backward and
forward() alone.  The method is that of tools/bench_train_ternary.py.

Every comparison is timed in one process, its sides alternating; a window is `steps` iterations between two device events
and ends in a synchronise; the figures are the median and the range over `repeats` windows.  One JSON line per case.  Then
one `rocprofv3 --kernel-trace --stats` run of the HIP step alone in a fresh child process (--no-profile: skipped), whose kernel
table follows.  Everything printed is also written to --out (default profiles/train_blatent.txt).

    python tools/bench_train_blatent.py [--batches 4096 8192] [--steps 10] [--warmup 2] [--repeats 5] [--no-profile] [--hip-only]
"""
from __future__ import annotations

import argparse
import csv
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from quantizedsae_amd.sae import BinaryLatentSAE  # noqa: E402
import train_blatent_util as U  # noqa: E402

D, H = 512, 32768
DEV = "cuda:0"
LR = 1e-3
PROFILE_ARGS = ["--hip-only", "--batches", "8192", "--steps", "4", "--warmup", "1", "--repeats", "1"]


def eager_step(params, opt, x):
    """The reference's step restated in eager torch (sae/binary_latent.py:19-27)."""
    W_e, b_e, W_d, b_d = params
    latent = torch.sigmoid(F.linear(x, W_e, b_e))
    with torch.no_grad():
        binary = (latent >= 0.5).float()
    recon = F.linear(latent + (binary - latent).detach(), W_d, b_d)
    loss = F.mse_loss(recon, x)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def hip_step(model, opt, x):
    _, recon = model.forward_train(x)
    loss = F.mse_loss(recon, x)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def window_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def alternate(sides: dict, steps, warmup, repeats):
    """{name: fn} -> {name: (median ms, min ms, max ms)}: every side warmed up, then `repeats` rounds of one window each."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            got[name].append(window_ms(fn, steps))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def fmt(stat):
    return {"median_ms": round(stat[0], 4), "min_ms": round(stat[1], 4), "max_ms": round(stat[2], 4)}


def backward_alone_ms(model, x, n):
    out = []
    for _ in range(n):
        model.zero_grad(set_to_none=True)
        _, recon = model.forward_train(x)
        loss = F.mse_loss(recon, x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def make_model(sd):
    m = BinaryLatentSAE(D, H)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def kernel_table(say) -> None:
    """One rocprofv3 --kernel-trace --stats run of the HIP step alone, in a fresh child process; prints its kernel table."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        say("== rocprofv3 not found: no kernel table")
        return
    with tempfile.TemporaryDirectory(prefix="qsae_blatent_prof_") as tmp:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               str(Path(__file__).resolve()), "--no-profile", "--out", str(Path(tmp) / "child.txt")] + PROFILE_ARGS
        say("== rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_train_blatent.py --no-profile "
            + " ".join(PROFILE_ARGS))
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            say(f"   rocprofv3 exited with {r.returncode}: {r.stderr[-400:]}")
            return
        files = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not files:
            say("   no kernel_stats.csv was written")
            return
        with open(files[0], newline="") as f:
            rows = list(csv.DictReader(f))
    say("   (5 steps at B = 8192; kernels above 0.3 % of the GPU time)")
    for row in rows:
        pct = float(row.get("Percentage", 0) or 0)
        if pct < 0.3:
            continue
        avg, lo, hi = (float(row[k]) / 1e3 for k in ("AverageNs", "MinNs", "MaxNs"))
        say(f"{pct:6.2f} %  calls {int(row['Calls']):4d}  avg {avg:9.1f} us  min {lo:9.1f}  max {hi:9.1f}  {row['Name'][:150]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="the HIP step alone (what the kernel trace runs)")
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "train_blatent.txt")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_blatent.py needs cuda:0 (MI355X); nothing is timed without it")
    lines = []

    def say(text: str) -> None:
        print(text, flush=True)
        lines.append(text)

    say(f"BinaryLatentSAE training step on one MI355X (D = {D}, H = {H}; forward_train, F.mse_loss, backward, torch.optim.Adam)")
    say("tools/bench_train_blatent.py: one process, sides alternating, windows of `steps` steps each ending in a synchronise;")
    say("median / min / max ms.  eager = the reference's op sequence restated in plain torch (autograd) on the same card.")
    say("")
    say("== python tools/bench_train_blatent.py " + " ".join(sys.argv[1:]))
    sd = U.blatent_params(7, D, H)
    for B in args.batches:
        x = torch.from_numpy(U.S.activations(8, B, D)).to(DEV)
        out = {"what": "step", "B": B, "D": D, "H": H, "steps": args.steps, "repeats": args.repeats}
        model = make_model(sd)
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        sides = {}
        if not args.hip_only:
            params = [model.state_dict()[k].detach().clone().requires_grad_(True) for k in U.PARAM_KEYS]
            ropt = torch.optim.Adam(params, lr=LR)
            sides["eager_reference_step"] = lambda: eager_step(params, ropt, x)
        sides["hip_step"] = lambda: hip_step(model, opt, x)
        for key, stat in alternate(sides, args.steps, args.warmup, args.repeats).items():
            out[key] = fmt(stat)
        if not args.hip_only:
            out["hip_forward_train"] = fmt(alternate({"f": lambda: model.forward_train(x)}, args.steps, args.warmup,
                                                     args.repeats)["f"])
            out["hip_backward"] = fmt(backward_alone_ms(model, x, args.steps))
            with torch.no_grad():
                out["hip_forward"] = fmt(alternate({"f": lambda: model(x)}, args.steps, args.warmup, args.repeats)["f"])
            out["speedup"] = round(out["eager_reference_step"]["median_ms"] / out["hip_step"]["median_ms"], 2)
        say(json.dumps(out))
        del model, opt, sides
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if not args.no_profile:
        say("")
        kernel_table(say)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
