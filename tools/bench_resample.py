#!/usr/bin/env python3
"""Time the resampling step of quantizedsae_amd.training.resample (csrc/resample.hip) against the same procedure written in
torch ops inside this tool, at the reference's config (B = 8192, D = 512, H = 32768) with n = 1, 1024 and 16384 dead units,
for both top-k models, and a non-resampling ``Trainer._step`` with ``resample_every`` on and off.

The torch side does what a hand-written trainer does: per-row squared loss, ``cumsum`` and ``searchsorted`` for the draw, a
scatter-min for the owner rule, norms, indexed writes of the encoder rows, the decoder columns or logit rows and the Adam
moments.  Its sums are torch's, not in the fixed order of the kernels: the two sides do the same work, not the same bits.
The reconstruction is computed once and handed to both sides, so the forward is not timed.

Every comparison is timed in one process, its sides alternating; a window is `steps` iterations between two device events
and ends in a synchronise; the figures are the median and the range over `repeats` windows.  One JSON line per case.  A side
is "faster" only when its slowest window beats the other side's fastest; overlapping windows are reported as not
distinguishable.

    python tools/bench_resample.py [--steps 10] [--warmup 3] [--repeats 5]
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

from bench_optim import alternate, fmt  # noqa: E402
from bench_trainer import CONFIG, DEV, make_chunk, verdict  # noqa: E402
from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, synthetic as S  # noqa: E402
from quantizedsae_amd.optim import Adam  # noqa: E402
from quantizedsae_amd.training import ShuffledChunk, Trainer, resample_dead  # noqa: E402

D, H, B, N_BITS = 512, 32768, 8192, 8
DEAD = (1, 1024, 16384)


def make_model(kind):
    if kind == "b_sae":
        m = BinarySAE(D, H, 4.0, N_BITS)
        sd = S.binary_sae_params(7, D, H, N_BITS, logit_std=1.0, dec_bias_std=0.1)
    else:
        m = BaselineSparseAutoencoder(D, H)
        sd = S.baseline_sae_params(7, D, H, bias_std=0.1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


@torch.no_grad()
def torch_resample(model, dead, x, recon, u, moments, last, rows_seen, scale=0.2):
    """The procedure of resample_dead in torch ops (double precision where the kernels use it)"""
    binary = isinstance(model, BinarySAE)
    lin, dec = model.encoder.linear, model.decoder
    W, b, Wd = lin.weight, lin.bias, dec.weight
    Hn, n = W.shape[0], dead.numel()
    dead = dead.long()
    e = (x - recon).double().pow(2).sum(1)
    w = torch.where(torch.isfinite(e), e * e, torch.zeros_like(e))
    cdf = torch.cumsum(w, 0)
    total = cdf[-1]
    r = torch.searchsorted(cdf, u * total, right=True).clamp_(max=x.shape[0] - 1)
    owner = torch.full((x.shape[0],), n, dtype=torch.long, device=x.device)
    owner.scatter_reduce_(0, r, torch.arange(n, device=x.device), "amin")
    alive = torch.ones(Hn, dtype=torch.bool, device=x.device)
    alive[dead] = False
    if not bool(alive.any()):
        alive[:] = True
    norm_mean = W.double().pow(2).sum(1).sqrt()[alive].mean()
    v = x[r] - dec.bias
    s = v.double().pow(2).sum(1)
    ok = (owner[r] == torch.arange(n, device=x.device)) & (s > 0) & torch.isfinite(s) & (total > 0)
    h, v = dead[ok], v[ok].double()
    nrm = s[ok].sqrt()[:, None]
    W[h] = (v * (scale * norm_mean / nrm)).float()
    b[h] = 0.0
    if binary:
        nb = dec.n_bits
        L = Wd.abs().double().mean(1)[alive].mean().float()
        qmax = 2 ** (nb - 1) - 1
        q = torch.round(v * (max(qmax, 1) / v.abs().amax(1, keepdim=True))).clamp_(-(2 ** (nb - 1)), qmax).long()
        bits = ((q[:, :, None] & (2 ** nb - 1)) >> torch.arange(nb, device=x.device)) & 1
        Wd[h] = torch.where(bits.reshape(h.numel(), -1) == 1, L, -L)
    else:
        Wd[:, h] = (v / nrm).float().t()
    for i, m in enumerate(moments):
        if m is None:
            continue
        if i >= 4 and not binary:
            m[:, h] = 0.0
        else:
            m[h] = 0.0
    if last is not None:
        last[h] = rows_seen
    model.invalidate_packed()
    return ok.sum()


def bench_step(args):
    for kind in ("baseline_sae", "b_sae"):
        model = make_model(kind)
        lin, dec = model.encoder.linear, model.decoder
        x = torch.from_numpy(S.activations(11, B, D)).to(DEV)
        with torch.no_grad():
            recon = model.forward_compact(x)[2].clone()
        opt = Adam(model.parameters(), lr=1e-4, model=model)
        for p in (lin.weight, lin.bias, dec.weight):
            opt._state_of(p)
        moments = [opt.state[p][k] for p in (lin.weight, lin.bias, dec.weight) for k in ("exp_avg", "exp_avg_sq")]
        last = torch.zeros(H, dtype=torch.int64, device=DEV)

        class Tracker:
            rows_seen = B
        Tracker.last = last
        for n in DEAD:
            gen = torch.Generator(device=DEV)
            gen.manual_seed(3)
            dead = torch.sort(torch.randperm(H, device=DEV, generator=gen)[:n]).values.to(torch.int32)
            u = torch.rand(n, dtype=torch.float64, device=DEV, generator=gen)
            sides = {"hip": lambda: resample_dead(model, dead, x, optimizer=opt, activity=Tracker, u=u, recon=recon),
                     "torch": lambda: torch_resample(model, dead, x, recon, u, moments, last, B)}
            stat = alternate(sides, args.steps, args.warmup, args.repeats)
            print(json.dumps({"case": "resample_dead", "sae_type": kind, "B": B, "D": D, "H": H, "dead": n, "hip": fmt(stat["hip"]),
                              "torch": fmt(stat["torch"]), "hip_vs_torch": verdict(stat["hip"], stat["torch"]),
                              "ratio_of_medians": round(stat["torch"][0] / stat["hip"][0], 2)}), flush=True)
        del model, opt, moments


def bench_trainer(args):
    """A step that is not a resampling step, with the option on and off: the option must cost it nothing"""
    chunk = make_chunk()
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("baseline_sae", "b_sae"):
            trainers = {}
            for name, every in (("off", None), ("on", 10 ** 9)):
                t = Trainer(dict(CONFIG, n_bits=N_BITS), kind, False, True, model=make_model(kind), dataset_dir=tmp, save_dir=tmp,
                            log_fn=lambda m: None, activity_window=10 ** 6, resample_every=every)
                t._opt = Adam(t.model.parameters(), lr=1e-4, model=t.model)
                trainers[name] = t
            torch.manual_seed(0)
            batch = next(iter(ShuffledChunk(chunk, B, torch.device(DEV)).epoch()))[1]

            def step(t):
                t._watch_due = False
                t._step(t._opt, batch, False)
                if t.resample_every is not None and 1 % t.resample_every == 0:      # batch_idx = 1: what one_epoch evaluates
                    t._resample(t._opt, batch)
            stat = alternate({name: (lambda t=t: step(t)) for name, t in trainers.items()}, args.steps, args.warmup, args.repeats)
            print(json.dumps({"case": "trainer_step_without_resampling", "sae_type": kind, "on": fmt(stat["on"]), "off": fmt(stat["off"]),
                              "on_vs_off": verdict(stat["on"], stat["off"])}), flush=True)
            del trainers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    bench_step(args)
    bench_trainer(args)


if __name__ == "__main__":
    main()
