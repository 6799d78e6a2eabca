#!/usr/bin/env python3
"""Time the loop-side work of quantizedsae_amd.training (csrc/trainer.hip) against the same work written by hand from torch
ops, at the reference's config (B = 8192, D = 512, H = 32768) on one card:

* gather_rows against ``chunk[idx].float()`` on the device, and rows_nan_bitmap over the chunk, each with a device-to-device
  copy of the same byte count as the yardstick;
* trainer_loss against the torch autograd sequence of each recipe (mse_loss per level, the detached doubled residual
  chain, backward) on leaf reconstructions;
* the full Trainer step of baseline_sae, b_sae and q_sae -- ShuffledChunk's batch, forward_train, trainer_loss, the type's
  step sequence, optim.Adam -- against the same loop written by hand: torch indexing of the resident chunk,
  ``isnan().any()`` with its host read, F.mse_loss, backward, and the same optim.Adam.

Every comparison is timed in one process, its sides alternating; a window is `steps` iterations between two device events
and ends in a synchronise; the figures are the median and the range over `repeats` windows.  One JSON line per case.  A side
is "faster" only when its slowest window beats the other side's fastest; overlapping windows are reported as not
distinguishable.

    python tools/bench_trainer.py [--steps 10] [--warmup 3] [--repeats 5] [--types baseline_sae b_sae q_sae]
                                  [--hip-only]     (--hip-only: the Trainer's baseline_sae step alone, then the kernels
                                                    and copy yardsticks of trace_extras, for a kernel trace)
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_optim import alternate, faster, fmt  # noqa: E402
from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, ops, synthetic as S  # noqa: E402
from quantizedsae_amd.optim import Adam  # noqa: E402
from quantizedsae_amd.training import ShuffledChunk, Trainer, epoch_permutation, trainer_loss  # noqa: E402

D, H, B, N_BITS, ROWS = 512, 32768, 8192, 4, 131072
CONFIG = {"input_dim": D, "n_bits": N_BITS, "hidden_dim": H, "gamma": 1.5, "epochs": 1, "lr": 1e-4, "top_k": 32,
          "sparsity_lambda": 1.5e-3, "polarize_lambda": 1e-2, "batch_size": B}
RQ_WEIGHTS = (1.0, 2.5, 4.0, 8.0)
DEV = "cuda:0"
MIB = 1 << 20


def verdict(new, old):
    if faster(new, old):
        return "faster"
    if faster(old, new):
        return "slower"
    return "not distinguishable"


def copy_stat(nbytes, args):
    """-> (stat of a device-to-device copy of nbytes, bytes/s moved (read + write) at its median)"""
    src = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    stat = alternate({"copy": lambda: dst.copy_(src)}, args.steps, args.warmup, args.repeats)["copy"]
    return stat, 2 * nbytes / (stat[0] * 1e-3)


def with_rate(stat, traffic, crate):
    rate = traffic / (stat[0] * 1e-3)
    return dict(fmt(stat), traffic_MiB=round(traffic / MIB, 1), GBps=round(rate / 1e9, 1), of_copy_rate=round(rate / crate, 3))


def make_chunk():
    return torch.from_numpy(S.activations(5, ROWS, D)).to(torch.float16).to(DEV)


def bench_supply(args):
    chunk = make_chunk()
    torch.manual_seed(0)
    perm = epoch_permutation(ROWS).to(DEV)
    idx = perm[:B]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = alternate({"gather_rows": lambda: ops.gather_rows(chunk, idx, flag), "torch_index_float": lambda: chunk[idx].float()},
                    args.steps, args.warmup, args.repeats)
    traffic = B * D * 6 + B * 8
    cstat, crate = copy_stat(traffic // 2, args)
    out = {"what": "gather_rows", "B": B, "D": D, "rows": ROWS, "dtype": "fp16", "copy_of_the_same_bytes": fmt(cstat),
           "copy_GBps": round(crate / 1e9, 1), "gather_rows": with_rate(got["gather_rows"], traffic, crate),
           "torch_index_float": fmt(got["torch_index_float"]), "gather_rows_is": verdict(got["gather_rows"], got["torch_index_float"])}
    print(json.dumps(out), flush=True)
    got = alternate({"rows_nan_bitmap": lambda: ops.rows_nan_bitmap(chunk), "torch_isnan_any_rows": lambda: torch.isnan(chunk).any(dim=1)},
                    args.steps, args.warmup, args.repeats)
    traffic = ROWS * D * 2
    cstat, crate = copy_stat(traffic // 2, args)
    out = {"what": "rows_nan_bitmap", "rows": ROWS, "D": D, "dtype": "fp16", "copy_of_the_same_bytes": fmt(cstat),
           "copy_GBps": round(crate / 1e9, 1), "rows_nan_bitmap": with_rate(got["rows_nan_bitmap"], traffic, crate),
           "torch_isnan_any_rows": fmt(got["torch_isnan_any_rows"]),
           "rows_nan_bitmap_is": verdict(got["rows_nan_bitmap"], got["torch_isnan_any_rows"])}
    print(json.dumps(out), flush=True)


def torch_recipe(sae_type, outputs, batch, cfg):
    """loss_total of training/trainer.py:88-173"""
    if sae_type == "q_sae":
        latent_group, recon_groups = outputs
        return sum(0.5 * F.mse_loss(r, batch) for r in recon_groups) + sum(latent_group) * cfg["sparsity_lambda"]
    if sae_type == "rq_sae":
        latent_group, recon_group = outputs
        residual, loss = batch, 0
        for i, recon in enumerate(recon_group):
            loss = loss + 0.5 * F.mse_loss(recon, residual)
            residual = (residual - recon).detach() * 2
            if i < 4:
                loss = loss + latent_group[i] * cfg["sparsity_lambda"] * RQ_WEIGHTS[i]
        return loss
    if sae_type == "b_sae":
        return 0.5 * F.mse_loss(outputs[1], batch) + cfg["polarize_lambda"] * outputs[2]
    return F.mse_loss(outputs[1], batch)


def bench_loss(args):
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((B, D), device=DEV, generator=gen)
    for sae_type in ("baseline_sae", "b_sae", "q_sae", "rq_sae"):
        n = N_BITS if sae_type in ("q_sae", "rq_sae") else 1
        recons = [torch.randn((B, D), device=DEV, generator=gen).requires_grad_(True) for _ in range(n)]
        groups = [torch.rand((), device=DEV, generator=gen).requires_grad_(True) for _ in range(n)]
        pol = torch.rand((), device=DEV, generator=gen).requires_grad_(True)
        outputs = (groups, recons) if n > 1 or sae_type in ("q_sae", "rq_sae") else ((None, recons[0], pol) if sae_type == "b_sae" else (None, recons[0]))
        leaves = recons + groups + [pol]

        def clear():
            for t in leaves:
                t.grad = None

        def hip():
            clear()
            trainer_loss(sae_type, outputs, x, CONFIG)

        def hand():
            clear()
            torch_recipe(sae_type, outputs, x, CONFIG).backward()
        got = alternate({"trainer_loss": hip, "torch_autograd": hand}, args.steps, args.warmup, args.repeats)
        traffic = (1 + 2 * n) * B * D * 4
        cstat, crate = copy_stat(traffic // 2, args)
        out = {"what": "trainer_loss", "sae_type": sae_type, "levels": n, "B": B, "D": D, "copy_of_the_same_bytes": fmt(cstat),
               "copy_GBps": round(crate / 1e9, 1), "trainer_loss": with_rate(got["trainer_loss"], traffic, crate),
               "torch_autograd": fmt(got["torch_autograd"]), "trainer_loss_is": verdict(got["trainer_loss"], got["torch_autograd"])}
        print(json.dumps(out), flush=True)


def make_model(sae_type):
    if sae_type == "b_sae":
        m = BinarySAE(D, H, gamma=4.0, n_bits=N_BITS)
        sd = S.binary_sae_params(7, D, H, N_BITS, logit_std=1.0, dec_bias_std=0.1)
    elif sae_type == "q_sae":
        m = QuantizedMatryoshkaSAE(D, H, CONFIG["top_k"], CONFIG["gamma"], N_BITS)
        sd = S.matryoshka_sae_params(7, D, H, bias_std=0.1, enc_bias_sigmas=-2.5)
    else:
        m = BaselineSparseAutoencoder(D, H)
        sd = S.baseline_sae_params(7, D, H)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def bench_steps(sae_type, chunk_data, dataset_dir, args, hip_only=False):
    chunk = ShuffledChunk(chunk_data, B, DEV)
    torch.manual_seed(0)
    perm = epoch_permutation(ROWS).to(DEV)
    slices = [(s, s + B) for s in range(0, ROWS, B)]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    trainer = Trainer(CONFIG, sae_type, False, True, model=make_model(sae_type), dataset_dir=dataset_dir, save_dir=dataset_dir)
    opt_hip = Adam(trainer.model.parameters(), lr=CONFIG["lr"], model=trainer.model)
    pos = {"hip": 0, "hand": 0}

    def hip():
        s, e = slices[pos["hip"] % len(slices)]
        pos["hip"] += 1
        trainer._step(opt_hip, ops.gather_rows(chunk.data, perm[s:e], flag), False)

    sides = {"trainer_step": hip}
    if not hip_only:
        model = make_model(sae_type)
        opt = Adam(model.parameters(), lr=CONFIG["lr"], model=model)
        data = chunk.data

        def hand():
            s, e = slices[pos["hand"] % len(slices)]
            pos["hand"] += 1
            batch = data[perm[s:e]].float()
            if torch.isnan(batch).any():
                return
            outputs = model.forward_train(batch) if sae_type == "q_sae" else model.forward_train(batch, dense_latent=False)
            opt.zero_grad(set_to_none=True)
            torch_recipe(sae_type, outputs, batch, CONFIG).backward()
            if sae_type == "q_sae":
                model.decoder.apply_secant_grad()
            opt.step()
            if sae_type == "baseline_sae":
                model.normalize_decoder_weights()
        sides["hand_written_step"] = hand
    got = alternate(sides, args.steps, args.warmup, args.repeats)
    out = {"what": "train_step", "sae_type": sae_type, "B": B, "D": D, "H": H, "steps": args.steps, "repeats": args.repeats}
    out.update({w: fmt(s) for w, s in got.items()})
    if not hip_only:
        out["trainer_median_not_above_hand_written"] = bool(got["trainer_step"][0] <= got["hand_written_step"][0])
        out["trainer_step_is"] = verdict(got["trainer_step"], got["hand_written_step"])
    print(json.dumps(out), flush=True)


def trace_extras(runs=10):
    """For a kernel trace: the two one-pass kernels at the shapes of bench_supply / bench_loss, ten launches each, and as
    the yardstick an elementwise kernel (``torch.mul(src, 1.0, out=dst)`` on fp32: one read, one write) that moves the same
    number of bytes -- 24, 128, 48 and 144 MiB.  In the trace the sizes are told apart by the launch's grid."""
    chunk = make_chunk()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.manual_seed(0)
    idx = epoch_permutation(ROWS).to(DEV)[:B]
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((B, D), device=DEV, generator=gen)
    recons = [torch.randn((B, D), device=DEV, generator=gen) for _ in range(N_BITS)]
    for _ in range(runs):
        ops.gather_rows(chunk, idx, flag)
        ops.rows_nan_bitmap(chunk)
        ops.trainer_loss(x, recons[:1], 0, 1.0)
        ops.trainer_loss(x, recons, 0, 0.5)
        ops.trainer_loss(x, recons, 1, 0.5)
    for moved_mib in (24, 128, 48, 144):
        src = torch.zeros(moved_mib * MIB // 8, dtype=torch.float32, device=DEV)
        dst = torch.empty_like(src)
        for _ in range(runs):
            torch.mul(src, 1.0, out=dst)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", nargs="*", default=["baseline_sae", "b_sae", "q_sae"], choices=["baseline_sae", "b_sae", "q_sae"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="the Trainer's baseline_sae step alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trainer.py needs cuda:0 (MI355X); nothing is timed without it")
    with tempfile.TemporaryDirectory() as tmp:
        if args.hip_only:
            bench_steps("baseline_sae", make_chunk(), tmp, args, hip_only=True)
            trace_extras()
            return
        bench_supply(args)
        bench_loss(args)
        data = make_chunk()
        for sae_type in args.types:
            bench_steps(sae_type, data, tmp, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
