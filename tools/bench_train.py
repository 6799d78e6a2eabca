#!/usr/bin/env python3
"""Time one BinarySAE training step on the GPU: forward_train + backward + Adam, against the reference's op sequence
(sae/binary.py:24-47, 91-103 and the b_sae branch of trainer.py:144-153) restated with autograd in eager torch on the same
card.  Prints one JSON line per configuration.

    python tools/bench_train.py [--batches 4096 8192] [--steps 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from quantizedsae_amd import BinarySAE, synthetic as S  # noqa: E402

D, H, N_BITS, GAMMA, LAM = 512, 32768, 4, 4.0, 1e-2


def eager_reference_step(params, x, k, step):
    """The reference's forward and loss in eager torch (dense [B, H] latent and mask, dense GEMMs)."""
    W, b, logits, bd = params
    latent = F.linear(x, W, b)
    _, ids = latent.topk(k, dim=1)
    mask = torch.zeros_like(latent)
    mask.scatter_(1, ids, 1.0)
    sparse = latent * mask
    p = torch.sigmoid(logits).view(H, D, N_BITS)
    bw = 2.0 ** torch.arange(N_BITS, device=x.device, dtype=p.dtype)
    bwf = bw.clone()
    bwf[-1] *= -1
    ints = (p * bwf).sum(-1)
    recon = step * sparse.matmul(ints) + bd
    pol = (p * (1 - p) * bw).mean()
    return 0.5 * F.mse_loss(recon, x) + LAM * pol


def time_steps(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    sd = S.binary_sae_params(7, D, H, N_BITS, logit_std=1.0, dec_bias_std=0.1)
    for B in args.batches:
        x = torch.from_numpy(S.activations(8, B, D)).to(dev)
        out = {"B": B, "D": D, "H": H, "n_bits": N_BITS}
        for dense in (True, False):
            model = BinarySAE(D, H, gamma=GAMMA, n_bits=N_BITS)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            model = model.to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)

            def step():
                opt.zero_grad(set_to_none=True)
                latent, recon, pol = model.forward_train(x, dense_latent=dense)
                (0.5 * F.mse_loss(recon, x) + LAM * pol).backward()
                opt.step()

            out[f"hip_step_ms_dense{int(dense)}"] = round(time_steps(step, args.steps, args.warmup), 3)

            def fwd_bwd():
                latent, recon, pol = model.forward_train(x, dense_latent=dense)
                loss = 0.5 * F.mse_loss(recon, x) + LAM * pol
                return loss

            # forward alone and backward alone (events around loss.backward())
            fw = time_steps(lambda: fwd_bwd(), args.steps, args.warmup)
            bw_ms = []
            for _ in range(args.steps):
                loss = fwd_bwd()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss.backward()
                e1.record()
                torch.cuda.synchronize()
                bw_ms.append(e0.elapsed_time(e1))
            out[f"hip_forward_train_ms_dense{int(dense)}"] = round(fw, 3)
            out[f"hip_backward_ms_dense{int(dense)}"] = round(sorted(bw_ms)[len(bw_ms) // 2], 3)
            del model, opt
        model = BinarySAE(D, H, gamma=GAMMA, n_bits=N_BITS)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model = model.to(dev)
        model.decoder.decode_mode = "soft"
        with torch.no_grad():
            out["hip_forward_soft_ms"] = round(time_steps(lambda: model(x), args.steps, args.warmup), 3)
        params = [torch.from_numpy(sd[k]).to(dev).requires_grad_(True)
                  for k in ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.bias")]
        ropt = torch.optim.Adam(params, lr=1e-4)
        k = model.top_k

        def ref_step():
            ropt.zero_grad(set_to_none=True)
            eager_reference_step(params, x, k, GAMMA / 2 ** (N_BITS - 1)).backward()
            ropt.step()

        out["eager_reference_step_ms"] = round(time_steps(ref_step, args.steps, args.warmup), 3)
        out["speedup_dense1"] = round(out["eager_reference_step_ms"] / out["hip_step_ms_dense1"], 2)
        out["speedup_dense0"] = round(out["eager_reference_step_ms"] / out["hip_step_ms_dense0"], 2)
        print(json.dumps(out), flush=True)
        del params, ropt, model


if __name__ == "__main__":
    main()
