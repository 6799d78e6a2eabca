#!/usr/bin/env python3
"""Time the sparsity-fidelity curve (csrc/sparsity_curve.hip, quantizedsae_amd/inference/sparsity_curve.py; DESIGN.md section
4.30) at the headline shape on one card: BinarySAE 512 -> 32768, n_bits = 4, 65536 rows, ks = default_ks(65) (ten points up to
256).  Four things:

* (a) ``ops.prefix_errors`` alone on a given top-256 list;
* (b) the same numbers from the ops that existed before: per point ``decode_binary_sparse`` on the sliced lists plus
  ``sq_err_sum``.  The two sides' sums are compared before anything is timed;
* (c) ``SparsityCurve.add`` end to end (one selection at K = 256, the op, the batch's moments);
* (d) one ``forward_compact`` per point with ``model.k`` set, plus ``sq_err_sum``: the sweep the curve replaces.

The method is tools/bench_trainer.py's: one process, the sides alternating; a window is ``steps`` iterations between two
device events and ends in a synchronise; median / min / max over ``repeats`` windows.  A side is "faster" only when its
slowest window beats the other side's fastest.  One JSON line per pair.

    python tools/bench_sparsity_curve.py [--rows 65536] [--steps 3] [--warmup 1] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_activity import verdict  # noqa: E402
from bench_optim import alternate, fmt  # noqa: E402
from quantizedsae_amd import BinarySAE, ops, synthetic as S  # noqa: E402
from quantizedsae_amd.inference import SparsityCurve, default_ks  # noqa: E402

D, H, N_BITS, GROUP_ROWS = 512, 32768, 4, 1024
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparsity_curve.py needs cuda:0 (MI355X); nothing is timed without it")
    B = args.rows
    sd = S.binary_sae_params(7, D, H, N_BITS, dec_bias_std=0.1)
    model = BinarySAE(D, H, gamma=4.0, n_bits=N_BITS)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(DEV).eval()
    k0 = model.k
    ks = default_ks(model.top_k)
    K, n = ks[-1], len(ks)
    x = torch.from_numpy(S.activations(5, B, D)).to(DEV)
    curve = SparsityCurve(model, ks, GROUP_ROWS)
    decoder, bias = curve._decoder()
    assert decoder[0] == "packed"
    with torch.no_grad():
        idx, val, _ = model._select(x, K, curve._path(B, K), False)
    sliced = [(idx[:, :k].contiguous(), val[:, :k].contiguous()) for k in ks]

    def op_alone():
        sums = torch.zeros((n,), dtype=torch.float64, device=DEV)
        counts = torch.zeros((2,), dtype=torch.int64, device=DEV)
        ops.prefix_errors(x, idx, val, ks, decoder, bias, GROUP_ROWS, sums, counts)
        return sums

    def composed():
        out = []
        for i, v in sliced:
            recon = ops.decode_binary_sparse(i, v, decoder[1], D, decoder[2], decoder[3], bias)
            out.append(ops.sq_err_sum(recon, x))
        return out

    def curve_add():
        c = SparsityCurve(model, ks, GROUP_ROWS)
        c.add(x)
        return c

    def forward_per_point():
        out = []
        with torch.no_grad():
            for k in ks:
                model.k = (k + 0.5) / H
                out.append(ops.sq_err_sum(model.forward_compact(x)[2], x))
        model.k = k0
        return out

    a = op_alone().cpu().tolist()
    b = [float(t.double().sum()) if t.numel() > 1 else float(t) for t in composed()]
    d = [float(t.double().sum()) if t.numel() > 1 else float(t) for t in forward_per_point()]
    c = curve_add().finish()["sse"].tolist()
    rel = lambda p, q: max(abs(u - v) / abs(v) for u, v in zip(p, q))                    # noqa: E731
    head = {"B": B, "D": D, "H": H, "n_bits": N_BITS, "ks": ks, "steps": args.steps, "repeats": args.repeats}
    got = alternate({"op": op_alone, "composition": composed}, args.steps, args.warmup, args.repeats)
    fma = B * D * sum(ks)
    gathered = sum(ks[i] for i in range(n - 1, -1, -4))          # a launch per four points gathers up to its largest k'
    print(json.dumps({"what": "prefix_errors_vs_decode_per_point", **head, "sse_rel_diff": float(f"{rel(a, b):.3g}"),
                      "op": fmt(got["op"]), "composition": fmt(got["composition"]), "op_is": verdict(got["op"], got["composition"]),
                      "median_ratio": round(got["op"][0] / got["composition"][0], 4),
                      "op_TFLOPs": round(2.0 * fma / (got["op"][0] * 1e-3) / 1e12, 2),
                      "op_gather_GBps": round(B * gathered * (D * N_BITS / 8) / (got["op"][0] * 1e-3) / 1e9, 1)}), flush=True)
    got = alternate({"curve_add": curve_add, "forward_per_point": forward_per_point}, args.steps, args.warmup, args.repeats)
    print(json.dumps({"what": "curve_add_vs_forward_per_point", **head, "sse_rel_diff": float(f"{rel(c, d):.3g}"),
                      "curve_add": fmt(got["curve_add"]), "forward_per_point": fmt(got["forward_per_point"]),
                      "curve_add_is": verdict(got["curve_add"], got["forward_per_point"]),
                      "median_ratio": round(got["curve_add"][0] / got["forward_per_point"][0], 4)}), flush=True)


if __name__ == "__main__":
    main()
