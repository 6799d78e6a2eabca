"""fp64 restatement of the BinaryLatentSAE gradient (reference sae/binary_latent.py:19-27 under
loss.backward()), written from the table: chunked over hidden units so that it never holds a dense [B, H] fp64 tensor for more
units than it checks.  It runs on whatever device its inputs are on.  Also the fixture recipes of
tools/gen_golden_train_blatent.py.

Notation: x [B, D], W_e = encoder.0.weight [H, D], b_e [H], W_d = decoder.weight [D, H], b_d [D];
pre = x W_e^T + b_e, p = sigmoid(pre); z = (p >= 0.5) is GIVEN (bool or 0/1 [B, H]); recon = z W_d^T + b_d;
G = the gradient arriving at recon."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"

#: gradient fixtures: name -> recipe (tools/gen_golden_train_blatent.py runs the reference on them and records the seed it
#: settled on; inputs are regenerated here from that seed)
CASES = {
    "train_blatent_d64": dict(D=64, H=256, B=24, seed=901),
    "train_blatent_d36": dict(D=36, H=96, B=7, seed=902),
    "train_blatent_h1056": dict(D=32, H=1056, B=257, seed=903),
}
PARAM_KEYS = ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.bias")

#: the trainer-loop fixture: steps of forward, F.mse_loss, backward, Adam on a fixed batch
LOOP_FIXTURE = "train_blatent_loop"
LOOP = dict(D=64, H=1024, B=256, seed=911, steps=20, lr=1e-3)

#: sigmoid(w) >= 0.5 in the reference's fp32 op sequence  <=>  w >= this value (bit pattern 0xB43FFFFE, sae/binary_latent.py of
#: the package; tests/golden/sigmoid_cutoffs.npz)
CUTOFF = float(np.array([0xB43FFFFE], dtype=np.uint32).view(np.float32)[0])


def blatent_params(seed: int, D: int, H: int) -> dict:
    """BinaryLatentSAE state_dict (the recipe of the binary_latent_small fixture): xavier encoder, small encoder bias,
    decoder U(+-1/sqrt(H)), decoder bias."""
    return {"encoder.0.weight": S.xavier_uniform(seed, H, D, stream=1),
            "encoder.0.bias": S.normal(seed, (H,), stream=2, std=0.05),
            "decoder.weight": S.uniform(seed, (D, H), -1.0 / np.sqrt(H), 1.0 / np.sqrt(H), stream=3),
            "decoder.bias": S.normal(seed, (D,), stream=4, std=0.1)}


def case_inputs(case: dict, seed: int):
    """(state_dict numpy, x numpy [B, D]) of a recipe at this seed."""
    return blatent_params(seed, case["D"], case["H"]), S.activations(seed, case["B"], case["D"])


def load_fixture(name: str):
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def pack_latent(z) -> np.ndarray:
    """0/1 [B, H] -> uint8 [B, ceil(H / 8)], little-endian within a byte (bit h % 8 of byte h / 8)."""
    return np.packbits(np.asarray(z) != 0, axis=1, bitorder="little")


def unpack_latent(bits, H: int) -> np.ndarray:
    return np.unpackbits(np.asarray(bits), axis=1, bitorder="little")[:, :H].astype(np.float32)


def _t(a, device=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    t = t.detach()
    return t.to(device=device if device is not None else t.device, dtype=torch.float64)


def forward64(z, W_d, b_d, chunk: int = 4096) -> torch.Tensor:
    """recon [B, D] fp64 of a given latent."""
    W_d = _t(W_d)
    dev = W_d.device
    z = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.asarray(z))
    recon = _t(b_d, dev).expand(z.shape[0], -1).clone()
    for u0 in range(0, W_d.shape[1], chunk):
        recon += z[:, u0:u0 + chunk].to(device=dev, dtype=torch.float64) @ W_d[:, u0:u0 + chunk].t()
    return recon


def trainer_incoming(x, recon, B: int, D: int) -> torch.Tensor:
    """G of F.mse_loss(recon, x)."""
    return 2.0 * (_t(recon) - _t(x, _t(recon).device)) / (B * D)


def grads64(x, W_e, b_e, W_d, z, G, want_dx: bool = True, chunk: int = 1024) -> dict:
    """The table of DESIGN.md section 4.24 in fp64, chunked over hidden units, z GIVEN:
        db_d = sum_r G[r];  dW_d = G^T z;  dz = G W_d;  dpre = dz p (1 - p);  dW_e = dpre^T x;  db_e = sum_r dpre[r];
        dx = dpre W_e.
    -> dict: encoder.0.weight [H, D], encoder.0.bias [H], decoder.weight [D, H], decoder.bias [D], x [B, D] (want_dx)."""
    x, W_e, b_e = _t(x), _t(W_e), _t(b_e)
    dev = x.device
    W_d, G = _t(W_d, dev), _t(G, dev)
    z = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.asarray(z))
    B, D = x.shape
    H = W_e.shape[0]
    out = {"encoder.0.weight": torch.zeros((H, D), dtype=torch.float64, device=dev),
           "encoder.0.bias": torch.zeros((H,), dtype=torch.float64, device=dev),
           "decoder.weight": torch.zeros((D, H), dtype=torch.float64, device=dev),
           "decoder.bias": G.sum(0)}
    dx = torch.zeros((B, D), dtype=torch.float64, device=dev) if want_dx else None
    for u0 in range(0, H, chunk):
        sl = slice(u0, min(u0 + chunk, H))
        p = torch.sigmoid(x @ W_e[sl].t() + b_e[sl])
        dpre = (G @ W_d[:, sl]) * (p * (1.0 - p))
        out["encoder.0.weight"][sl] = dpre.t() @ x
        out["encoder.0.bias"][sl] = dpre.sum(0)
        out["decoder.weight"][:, sl] = G.t() @ z[:, sl].to(device=dev, dtype=torch.float64)
        if want_dx:
            dx += dpre @ W_e[sl]
    if want_dx:
        out["x"] = dx
    return out


def max_rel_err(got, want) -> float:
    """max |got - want| / max |want| (0 / 0 = 0)."""
    w = _t(want)
    g = _t(got, w.device)
    scale = float(w.abs().max()) if w.numel() else 0.0
    err = float((g - w).abs().max()) if w.numel() else 0.0
    return err / scale if scale > 0 else err
