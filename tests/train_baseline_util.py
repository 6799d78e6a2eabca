"""fp64 CPU restatement of the BaselineSparseAutoencoder gradient (reference sae/baseline.py:17-40
under loss.backward()), built from the selection idx [B, k] with gathers and index_add_ -- never a dense [B, H] tensor --
so that it runs at B = 8192, H = 32768 in seconds.  Also the fixture recipes of tools/gen_golden_train_baseline.py."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"

#: fixture name -> recipe (tools/gen_golden_train_baseline.py writes them with the reference; inputs are regenerated here)
CASES = {
    "train_baseline_d64": dict(D=64, H=256, k=8, B=24, mu=0.0, x_grad=False, seed=601),
    "train_baseline_d64_l1": dict(D=64, H=256, k=8, B=24, mu=3e-3, x_grad=True, seed=602),
    "train_baseline_d32_k32": dict(D=32, H=256, k=32, B=24, mu=0.0, x_grad=False, seed=603),
}
#: the fixture that also stores decoder.weight after the reference's normalize_decoder_weights()
NORMALIZED_CASE = "train_baseline_d64"

GRAD_KEYS = ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.bias")


def case_inputs(case: dict, seed: int):
    """(state_dict numpy, x numpy [B, D]) of a fixture recipe at this seed."""
    return S.baseline_sae_params(seed, case["D"], case["H"], bias_std=0.1), S.activations(seed, case["B"], case["D"])


def load_fixture(name: str):
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def _t(a) -> torch.Tensor:
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).detach().cpu().to(torch.float64)


def _idx(idx) -> torch.Tensor:
    return torch.as_tensor(np.asarray(idx) if not isinstance(idx, torch.Tensor) else idx).long().cpu()


def _rows(B: int, chunk: int):
    for r0 in range(0, B, chunk):
        yield r0, min(B, r0 + chunk)


def forward64(x, W, b, W_dec, b_dec, idx, chunk: int = 512):
    """(val [B, k], recon [B, D]) in fp64 on a given selection idx; W_dec is decoder.weight [D, H]."""
    x, W, b, b_dec = _t(x), _t(W), _t(b), _t(b_dec)
    T = _t(W_dec).t().contiguous()
    idx = _idx(idx)
    val = torch.empty(idx.shape, dtype=torch.float64)
    recon = torch.empty(x.shape, dtype=torch.float64)
    for r0, r1 in _rows(x.shape[0], chunk):
        ii = idx[r0:r1]
        v = torch.einsum("rd,rjd->rj", x[r0:r1], W[ii]) + b[ii]
        val[r0:r1] = v
        recon[r0:r1] = torch.einsum("rj,rjd->rd", v, T[ii]) + b_dec
    return val, recon


def grads64(x, W, W_dec, idx, val, g_recon=None, g_latent_sel=None, want_dx: bool = False, chunk: int = 512):
    """The table of DESIGN.md section 4.11 in fp64.  idx / val [B, k] are the selection and its values; g_recon [B, D],
    g_latent_sel [B, k] (the incoming latent gradient at the selected positions); None = 0.
    -> dict of encoder.0.weight, encoder.0.bias, decoder.weight [D, H], decoder.bias, x (if want_dx), gv."""
    x, W = _t(x), _t(W)
    T = _t(W_dec).t().contiguous()
    idx = _idx(idx)
    val = _t(val)
    B, D = x.shape
    H = W.shape[0]
    k = idx.shape[1]
    gR = _t(g_recon) if g_recon is not None else None
    gv = _t(g_latent_sel).clone() if g_latent_sel is not None else torch.zeros((B, k), dtype=torch.float64)
    dW = torch.zeros((H, D), dtype=torch.float64)
    db = torch.zeros((H,), dtype=torch.float64)
    dT = torch.zeros((H, D), dtype=torch.float64)
    dx = torch.zeros((B, D), dtype=torch.float64) if want_dx else None
    for r0, r1 in _rows(B, chunk):
        ii = idx[r0:r1]
        if gR is not None:
            gv[r0:r1] += torch.einsum("rd,rjd->rj", gR[r0:r1], T[ii])
        flat = ii.reshape(-1)
        g = gv[r0:r1]
        dW.index_add_(0, flat, (g[:, :, None] * x[r0:r1, None, :]).reshape(-1, D))
        db.index_add_(0, flat, g.reshape(-1))
        if gR is not None:
            dT.index_add_(0, flat, (val[r0:r1, :, None] * gR[r0:r1, None, :]).reshape(-1, D))
        if want_dx:
            dx[r0:r1] = torch.einsum("rj,rjd->rd", g, W[ii])
    out = {"encoder.0.weight": dW, "encoder.0.bias": db, "decoder.weight": dT.t().contiguous(),
           "decoder.bias": gR.sum(0) if gR is not None else torch.zeros((D,), dtype=torch.float64), "gv": gv}
    if want_dx:
        out["x"] = dx
    return out


def trainer_loss_grads(x, recon, val, mu: float = 0.0):
    """Incoming gradients of loss = mse(recon, x) + mu |h_sparse|.sum() / B (the baseline_sae branch of trainer.py:166-173,
    plus an optional L1 term): (g_recon [B, D], g_latent_sel [B, k] or None)."""
    x, recon, val = _t(x), _t(recon), _t(val)
    B, D = x.shape
    gR = 2.0 * (recon - x) / (B * D)
    gL = mu * torch.sign(val) / B if mu else None
    return gR, gL


def loss64(x, recon, val, mu: float = 0.0) -> float:
    x, recon, val = _t(x), _t(recon), _t(val)
    loss = ((recon - x) ** 2).mean()
    if mu:
        loss = loss + mu * val.abs().sum() / x.shape[0]
    return float(loss)


def normalize64(W_dec) -> torch.Tensor:
    """decoder.weight / clamp(norm over dim 0, min=1e-8) in fp64 (sae/baseline.py:42-51)."""
    w = _t(W_dec)
    return w / torch.clamp(torch.linalg.vector_norm(w, dim=0, keepdim=True), min=1e-8)


def max_rel_err(got, want) -> float:
    """max |got - want| / max |want| (0 / 0 = 0)."""
    g, w = _t(got), _t(want)
    scale = float(w.abs().max()) if w.numel() else 0.0
    err = float((g - w).abs().max()) if w.numel() else 0.0
    return err / scale if scale > 0 else err
