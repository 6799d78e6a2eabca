"""fp64 CPU restatement of the BinarySAE gradient (reference sae/binary.py:24-47, 91-103 under
loss.backward()), built from the selection idx [B, k] with gathers and index_add_ -- never a dense [B, H] tensor -- so
that it runs at B = 8192, H = 32768 in seconds.  Also the fixture recipes of tools/gen_golden_train.py."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"

#: fixture name -> recipe (tools/gen_golden_train.py writes them with the reference; the inputs are regenerated here)
CASES = {
    "train_binary_d64": dict(D=64, H=256, n_bits=4, gamma=4.0, k=8, B=24, logit_std=1.0, lam=1e-2, mu=0.0, x_grad=False,
                             seed=501),
    "train_binary_d64_l1": dict(D=64, H=256, n_bits=4, gamma=4.0, k=8, B=24, logit_std=1.0, lam=1e-2, mu=3e-3,
                                x_grad=True, seed=502),
    "train_binary_d32_kaiming": dict(D=32, H=256, n_bits=8, gamma=1.5, k=8, B=24, logit_std=float(np.sqrt(2.0 / (32 * 8))),
                                     lam=1e-2, mu=0.0, x_grad=False, seed=503),
}

GRAD_KEYS = ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.bias")


def case_inputs(case: dict, seed: int):
    """(state_dict numpy, x numpy [B, D]) of a fixture recipe at this seed."""
    sd = S.binary_sae_params(seed, case["D"], case["H"], case["n_bits"], logit_std=case["logit_std"], dec_bias_std=0.1,
                             enc_bias_std=0.05)
    x = S.activations(seed, case["B"], case["D"])
    return sd, x


def load_fixture(name: str):
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def _t(a) -> torch.Tensor:
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).detach().cpu().to(torch.float64)


def soft_table64(logits, D: int, n_bits: int):
    """(T [H, D], p [H, D, n]) in fp64: T = sum_b sigmoid(logit_b) bw_b, bw = [1, 2, .., -2^(n-1)]."""
    L = _t(logits)
    p = torch.sigmoid(L).view(L.shape[0], D, n_bits)
    bw = 2.0 ** torch.arange(n_bits, dtype=torch.float64)
    bw[-1] = -bw[-1]
    return (p * bw).sum(-1), p


def _rows(B: int, chunk: int):
    for r0 in range(0, B, chunk):
        yield r0, min(B, r0 + chunk)


def forward64(x, W, b, logits, b_dec, n_bits: int, gamma: float, idx, chunk: int = 512):
    """(val [B, k], recon [B, D], polarize) in fp64 on a given selection idx."""
    x, W, b, b_dec = _t(x), _t(W), _t(b), _t(b_dec)
    idx = torch.as_tensor(np.asarray(idx) if not isinstance(idx, torch.Tensor) else idx).long().cpu()
    B, D = x.shape
    step = gamma / 2 ** (n_bits - 1)
    T, p = soft_table64(logits, D, n_bits)
    val = torch.empty(idx.shape, dtype=torch.float64)
    recon = torch.empty((B, D), dtype=torch.float64)
    for r0, r1 in _rows(B, chunk):
        ii = idx[r0:r1]
        v = torch.einsum("rd,rjd->rj", x[r0:r1], W[ii]) + b[ii]
        val[r0:r1] = v
        recon[r0:r1] = step * torch.einsum("rj,rjd->rd", v, T[ii]) + b_dec
    pw = 2.0 ** torch.arange(n_bits, dtype=torch.float64)
    pol = (p * (1 - p) * pw).mean()
    return val, recon, float(pol)


def grads64(x, W, logits, n_bits: int, gamma: float, idx, val, g_recon=None, g_latent_sel=None, g_pol=None,
            want_dx: bool = False, chunk: int = 512):
    """The table of DESIGN.md section 4.10 in fp64.  idx / val [B, k] are the selection and its (fp32) values;
    g_recon [B, D], g_latent_sel [B, k] (the incoming latent gradient at the selected positions), g_pol a float; any of
    them None = 0.  -> dict of encoder.0.weight, encoder.0.bias, decoder.weight, decoder.bias, x (if want_dx), gv."""
    x, W, L = _t(x), _t(W), _t(logits)
    idx = torch.as_tensor(np.asarray(idx) if not isinstance(idx, torch.Tensor) else idx).long().cpu()
    val = _t(val)
    B, D = x.shape
    H = W.shape[0]
    k = idx.shape[1]
    step = gamma / 2 ** (n_bits - 1)
    T, p = soft_table64(L, D, n_bits)
    gR = _t(g_recon) if g_recon is not None else None
    gv = _t(g_latent_sel).clone() if g_latent_sel is not None else torch.zeros((B, k), dtype=torch.float64)
    dW = torch.zeros((H, D), dtype=torch.float64)
    db = torch.zeros((H,), dtype=torch.float64)
    Sg = torch.zeros((H, D), dtype=torch.float64)
    dx = torch.zeros((B, D), dtype=torch.float64) if want_dx else None
    for r0, r1 in _rows(B, chunk):
        ii = idx[r0:r1]
        if gR is not None:
            gv[r0:r1] += step * torch.einsum("rd,rjd->rj", gR[r0:r1], T[ii])
        flat = ii.reshape(-1)
        g = gv[r0:r1]
        dW.index_add_(0, flat, (g[:, :, None] * x[r0:r1, None, :]).reshape(-1, D))
        db.index_add_(0, flat, g.reshape(-1))
        if gR is not None:
            Sg.index_add_(0, flat, (val[r0:r1, :, None] * gR[r0:r1, None, :]).reshape(-1, D))
        if want_dx:
            dx[r0:r1] = torch.einsum("rj,rjd->rd", g, W[ii])
    dInt = step * Sg
    bw = 2.0 ** torch.arange(n_bits, dtype=torch.float64)
    pw = bw.clone()
    bw[-1] = -bw[-1]
    gp = float(g_pol) if g_pol is not None else 0.0
    dl = (dInt[:, :, None] * bw + gp * pw * (1 - 2 * p) / (H * D * n_bits)) * p * (1 - p)
    out = {"encoder.0.weight": dW, "encoder.0.bias": db, "decoder.weight": dl.reshape(H, D * n_bits),
           "decoder.bias": gR.sum(0) if gR is not None else torch.zeros((D,), dtype=torch.float64), "gv": gv}
    if want_dx:
        out["x"] = dx
    return out


def trainer_loss_grads(x, recon, val, lam: float, mu: float = 0.0):
    """Incoming gradients of loss = 0.5 mse(recon, x) + lam polarize + mu |sparse latent|.sum() / B (the b_sae branch of
    trainer.py:144-153, plus an optional L1 term): (g_recon [B, D], g_latent_sel [B, k], g_pol)."""
    x, recon, val = _t(x), _t(recon), _t(val)
    B, D = x.shape
    gR = (recon - x) / (B * D)
    gL = mu * torch.sign(val) / B if mu else None
    return gR, gL, lam


def max_rel_err(got, want) -> float:
    """max |got - want| / max |want| (0 / 0 = 0)."""
    g, w = _t(got), _t(want)
    scale = float(w.abs().max()) if w.numel() else 0.0
    err = float((g - w).abs().max()) if w.numel() else 0.0
    return err / scale if scale > 0 else err
