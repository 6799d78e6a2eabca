"""fp64 restatement of the QuantizedMatryoshkaSAE gradient (reference
sae/quantized_matryoshka.py:47-190 under loss.backward(), joint_gradient=False), written from the table: per-unit terms only,
chunked over hidden units so that it never holds a dense [B, H] fp64 tensor for more units than it checks.  It runs on
whatever device its inputs are on.  Also the fixture recipes of tools/gen_golden_train_matryoshka.py.

Notation: p = sigmoid(x W_enc^T + b_enc); z = (p > 0.5) is GIVEN (bool [B, H], hidden units in the parameters' order);
S = Bs + Bm with Bs = sgn(weight >= 0) (sigmoid(w) >= .5), Bm likewise from weight_mirror;
scale_h = 2^(n-i-2) quant_step / (||S_h|| + 1e-8) for h in level i."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from quantizedsae_amd import synthetic as S
from quantizedsae_amd.sae.quantized_matryoshka import nested_sizes

GOLDEN = Path(__file__).resolve().parent / "golden"

#: fixture name -> recipe (tools/gen_golden_train_matryoshka.py runs the reference on them; inputs are regenerated here)
CASES = {
    "train_matryoshka_d64": dict(kind="q", D=64, H=256, n_bits=4, B=24, lam=1.5e-3, sigmas=-2.5, allow_bias=True, seed=701),
    "train_matryoshka_d64_dense": dict(kind="q", D=64, H=256, n_bits=4, B=24, lam=1.5e-3, sigmas=0.0, allow_bias=True, seed=702),
    "train_matryoshka_n1_nobias": dict(kind="q", D=64, H=256, n_bits=1, B=24, lam=1.5e-3, sigmas=-2.5, allow_bias=False, seed=703),
    "train_matryoshka_h1000": dict(kind="q", D=32, H=1000, n_bits=4, B=8, lam=1.5e-3, sigmas=-2.5, allow_bias=True, seed=704),
    "train_matryoshka_residual": dict(kind="rq", D=64, H=512, n_bits=4, B=24, lam=1.5e-3, sigmas=-2.5, allow_bias=True, seed=705),
}
ABS_RANGE = 1.5                                  # the q_sae / rq_sae entries of SAE_REGISTRY
RQ_STAGE_WEIGHTS = (1.0, 2.5, 4.0, 8.0)          # sparsity weights of the rq_sae branch (training/trainer.py:127-134)
PARAM_KEYS = ("encoder.0.weight", "encoder.0.bias", "decoder.weight", "decoder.weight_mirror", "decoder.bias")

#: the trainer-loop fixture: 30 steps of the q_sae / rq_sae branches on a fixed batch
LOOP_FIXTURE = "train_matryoshka_loop"
LOOP = dict(D=64, H=1024, n_bits=4, B=256, lam=1.5e-3, seed=711, steps=30)
LOOP_CASES = {
    "q_sparse": dict(kind="q", sigmas=-2.5, lr=1e-2),
    "q_dense": dict(kind="q", sigmas=0.0, lr=1e-2),
    "rq": dict(kind="rq", sigmas=-2.5, lr=1e-3),
}


def q_params(seed: int, D: int, H: int, sigmas: float, stream0: int = 0) -> dict:
    return S.matryoshka_sae_params(seed, D, H, bias_std=0.1, stream0=stream0, enc_bias_sigmas=sigmas)


def rq_params(seed: int, D: int, H: int, n_bits: int, sigmas: float) -> dict:
    """state_dict of a ResidualQuantizedSAE: stage i from matryoshka_sae_params with stream0 = 16 i."""
    sd = {}
    for i, h in enumerate(nested_sizes(H, n_bits)):
        for k, v in q_params(seed, D, h, sigmas, stream0=16 * i).items():
            sd[f"saes.{i}.{k}"] = v
    return sd


def case_inputs(case: dict, seed: int):
    """(state_dict numpy, x numpy [B, D]) of a fixture recipe at this seed."""
    D, H = case["D"], case["H"]
    sd = rq_params(seed, D, H, case["n_bits"], case["sigmas"]) if case["kind"] == "rq" else q_params(seed, D, H, case["sigmas"])
    return sd, S.activations(seed, case["B"], D)


def load_fixture(name: str):
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def _t(a, device=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    t = t.detach()
    return t.to(device=device if device is not None else t.device, dtype=torch.float64)


def level_of_units(H: int, n_bits: int) -> torch.Tensor:
    """int64 [H]: the level of every hidden unit."""
    return torch.repeat_interleave(torch.arange(n_bits), torch.tensor(nested_sizes(H, n_bits)))


def decoder_terms(w, wm, n_bits: int, abs_range: float = ABS_RANGE, H_total: int = None, units=None):
    """(S [U, D], scale [U], Bs, Bm, level [U]) of the given rows of weight / weight_mirror.  ``units``: the hidden indices the
    rows belong to (default: all H_total = len(w) of them)."""
    w, wm = _t(w), _t(wm)
    H = H_total if H_total is not None else w.shape[0]
    units = torch.arange(H) if units is None else torch.as_tensor(units).long().cpu()
    level = level_of_units(H, n_bits)[units].to(w.device)
    Bs = torch.where(w >= 0, 1.0, -1.0).to(torch.float64)
    Bm = torch.where(wm >= 0, 1.0, -1.0).to(torch.float64)
    Ssum = Bs + Bm
    quant_step = abs_range / (2 ** (n_bits - 1))
    factor = torch.tensor([2.0 ** (n_bits - i - 2) * quant_step for i in range(n_bits)], dtype=torch.float64, device=w.device)
    scale = factor[level] / (torch.linalg.vector_norm(Ssum, dim=1) + 1e-8)
    return Ssum, scale, Bs, Bm, level


def forward64(z, w, wm, bias, n_bits: int, allow_bias: bool, abs_range: float = ABS_RANGE, chunk: int = 4096):
    """(groups [n], levels [n, B, D]) in fp64 on the given z (bool [B, H])."""
    w, wm = _t(w), _t(wm)
    dev = w.device
    z = torch.as_tensor(z).to(dev)
    B, H = z.shape
    D = w.shape[1]
    sizes = nested_sizes(H, n_bits)
    levels = torch.zeros((n_bits, B, D), dtype=torch.float64, device=dev)
    groups = torch.zeros((n_bits,), dtype=torch.float64, device=dev)
    run = torch.zeros((B, D), dtype=torch.float64, device=dev)
    start = 0
    for i, size in enumerate(sizes):
        for u0 in range(start, start + size, chunk):
            u1 = min(start + size, u0 + chunk)
            units = torch.arange(u0, u1)
            Ssum, scale, _, _, _ = decoder_terms(w[u0:u1], wm[u0:u1], n_bits, abs_range, H, units)
            zc = z[:, u0:u1].to(torch.float64)
            run = run + (zc * scale) @ Ssum
            groups[i] += zc.sum() / B
        if i == 0 and allow_bias:
            run = run + _t(bias, dev)
        levels[i] = run
        start += size
    return groups, levels


def trainer_incoming(x, levels, n_bits: int, lam: float, target=None):
    """Incoming gradients of the q_sae loss (training/trainer.py:88-112): sum_i 0.5 mse(result[i], x) + lam sum_i
    latent_group[i] -> (G [n, B, D], gg [n])."""
    levels = _t(levels)
    x = _t(x, levels.device) if target is None else _t(target, levels.device)
    B, D = x.shape
    G = 0.5 * 2.0 * (levels - x) / (B * D)
    gg = torch.full((n_bits,), lam, dtype=torch.float64, device=levels.device)
    return G, gg


def trainer_loss64(x, levels, groups, lam: float) -> float:
    levels, groups = _t(levels), _t(groups)
    x = _t(x, levels.device)
    return float(sum(0.5 * ((levels[i] - x) ** 2).mean() for i in range(levels.shape[0])) + lam * groups.sum())


def grads64(x, W, b, w, wm, z, G, gg, n_bits: int, allow_bias: bool, abs_range: float = ABS_RANGE, units=None,
            want_dx: bool = False, chunk: int = 1024):
    """The table of DESIGN.md section 4.12 in fp64 for the hidden units ``units`` (default all), all D columns of each.
    z: bool [B, H]; G: [n, B, D] incoming gradients of result[i] or None; gg: [n] incoming gradients of latent_group[i] or
    None.  -> dict: encoder.0.weight [U, D], encoder.0.bias [U], decoder.weight [U, D], decoder.weight_mirror [U, D],
    decoder.bias [D] (None without allow_bias), cnt [U], secant.decoder.weight / secant.decoder.weight_mirror (the decoder
    gradients after apply_secant_grad()), x [B, D] (want_dx; only meaningful when units covers every unit)."""
    x, W, b = _t(x), _t(W), _t(b)
    dev = x.device
    w, wm = _t(w, dev), _t(wm, dev)
    z = torch.as_tensor(z).to(dev)
    B, D = x.shape
    H = W.shape[0]
    units = torch.arange(H) if units is None else torch.as_tensor(units).long().cpu()
    U = units.numel()
    G = _t(G, dev) if G is not None else None
    gg = _t(gg, dev) if gg is not None else torch.zeros((n_bits,), dtype=torch.float64, device=dev)
    out = {k: torch.zeros((U, D), dtype=torch.float64, device=dev)
           for k in ("encoder.0.weight", "decoder.weight", "decoder.weight_mirror", "secant.decoder.weight",
                     "secant.decoder.weight_mirror")}
    out["encoder.0.bias"] = torch.zeros((U,), dtype=torch.float64, device=dev)
    out["cnt"] = torch.zeros((U,), dtype=torch.float64, device=dev)
    dx = torch.zeros((B, D), dtype=torch.float64, device=dev) if want_dx else None
    c = 1.0 / (B * D)
    for c0 in range(0, U, chunk):
        uu = units[c0:c0 + chunk]
        ud = uu.to(dev)
        Ssum, scale, Bs, Bm, level = decoder_terms(w[ud], wm[ud], n_bits, abs_range, H, uu)
        p = torch.sigmoid(x @ W[ud].t() + b[ud])                     # [B, u]
        zc = z[:, ud].to(torch.float64)
        dz = (gg[level] / B).expand(B, -1).clone()
        dsum = torch.zeros((uu.numel(), D), dtype=torch.float64, device=dev)
        if G is not None:
            for i in range(n_bits):
                sel = level == i
                if bool(sel.any()):
                    dz[:, sel] += (G[i] @ Ssum[sel].t()) * scale[sel]
                    dsum[sel] = zc[:, sel].t() @ G[i]
        dpre = dz * p * (1.0 - p)
        sl = slice(c0, c0 + uu.numel())
        out["encoder.0.weight"][sl] = dpre.t() @ x
        out["encoder.0.bias"][sl] = dpre.sum(0)
        if want_dx:
            dx += dpre @ W[ud]
        cnt = zc.sum(0)
        out["cnt"][sl] = cnt
        sec = (c * cnt * scale ** 2)[:, None]
        for key, logit, sign in (("decoder.weight", w[ud], Bs), ("decoder.weight_mirror", wm[ud], Bm)):
            sw = torch.sigmoid(logit)
            g = scale[:, None] * dsum * sw * (1.0 - sw)
            out[key][sl] = g
            out["secant." + key][sl] = g - sec * sign * sw * (1.0 - sw)
    out["decoder.bias"] = G[0].sum(0) if (allow_bias and G is not None) else (
        torch.zeros((D,), dtype=torch.float64, device=dev) if allow_bias else None)
    if want_dx:
        out["x"] = dx
    return out


def unpack_bits(zbits, H: int, index=None) -> torch.Tensor:
    """bool [B, H] from int32-packed z bits [B, words] in the packed (padded) hidden order; ``index`` is the decoder's
    padded_index (source unit of every padded slot, -1 for a pad slot) or None."""
    zb = torch.as_tensor(zbits)
    shifts = torch.arange(32, device=zb.device, dtype=torch.int32)
    bits = ((zb.unsqueeze(-1) >> shifts) & 1).reshape(zb.shape[0], -1).bool()
    if index is None:
        return bits[:, :H]
    index = torch.as_tensor(index).to(zb.device)
    out = torch.zeros((zb.shape[0], H), dtype=torch.bool, device=zb.device)
    out[:, index[index >= 0]] = bits[:, : index.numel()][:, index >= 0]
    return out


def max_rel_err(got, want) -> float:
    """max |got - want| / max |want| (0 / 0 = 0)."""
    w = _t(want)
    g = _t(got, w.device)
    scale = float(w.abs().max()) if w.numel() else 0.0
    err = float((g - w).abs().max()) if w.numel() else 0.0
    return err / scale if scale > 0 else err
