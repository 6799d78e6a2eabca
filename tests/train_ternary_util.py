"""fp64 restatement of the TernarySparseAutoencoder gradient and exact restatement of the RigL mask rules (DESIGN.md section
4.13; reference sae/ternary.py:27-90,116-122 under loss.backward()), written from the table: chunked over hidden units so
that it never holds a dense [B, H] fp64 tensor for more units than it checks.  It runs on whatever device its inputs are on.
Also the fixture recipes of tools/gen_golden_train_ternary.py.

Notation: x [B, D], W [H, D], b [H], w = decoder.weight [D, H], m = decoder.mask [D, H];
h = relu(x W^T + b), T = sign(w) (|w| >= 0.5), recon = h T^T; G / gh = the gradients arriving at recon / h.

Mask rules: flat index d H + h.  Keys are compared as the bit patterns of non-negative fp32 values (integers), so every
decision here is exact integer / comparison logic; the exactly-k selections take ties in ascending flat index (a stable
sort), the order the HIP kernels document."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"
THRESHOLD = 0.5
SPARSITY = 0.7                                   # init_mask(0.7) / update_mask(f_decay, 0.7) of the t_sae trainer

#: gradient fixtures: name -> recipe.  l1 > 0 adds l1 * h.abs().mean() to the loss (a gradient arriving at h).
CASES = {
    "train_ternary_d64": dict(D=64, H=256, B=24, l1=0.0, seed=801),
    "train_ternary_d64_l1": dict(D=64, H=256, B=24, l1=0.05, seed=802),
    "train_ternary_h1000": dict(D=32, H=1000, B=8, l1=0.0, seed=803),
}
#: mask fixtures: name -> recipe.  stats: a / delta given (one-row tensors in the reference); ties: duplicated |w| values
#: placed at the drop threshold; f_decay = 0 gives n = 0.
MASK_CASES = {
    "train_ternary_mask_d64": dict(D=64, H=256, f_decay=0.3, stats=True, ties=False, seed=811),
    "train_ternary_mask_h1000": dict(D=32, H=1000, f_decay=0.1, stats=True, ties=False, seed=812),
    "train_ternary_mask_ties": dict(D=64, H=256, f_decay=0.3, stats=True, ties=True, seed=813),
    "train_ternary_mask_nostats": dict(D=64, H=256, f_decay=0.3, stats=False, ties=False, seed=814),
    "train_ternary_mask_n0": dict(D=64, H=256, f_decay=0.0, stats=True, ties=False, seed=815),
}
PARAM_KEYS = ("encoder.0.weight", "encoder.0.bias", "decoder.weight")

#: the trainer-loop fixture: 30 steps of the t_sae branch on a fixed batch
LOOP_FIXTURE = "train_ternary_loop"
LOOP = dict(D=64, H=1024, B=256, seed=721, steps=30, lr=1e-2, f_decay=0.3)


def load_fixture(name: str):
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def pack_mask(m) -> np.ndarray:
    return np.packbits(np.asarray(m).reshape(-1) != 0, bitorder="little")


def unpack_mask(bits, D: int, H: int) -> np.ndarray:
    return np.unpackbits(np.asarray(bits), bitorder="little")[: D * H].reshape(D, H).astype(np.float32)


def _t(a, device=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    t = t.detach()
    return t.to(device=device if device is not None else t.device, dtype=torch.float64)


def _f32(a, device=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    return t.detach().to(device=device if device is not None else t.device, dtype=torch.float32)


# ---- recipes ---------------------------------------------------------------------------------------------------------
def case_inputs(case: dict, seed: int):
    """(state_dict numpy BEFORE init_mask, x numpy [B, D]) of a gradient recipe at this seed."""
    return S.ternary_sae_params(seed, case["D"], case["H"]), S.activations(seed, case["B"], case["D"])


def masked_params(case: dict, seed: int):
    """(state_dict numpy after init_mask(0.7) by the restatement below, x): what the fixtures' gradients belong to."""
    sd, x = case_inputs(case, seed)
    w, m = init_mask_ref(torch.from_numpy(sd["decoder.weight"]), SPARSITY)
    sd = dict(sd)
    sd["decoder.weight"], sd["decoder.mask"] = w.numpy(), m.numpy()
    return sd, x


def mask_case_inputs(case: dict, seed: int):
    """(w [D, H] BEFORE init_mask, a [H] or None, delta [D] or None).  ties: after init_mask the caller duplicates values
    (see plant_drop_ties)."""
    D, H = case["D"], case["H"]
    w = S.ternary_sae_params(seed, D, H)["decoder.weight"]
    if not case["stats"]:
        return w, None, None
    a = np.abs(S.normal(seed, (H,), stream=5)).astype(np.float32)      # a latent mean is non-negative; update_mask takes |a|
    delta = (S.normal(seed, (D,), stream=6) * np.float32(1e-3)).astype(np.float32)
    return w, a, delta


def update_n(numel: int, f_decay: float, sparsity_rate: float = SPARSITY) -> int:
    return int(f_decay * (1 - sparsity_rate) * numel)


def plant_drop_ties(w: torch.Tensor, m: torch.Tensor, n: int, copies: int = 5) -> torch.Tensor:
    """Duplicates the drop threshold: the n-th smallest active |w| is written (with alternating sign) over the `copies`
    next-larger active values, so that the <= rule drops n + copies positions."""
    flat, act = w.reshape(-1).clone(), m.reshape(-1) != 0
    idx = torch.nonzero(act).reshape(-1)
    order = torch.argsort(flat[idx].abs(), stable=True)
    thr = flat[idx[order[n - 1]]].abs()
    for j in range(copies):
        flat[idx[order[n + j]]] = thr if j % 2 == 0 else -thr
    return flat.reshape(w.shape)


# ---- the mask rules, exactly ---------------------------------------------------------------------------------------------
def abs_key(v: torch.Tensor) -> torch.Tensor:
    """int64 bit pattern of |v| (fp32): orders as the value does."""
    return v.detach().to(torch.float32).abs().contiguous().view(torch.int32).to(torch.int64).reshape(-1)


def _best_k(key: torch.Tensor, eligible: torch.Tensor, k: int) -> torch.Tensor:
    """bool [n]: the k eligible elements with the smallest int64 key, ties in ascending index; all of them if fewer."""
    big = torch.full_like(key, 1 << 40)
    order = torch.argsort(torch.where(eligible, key, big), stable=True)
    k = min(int(k), int(eligible.sum()))
    sel = torch.zeros_like(eligible)
    sel[order[:k]] = True
    return sel


def init_mask_ref(w: torch.Tensor, sparsity: float):
    """-> (w * mask, mask) fp32 [D, H]."""
    n = int(w.numel() * sparsity)
    key = abs_key(w)
    sel = _best_k(key, torch.ones_like(key, dtype=torch.bool), n)
    m = (~sel).to(torch.float32).reshape(w.shape)
    return w.to(torch.float32) * m, m


def score_key(a: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """int64 [D H]: bit pattern of |delta[d]| * |a[h]| as one fp32 product."""
    return abs_key(torch.outer(delta.to(torch.float32).abs(), a.to(torch.float32).abs()))


def update_mask_ref(w: torch.Tensor, m: torch.Tensor, a, delta, n: int):
    """-> (w * mask, mask, info).  info: dropped / grown (bool [D H]), the boundary keys either side of each selection."""
    flat = w.to(torch.float32).reshape(-1)
    active = m.reshape(-1) != 0
    info = {"n": n}
    dropped = torch.zeros_like(active)
    grown = torch.zeros_like(active)
    if n > 0:
        key = abs_key(flat)
        n_act = int(active.sum())
        if n_act:
            sorted_keys = torch.sort(key[active]).values
            thr = sorted_keys[min(n, n_act) - 1]
            dropped = active & (key <= thr)
            info["drop_key"] = int(thr)
            above = sorted_keys[sorted_keys > thr]
            info["drop_next_key"] = int(above[0]) if above.numel() else -1
        active = active & ~dropped
    if n > 0 and a is not None:
        sk = score_key(a.to(flat.device), delta.to(flat.device))
        grown = _best_k((1 << 31) - sk, ~active, n)
        if bool(grown.any()):
            info["grow_key"] = int(sk[grown].min())
            rest = sk[~active & ~grown]
            info["grow_next_key"] = int(rest.max()) if rest.numel() else -1
        active = active | grown
    info["dropped"], info["grown"] = dropped, grown
    mm = active.to(torch.float32).reshape(w.shape)
    return w.to(torch.float32) * mm, mm, info


# ---- the gradient table in fp64 --------------------------------------------------------------------------------------------
def ternary64(w) -> torch.Tensor:
    w = _t(w)
    return torch.sign(w) * (w.abs() >= THRESHOLD).to(torch.float64)


def forward64(x, W, b, w, chunk: int = 4096):
    """(recon [B, D] fp64, min |pre|) -- the latent is not kept."""
    x, W, b = _t(x), _t(W), _t(b)
    dev = x.device
    T = ternary64(_t(w, dev))
    recon = torch.zeros((x.shape[0], T.shape[0]), dtype=torch.float64, device=dev)
    min_abs = float("inf")
    for u0 in range(0, W.shape[0], chunk):
        pre = x @ W[u0:u0 + chunk].t() + b[u0:u0 + chunk]
        min_abs = min(min_abs, float(pre.abs().min()))
        recon += torch.relu(pre) @ T[:, u0:u0 + chunk].t()
    return recon, min_abs


def trainer_incoming(x, recon, B: int, D: int):
    """G of F.mse_loss(recon, x)."""
    return 2.0 * (_t(recon) - _t(x, _t(recon).device)) / (B * D)


def grads64(x, W, b, w, m, G, gh=None, units=None, want_dx: bool = False, chunk: int = 1024, active=None):
    """The table of DESIGN.md section 4.13 in fp64 for the hidden units ``units`` (default all).  G [B, D] or None; gh: a
    callable units -> [B, u] (or a tensor [B, H], or None).  active: bool [B, H] -- which latents the forward under test
    found positive -- makes the ReLU pattern GIVEN (at full size some of the 2.7e8 pre-activations lie within fp32 rounding
    of zero); None: pre > 0 in fp64.  -> dict: encoder.0.weight [U, D], encoder.0.bias [U],
    decoder.weight [D, U] (columns ``units``), a [U] (batch mean of h), x [B, D] (want_dx; all units only)."""
    x, W, b = _t(x), _t(W), _t(b)
    dev = x.device
    w, m = _t(w, dev), _t(m, dev)
    B, D = x.shape
    H = W.shape[0]
    units = torch.arange(H) if units is None else torch.as_tensor(units).long().cpu()
    U = units.numel()
    G = _t(G, dev) if G is not None else None
    out = {"encoder.0.weight": torch.zeros((U, D), dtype=torch.float64, device=dev),
           "encoder.0.bias": torch.zeros((U,), dtype=torch.float64, device=dev),
           "decoder.weight": torch.zeros((D, U), dtype=torch.float64, device=dev),
           "a": torch.zeros((U,), dtype=torch.float64, device=dev)}
    dx = torch.zeros((B, D), dtype=torch.float64, device=dev) if want_dx else None
    for c0 in range(0, U, chunk):
        uu = units[c0:c0 + chunk]
        ud = uu.to(dev)
        pre = x @ W[ud].t() + b[ud]
        pos = (pre > 0) if active is None else torch.as_tensor(active)[:, ud].to(dev)
        h = torch.where(pos, pre, torch.zeros_like(pre))
        T = ternary64(w[:, ud])                                      # [D, u]
        dh = torch.zeros_like(pre)
        if gh is not None:
            dh = dh + (_t(gh(uu), dev) if callable(gh) else _t(gh, dev)[:, ud])
        if G is not None:
            dh = dh + G @ T
        dpre = dh * pos
        sl = slice(c0, c0 + uu.numel())
        out["encoder.0.weight"][sl] = dpre.t() @ x
        out["encoder.0.bias"][sl] = dpre.sum(0)
        out["a"][sl] = h.mean(0)
        if G is not None:
            out["decoder.weight"][:, sl] = m[:, ud] * (G.t() @ h)
        if want_dx:
            dx += dpre @ W[ud]
    if want_dx:
        out["x"] = dx
    return out


def l1_incoming(x, W, b, l1: float):
    """gh of l1 * h.abs().mean() as a callable over units: l1 * (pre > 0) / (B H)."""
    x64, W64, b64 = _t(x), _t(W), _t(b)
    B, H = x64.shape[0], W64.shape[0]

    def gh(units):
        ud = torch.as_tensor(units).long().to(x64.device)
        return l1 * ((x64 @ W64[ud].t() + b64[ud]) > 0).to(torch.float64) / (B * H)
    return gh


def max_rel_err(got, want) -> float:
    """max |got - want| / max |want| (0 / 0 = 0)."""
    w = _t(want)
    g = _t(got, w.device)
    scale = float(w.abs().max()) if w.numel() else 0.0
    err = float((g - w).abs().max()) if w.numel() else 0.0
    return err / scale if scale > 0 else err
