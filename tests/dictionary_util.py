"""Recipes of the decoder-dictionary fixtures (tests/golden/dictionary_*.npz): model state dicts from the portable PRNG
of quantizedsae_amd/synthetic.py, and an fp64 numpy restatement of the comparison on atoms."""
from __future__ import annotations

import numpy as np

from quantizedsae_amd import synthetic as S
from quantizedsae_amd.sae.quantized_matryoshka import nested_sizes

N_BITS, GAMMA, ABS_RANGE, TOP_K = 4, 1.5, 1.5, 32


def state_dict(spec: dict, D: int, H: int) -> dict:
    v, seed = spec["variant"], spec["seed"]
    if v == "binary":
        sd = S.binary_sae_params(seed, D, H, N_BITS)
    elif v == "baseline":
        sd = S.baseline_sae_params(seed, D, H)
    elif v == "matryoshka":
        sd = S.matryoshka_sae_params(seed, D, H)
    elif v == "residual":
        sd = {}
        for i, h in enumerate(nested_sizes(H, N_BITS)):
            for k, a in S.matryoshka_sae_params(seed, D, h, stream0=100 * (i + 1)).items():
                sd[f"saes.{i}.{k}"] = a
    else:
        raise KeyError(v)
    z = spec.get("zero_atom")
    if z is not None:       # baseline only: atom z is column z of decoder.weight [D, H]
        sd["decoder.weight"] = sd["decoder.weight"].copy()
        sd["decoder.weight"][:, z] = 0.0
    return sd


def build(classes, spec: dict, D: int, H: int):
    """classes: namespace with BinarySAE, BaselineSparseAutoencoder, QuantizedMatryoshkaSAE, ResidualQuantizedSAE
    (this package's or the reference's: same constructors, same state-dict keys)."""
    import torch
    v = spec["variant"]
    if v == "binary":
        m = classes.BinarySAE(D, H, gamma=GAMMA, n_bits=N_BITS)
    elif v == "baseline":
        m = classes.BaselineSparseAutoencoder(D, H)
    elif v == "matryoshka":
        m = classes.QuantizedMatryoshkaSAE(D, H, top_k=TOP_K, abs_range=ABS_RANGE, n_bits=N_BITS)
    else:
        m = classes.ResidualQuantizedSAE(D, H, top_k=TOP_K, abs_range=ABS_RANGE, n_bits=N_BITS)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in state_dict(spec, D, H).items()})
    return m.eval()


def atoms_np(spec: dict, D: int, H: int) -> np.ndarray:
    """fp32 atoms [n, D] by the reference's selection and orientation rule, restated in numpy."""
    sd = state_dict(spec, D, H)
    v = spec["variant"]
    if v == "binary":
        w = sd["decoder.weight"].reshape(H, D, N_BITS) > 0          # saturated logits: bit = w > 0
        ints = sum(w[..., j].astype(np.int64) << j for j in range(N_BITS))
        ints = np.where(ints >= 1 << (N_BITS - 1), ints - (1 << N_BITS), ints).astype(np.float32)
        step = np.float32(GAMMA) / np.float32(2 ** (N_BITS - 1))
        mats = [(step * ints).astype(np.float32)]
    elif v == "baseline":
        mats = [sd["decoder.weight"]]
    elif v == "matryoshka":
        mats = [sd["decoder.weight"] + sd["decoder.weight_mirror"]]
    else:
        mats = [sd[f"saes.{i}.decoder.weight"] + sd[f"saes.{i}.decoder.weight_mirror"]
                for i in range(len(nested_sizes(H, N_BITS)))]
    out = []
    for t in mats:
        if t.shape[1] == D:
            out.append(t)
        elif t.shape[0] == D:
            out.append(t.T)
        else:
            out.append(t)
    return np.ascontiguousarray(np.concatenate(out, 0), dtype=np.float32)


def cosine_f64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    na = np.maximum(np.linalg.norm(a, axis=1), 1e-12)
    nb = np.maximum(np.linalg.norm(b, axis=1), 1e-12)
    return (a / na[:, None]) @ (b / nb[:, None]).T
