#!/usr/bin/env python3
"""Generate tests/golden/trainer_epoch.npz: the REFERENCE model classes (tools/ref_loader.py) inside a restatement of the
reference's Trainer.one_epoch / train (training/trainer.py:66-173, 234-258; the file itself cannot be imported: it imports
wandb and starts a training run at import), on the CPU.

The recipe is tests/trainer_util.py's EPOCH: a chunk of 6 x 50 x 64 fp16 hidden states with one NaN planted, stored under
two chunk-file names (two epochs), batches of 64 through DataLoader(HiddenStatesTorchDataset, shuffle=True, num_workers=0)
-- five per epoch, the last one short, one skipped for its NaN -- H = 1024, a fresh Adam per epoch, the per-type step
sequence, and for t_sae the rigL schedule.  Weights come from the portable PRNG recipes.  Per type the fixture records the
batch indices that were trained on, the loss of every step from a run with the model in fp64 and from one in fp32, the
largest relative gap between the two and bound = max(10 * gap, 1e-5), which the GPU loop is held to.  Seeds are searched
until gap < MAX_GAP for every type: a looser curve pins nothing (a top-k selection or a mask update that falls differently
in fp32 and fp64 shows as a large gap).  bl_sae has no branch in the reference's loop; it is trained with mse + Adam, the
recipe of train_blatent_loop.npz.  Only data is written.

Run:  python tools/gen_golden_trainer.py        (needs the reference checkout; CPU only, a few minutes)
"""
from __future__ import annotations

import json
import math
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import trainer_util as U  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = ROOT / "tests" / "golden"
MAX_BYTES = 600 * 1024
MAX_GAP = 1e-2
MAX_TRIES = 60


def build(ref, sae_type: str, cfg: dict, seed: int, dtype):
    D, H = cfg["input_dim"], cfg["hidden_dim"]
    if sae_type == "t_sae":
        model = ref.TernarySparseAutoencoder(D, H)
    elif sae_type == "bl_sae":
        model = ref.BinaryLatentSAE(D, H)
    elif sae_type == "b_sae":
        model = ref.BinarySAE(D, H, cfg["n_bits"])
    elif sae_type == "q_sae":
        model = ref.QuantizedMatryoshkaSAE(D, H, cfg["top_k"], cfg["gamma"], cfg["n_bits"])
    elif sae_type == "rq_sae":
        model = ref.ResidualQuantizedSAE(D, H, cfg["top_k"], cfg["gamma"], cfg["n_bits"])
    else:
        model = ref.BaselineSparseAutoencoder(D, H)
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in U.epoch_params(sae_type, seed).items()}, strict=False)
    assert not missing.unexpected_keys, missing
    if sae_type == "t_sae":
        model.decoder.init_mask(U.T_SPARSITY)
    return model.to(dtype)


def step(sae_type: str, model, optimizer, batch, cfg: dict, f_decay):
    """One step of training/trainer.py:88-173 -> loss_total as a float"""
    if sae_type == "q_sae":
        latent_group, recon_groups = model(batch)
        optimizer.zero_grad(set_to_none=True)
        loss, _ = U.recipe_loss(sae_type, (latent_group, recon_groups), batch, cfg)
        loss.backward()
        model.decoder.apply_secant_grad()
        optimizer.step()
    elif sae_type == "rq_sae":
        outputs = model(batch)
        optimizer.zero_grad(set_to_none=True)
        loss, _ = U.recipe_loss(sae_type, outputs, batch, cfg)
        loss.backward()
        model.apply_secant_grad()
        optimizer.step()
    else:
        outputs = model(batch)
        loss, _ = U.recipe_loss(sae_type, outputs, batch, cfg)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if sae_type == "t_sae":
            model.decoder.mask_grad()
        optimizer.step()
        if sae_type == "t_sae":
            model.decoder.update_mask(f_decay, U.T_SPARSITY)
        elif sae_type == "baseline_sae":
            model.normalize_decoder_weights()
    return float(loss.item())


class keep_double:
    """The reference's BinarySAE decoder calls ``.float()`` on its soft integer weights (sae/binary.py:35), which a model in
    fp64 cannot multiply with; inside this block ``.float()`` leaves an fp64 tensor as it is."""

    def __enter__(self):
        self.orig = orig = torch.Tensor.float
        torch.Tensor.float = lambda t, *a, **k: t if t.dtype == torch.float64 else orig(t, *a, **k)

    def __exit__(self, *exc):
        torch.Tensor.float = self.orig
        return False


def run(ref, sae_type: str, seed: int, files, dtype):
    """-> (batch indices per epoch, losses): train() over the chunk files with the reference's loop"""
    if dtype == torch.float64:
        with keep_double():
            return run(ref, sae_type, seed, files, None)
    dtype = dtype or torch.float64
    cfg = U.epoch_config()
    model = build(ref, sae_type, cfg, seed, dtype)
    torch.manual_seed(seed)
    idx, losses = [], []
    for epoch, f in enumerate(files):
        dataset = ref.dataset.HiddenStatesTorchDataset(str(f))
        f_decay = None
        if sae_type == "t_sae":
            f_decay = 0.3 / 2 * (1 + math.cos(epoch * math.pi / len(files)))
            model.decoder.update_mask(f_decay, U.T_SPARSITY)
        optimizer = torch.optim.Adam(model.parameters(), lr=cfg["lr"])
        batch_idx, kept = 0, []
        for batch in DataLoader(dataset, batch_size=cfg["batch_size"], shuffle=True, num_workers=0):
            batch_idx += 1
            if torch.isnan(batch).any():
                continue
            kept.append(batch_idx)
            losses.append(step(sae_type, model, optimizer, batch.to(dtype), cfg, f_decay))
        idx.append(kept)
    return idx, np.array(losses, np.float64), sorted(model.state_dict().keys())


def main():
    ref = load_reference()
    E = U.EPOCH
    seed = E["seed"]
    for _ in range(MAX_TRIES):
        with tempfile.TemporaryDirectory() as tmp:
            files = [Path(tmp) / U.CHUNK_NAME, Path(tmp) / U.CHUNK_NAME_2]
            for f in files:
                torch.save(U.epoch_chunk(seed), f)
            results, worst = {}, 0.0
            for t in U.TYPES:
                i32, l32, keys = run(ref, t, seed, files, torch.float32)
                i64, l64, _ = run(ref, t, seed, files, torch.float64)
                assert i32 == i64 and len(l64) == sum(len(k) for k in i64)
                gap = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
                results[t] = (i64, l32, l64, gap, keys)
                worst = max(worst, gap)
                print(f"  seed {seed} {t}: loss {l64[0]:.5f} -> {l64[-1]:.5f}  gap {gap:.3g}  batches {i64}")
                if gap >= MAX_GAP or not l64[-1] < l64[0]:
                    worst = float("inf")
                    break
        if worst < MAX_GAP:
            break
        seed += 1000
    assert worst < MAX_GAP, "no seed found"
    meta = dict(E, seed=seed, types={}, state_dict_keys={})
    arrays = {}
    for t, (idx, l32, l64, gap, keys) in results.items():
        meta["types"][t] = {"batch_idx": idx, "gap": gap, "bound": max(10.0 * gap, 1e-5)}
        meta["state_dict_keys"][t] = keys
        arrays[f"{t}.loss32"], arrays[f"{t}.loss64"] = l32, l64
    path = OUT / f"{U.EPOCH_FIXTURE}.npz"
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    size = path.stat().st_size
    assert size <= MAX_BYTES, f"{path.name} is {size} bytes"
    print(f"wrote {path.name}: {size / 1024:.1f} KiB, seed {seed}, worst gap {worst:.3g}")


if __name__ == "__main__":
    main()
