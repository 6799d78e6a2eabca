"""What the trainer tests share: the numpy / torch restatements of the three kernels of csrc/trainer.hip (the GPU and the
emulation tests compare with them bit for bit), the six loss recipes of training/trainer.py:88-173 as torch code, and the
recipe of tests/golden/trainer_epoch.npz (tools/gen_golden_trainer.py writes it, tests/test_trainer_gpu.py replays it)."""
import json
import math
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from quantizedsae_amd import synthetic as S

GOLDEN = Path(__file__).resolve().parent / "golden"
TYPES = ("t_sae", "bl_sae", "b_sae", "q_sae", "rq_sae", "baseline_sae")
TORCH_DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
DTYPE_CODES = {"fp32": 0, "fp16": 1, "bf16": 2}
RQ_WEIGHTS = (1.0, 2.5, 4.0, 8.0)

# kernel shapes (the issue's lists)
GATHER_ROWS, GATHER_D, GATHER_B = (1, 300, 4099), (1, 5, 64, 512), (1, 64, 257)
BITMAP_ROWS = (1, 31, 32, 33, 4099)
LOSS_SHAPES = ((1, 1), (63, 4), (257, 36), (256, 64))
LOSS_LEVELS = (1, 4, 8)
LOSS_BLOCK, LOSS_THREADS = 4096, 256        # elements of one workgroup of qsae_trainer_loss, threads of a workgroup


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- chunks ---------------------------------------------------------------------------------------------------------------
def special_chunk(n_rows: int, D: int, dtype: str, seed: int = 3) -> torch.Tensor:
    """[n_rows, D] in the stored dtype: normal values with NaN (two payloads), +-inf, -0, the smallest and largest
    subnormal and the largest finite value planted at fixed flat positions (as far as the chunk has room)."""
    dt = TORCH_DTYPES[dtype]
    x = torch.from_numpy(S.normal(seed, (n_rows, D), stream=2)).to(dt)
    flat = x.reshape(-1)
    if dtype == "fp32":
        bits = flat.view(torch.int32)
        plants = [0x7FC00000, 0x7FC01234, 0x7F800000, 0xFF800000 - (1 << 32), 0x80000000 - (1 << 32), 0x00000001, 0x007FFFFF,
                  0x7F7FFFFF]
    elif dtype == "fp16":
        bits = flat.view(torch.int16)
        plants = [0x7E00, 0x7E01, 0x7C00, 0xFC00 - (1 << 16), 0x8000 - (1 << 16), 0x0001, 0x03FF, 0x7BFF]
    else:
        bits = flat.view(torch.int16)
        plants = [0x7FC0, 0x7FC1, 0x7F80, 0xFF80 - (1 << 16), 0x8000 - (1 << 16), 0x0001, 0x007F, 0x7F7F]
    n = flat.numel()
    for j, p in enumerate(plants):
        pos = (j * 37 + 5) % n if n > len(plants) else j
        if pos < n:
            bits[pos] = p
    return x


def widen_exact(src: torch.Tensor) -> np.ndarray:
    """The exact fp32 image of every stored value, from the bits: fp32 as it is, bf16 shifted up by 16, fp16 by numpy's
    conversion (which keeps a NaN's sign and payload, as the GPU's conversion does for quiet NaNs).  Equal to torch's
    ``.float()`` on the CPU -- the reference's widening -- wherever the value is not a NaN (asserted); torch's CPU
    conversion maps every fp16 NaN to one pattern of its own."""
    if src.dtype == torch.float32:
        out = src.numpy().copy()
    elif src.dtype == torch.bfloat16:
        out = (src.contiguous().view(torch.int16).numpy().view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    else:
        out = src.contiguous().view(torch.int16).numpy().view(np.float16).astype(np.float32)
    theirs = src.float().numpy()
    keep = ~np.isnan(theirs)
    assert np.array_equal(np.isnan(out), ~keep) and np.array_equal(out.view(np.uint32)[keep], theirs.view(np.uint32)[keep])
    return out


def gather_ref(src: torch.Tensor, idx) -> np.ndarray:
    """out[b] = float(src[idx[b]]), the exact widening; rows of zeros for indices outside the chunk."""
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < src.shape[0])
    out = np.zeros((idx.size, src.shape[1]), np.float32)
    if ok.any():
        out[ok] = widen_exact(src)[idx[ok]]
    return out


def gather_indices(n_rows: int, B: int, seed: int = 1) -> np.ndarray:
    """B indices holding 0, n_rows - 1 and a repeat, otherwise hashed"""
    idx = (S.hash_u64(seed, B, stream=4) % np.uint64(n_rows)).astype(np.int64)
    idx[0] = 0
    if B > 1:
        idx[-1] = n_rows - 1
    if B > 3:
        idx[2] = idx[1]
    return idx


def nan_bitmap_ref(src: torch.Tensor) -> np.ndarray:
    rows = torch.isnan(src.float()).any(dim=1).numpy()
    words = np.zeros(((rows.size + 31) // 32,), np.uint32)
    for r in np.flatnonzero(rows):
        words[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return words


# ---- qsae_trainer_loss ------------------------------------------------------------------------------------------------------
def _butterfly(v: np.ndarray) -> np.ndarray:
    """[..., 64] lane values -> the lanes after the xor 32, 16, ..., 1 exchange-and-add"""
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ m]
    return v


def _block_add(acc: np.ndarray) -> np.ndarray:
    """[..., 256] thread sums (fp64) -> [...]: butterfly per wave, then the 4 wave sums in ascending order"""
    w = _butterfly(acc.reshape(acc.shape[:-1] + (4, 64)))[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def ordered_sum(sq: np.ndarray) -> np.float64:
    """The fp64 sum of the fp32 terms ``sq`` (flat) in the order of qsae_trainer_loss (include/qsae.h)."""
    sq = np.asarray(sq, np.float32).reshape(-1)
    N = sq.size
    nb = (N + LOSS_BLOCK - 1) // LOSS_BLOCK
    v = np.zeros((nb * LOSS_BLOCK,), np.float64)
    v[:N] = sq
    v = v.reshape(nb, LOSS_BLOCK // (4 * LOSS_THREADS), LOSS_THREADS, 4)
    acc = np.zeros((nb, LOSS_THREADS), np.float64)
    for k in range(v.shape[1]):
        for j in range(4):
            acc = acc + v[:, k, :, j]
    partials = _block_add(acc)
    rounds = (nb + LOSS_THREADS - 1) // LOSS_THREADS
    p = np.zeros((rounds * LOSS_THREADS,), np.float64)
    p[:nb] = partials
    acc = np.zeros((LOSS_THREADS,), np.float64)
    for row in p.reshape(rounds, LOSS_THREADS):
        acc = acc + row
    return np.float64(_block_add(acc))


def loss_targets(x: np.ndarray, recons, mode: int):
    """The fp32 target of every level: x, or the rq_sae chain t_{i+1} = fl(fl(t_i - r_i) * 2)"""
    t, out = np.asarray(x, np.float32), []
    for r in recons:
        out.append(t)
        if mode == 1:
            t = ((t - r).astype(np.float32) * np.float32(2.0)).astype(np.float32)
    return out


def loss_ref(x: np.ndarray, recons, mode: int, coef: float):
    """-> (losses fp32 [n], grads [n] of fp32 [B, D]): qsae_trainer_loss operation by operation"""
    N = x.size
    s = np.float32(2.0 * coef / N)
    losses, grads = [], []
    with np.errstate(all="ignore"):
        for r, t in zip(recons, loss_targets(x, recons, mode)):
            d = (r - t).astype(np.float32)
            grads.append((d * s).astype(np.float32))
            S_i = ordered_sum((d * d).astype(np.float32))
            losses.append(np.float32((np.float64(coef) * S_i) / np.float64(N)))
    return np.array(losses, np.float32), grads


def loss_f64(x: np.ndarray, recons, mode: int, coef: float):
    """The same quantities in fp64 from the fp32 inputs of every level (r_i and the fp32 target t_i)"""
    N = x.size
    losses, grads = [], []
    for r, t in zip(recons, loss_targets(x, recons, mode)):
        d = r.astype(np.float64) - t.astype(np.float64)
        grads.append(d * (2.0 * coef / N))
        losses.append(coef * math.fsum((d * d).reshape(-1).tolist()) / N)
    return np.array(losses, np.float64), grads


def loss_case(B: int, D: int, n: int, seed: int = 7, equal_level: int = None):
    """x and n reconstructions fp32 [B, D]; ``equal_level``: that level equals its mode-0 target bit for bit"""
    x = S.normal(seed, (B, D), stream=1)
    recons = [(x * np.float32(0.5 ** i) + S.normal(seed, (B, D), stream=10 + i, std=0.3)).astype(np.float32) for i in range(n)]
    if equal_level is not None:
        recons[equal_level] = x.copy()
    return x, recons


# ---- the six recipes as the reference writes them (training/trainer.py:88-173) -----------------------------------------------
def recipe_loss(sae_type: str, outputs, batch: torch.Tensor, config: dict):
    """-> (loss_total, per-level reconstruction losses): the reference's torch code, for autograd"""
    if sae_type == "q_sae":
        latent_group, recon_groups = outputs
        recon_losses = [0.5 * F.mse_loss(recon, batch) for recon in recon_groups]
        return sum(recon_losses) + sum(latent_group) * config["sparsity_lambda"], recon_losses
    if sae_type == "rq_sae":
        latent_group, recon_group = outputs
        residual, recon_losses, sparsity_loss = batch, [], 0
        for i, recon in enumerate(recon_group):
            recon_losses.append(0.5 * F.mse_loss(recon, residual))
            residual = (residual - recon).detach() * 2
            if i < 4:
                sparsity_loss = sparsity_loss + latent_group[i] * config["sparsity_lambda"] * RQ_WEIGHTS[i]
        return sum(recon_losses) + sparsity_loss, recon_losses
    if sae_type == "b_sae":
        _latent, reconstruction, polarize_loss = outputs
        recon_loss = 0.5 * F.mse_loss(reconstruction, batch)
        return recon_loss + config["polarize_lambda"] * polarize_loss, [recon_loss]
    loss = F.mse_loss(outputs[1], batch)
    return loss, [loss]


def fake_outputs(sae_type: str, batch: torch.Tensor, n_bits: int, seed: int = 0, on_device: bool = False):
    """Leaf tensors in the layout of the type's forward_train outputs -> (outputs, leaves that the loss should reach,
    leaves it should not).  The values are fp32 numbers from ``seed`` whatever the dtype of ``batch``; ``on_device``: drawn
    on the batch's device instead (no copy from the host, which would wait for the device)."""
    g = torch.Generator().manual_seed(seed)
    dev, dt = batch.device, batch.dtype

    def leaf(*shape):
        if on_device:
            return torch.randn(shape, dtype=dt, device=dev).requires_grad_(True)
        return (torch.randn(shape, generator=g, dtype=torch.float32).to(dt).to(dev)).requires_grad_(True)
    B, D = batch.shape
    if sae_type in ("q_sae", "rq_sae"):
        groups = [leaf() for _ in range(n_bits)]
        recons = [leaf(B, D) for _ in range(n_bits)]
        reached = recons + (groups if sae_type == "q_sae" else groups[:4])
        return (groups, recons), reached, ([] if sae_type == "q_sae" else groups[4:])
    recon, latent = leaf(B, D), leaf(B, 8)
    if sae_type == "b_sae":
        pol = leaf()
        return (latent, recon, pol), [recon, pol], [latent]
    return (latent, recon), [recon], [latent]


# ---- the epoch fixture ---------------------------------------------------------------------------------------------------------
EPOCH_FIXTURE = "trainer_epoch"
EPOCH = dict(contexts=6, tokens=50, D=64, H=1024, batch_size=64, epochs=2, n_bits=4, gamma=1.5, top_k=32, lr=3e-3,
             sparsity_lambda=1.5e-3, polarize_lambda=1e-2, nan_row=123, seed=4100, f_decay=0.3)
CHUNK_NAME, CHUNK_NAME_2 = "the_pile_hidden_states_L3_0.pt", "the_pile_hidden_states_L3_1.pt"     # two files: two epochs
T_SPARSITY = 0.7                                 # init_mask(0.7) / update_mask(f_decay, 0.7) of the t_sae trainer


def epoch_config() -> dict:
    E = EPOCH
    return {"input_dim": E["D"], "n_bits": E["n_bits"], "hidden_dim": E["H"], "gamma": E["gamma"], "epochs": 1, "lr": E["lr"],
            "top_k": E["top_k"], "sparsity_lambda": E["sparsity_lambda"], "polarize_lambda": E["polarize_lambda"],
            "batch_size": E["batch_size"]}


def epoch_chunk(seed: int) -> torch.Tensor:
    """The fixture's chunk, fp16 [contexts, tokens, D] with one NaN planted in row ``nan_row``"""
    E = EPOCH
    x = torch.from_numpy(S.activations(seed, E["contexts"] * E["tokens"], E["D"])).to(torch.float16)
    x[E["nan_row"], 7] = float("nan")
    return x.reshape(E["contexts"], E["tokens"], E["D"])


def _blatent_params(seed: int, D: int, H: int) -> dict:
    return {"encoder.0.weight": S.xavier_uniform(seed, H, D, stream=0), "encoder.0.bias": S.normal(seed, (H,), stream=1, std=0.05),
            "decoder.weight": S.uniform(seed, (D, H), -H ** -0.5, H ** -0.5, stream=2),
            "decoder.bias": S.normal(seed, (D,), stream=3, std=0.05)}


def epoch_params(sae_type: str, seed: int) -> dict:
    """Initial state dict (numpy) of the type's model at the fixture's shape, from the portable PRNG recipes"""
    E = EPOCH
    D, H = E["D"], E["H"]
    if sae_type == "b_sae":
        return S.binary_sae_params(seed, D, H, 8, dec_bias_std=0.05, logit_std=(2.0 / (D * 8)) ** 0.5)   # 8 bits: the constructor call's default
    if sae_type == "baseline_sae":
        return S.baseline_sae_params(seed, D, H)
    if sae_type == "t_sae":
        return S.ternary_sae_params(seed, D, H)
    if sae_type == "bl_sae":
        return _blatent_params(seed, D, H)
    import train_matryoshka_util as M
    if sae_type == "q_sae":
        return M.q_params(seed, D, H, -2.5)
    return M.rq_params(seed, D, H, E["n_bits"], -2.5)


def load_epoch_fixture():
    with np.load(GOLDEN / f"{EPOCH_FIXTURE}.npz") as z:
        meta = json.loads(bytes(z["meta"]).decode())
        return meta, {k: z[k] for k in z.files if k != "meta"}
