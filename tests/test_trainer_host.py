"""The Trainer's host surface; runs without a GPU: the four new C-ABI entry points and their argument checks, the dispatcher
schemas, epoch_permutation against the reference's DataLoader, the skip planning from a bitmap and a permutation, the
checkpoint names, the constructor's and the CPU-tensor refusals, and the numpy / torch restatement of the loss kernel pinned
to torch's fp64 autograd on the six recipes of training/trainer.py:88-173."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import quantizedsae_amd
import trainer_util as U
from quantizedsae_amd import _lib, training
from quantizedsae_amd import torch_ops  # noqa: F401  (registers torch.ops.qsae.*)
from quantizedsae_amd.training import ShuffledChunk, Trainer, epoch_permutation, model_path_for, plan_epoch, trainer_loss

ROOT = Path(__file__).resolve().parents[1]
P = ctypes.c_void_p
NEW = ("qsae_rows_nan_bitmap", "qsae_gather_rows", "qsae_trainer_loss_workspace_bytes", "qsae_trainer_loss")


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """these tests run autograd; a test that ran earlier in the session may have left grad mode off"""
    with torch.enable_grad():
        yield


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.load().qsae_abi_version() == _lib.ABI_VERSION == 4
    assert "trainer.hip" in __import__("quantizedsae_amd.build", fromlist=["SOURCES"]).SOURCES
    assert quantizedsae_amd.Trainer is Trainer and quantizedsae_amd.training is training
    for name in ("Trainer", "ShuffledChunk", "epoch_permutation", "plan_epoch", "trainer_loss"):
        assert name in training.__all__


def test_invalid_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    a, odd = P(4096), P(4096 + 2)
    # rows_nan_bitmap
    assert lib.qsae_rows_nan_bitmap(None, 1, 0, 64, None, None) == _lib.OK                   # nothing to do, nothing launched
    assert lib.qsae_rows_nan_bitmap(a, 1, -1, 64, a, None) == _lib.ERR_INVALID_ARG
    assert b"invalid argument" in lib.qsae_last_error() and b"qsae_rows_nan_bitmap" in lib.qsae_last_error()
    assert lib.qsae_rows_nan_bitmap(a, 1, 8, 0, a, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_rows_nan_bitmap(None, 1, 8, 64, a, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_rows_nan_bitmap(a, 1, 8, 64, None, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_rows_nan_bitmap(a, 3, 8, 64, a, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_rows_nan_bitmap(odd, 0, 8, 64, a, None) == _lib.ERR_INVALID_ARG           # fp32 at a 2-byte offset
    assert lib.qsae_rows_nan_bitmap(a, 1, 32 * (2 ** 31 - 1) + 1, 64, a, None) == _lib.ERR_UNSUPPORTED
    # gather_rows
    assert lib.qsae_gather_rows(None, 1, 8, 64, None, 0, None, None, None) == _lib.OK
    assert lib.qsae_gather_rows(a, 1, 8, 64, a, -1, a, a, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_gather_rows(a, 1, -1, 64, a, 4, a, a, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_gather_rows(a, 1, 8, 0, a, 4, a, a, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_gather_rows(a, 7, 8, 64, a, 4, a, a, None) == _lib.ERR_UNSUPPORTED
    for k in range(4):                                                                        # src, idx, out, flag
        args = [a, a, a, a]
        args[k] = None
        assert lib.qsae_gather_rows(args[0], 1, 8, 64, args[1], 4, args[2], args[3], None) == _lib.ERR_INVALID_ARG, k
    assert lib.qsae_gather_rows(a, 1, 8, 64, P(4096 + 4), 4, a, a, None) == _lib.ERR_INVALID_ARG   # idx off its 8 bytes
    # trainer_loss
    ptrs = (P * 8)(*[4096] * 8)
    assert lib.qsae_trainer_loss(None, None, 0, 4, 8, 0, 0.5, None, None, None, 0, None) == _lib.OK
    assert lib.qsae_trainer_loss(None, None, 4, 0, 8, 0, 0.5, None, None, None, 0, None) == _lib.OK
    assert lib.qsae_trainer_loss(a, ptrs, -1, 4, 8, 0, 0.5, ptrs, a, a, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_trainer_loss(a, ptrs, 4, 4, 0, 0, 0.5, ptrs, a, a, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_trainer_loss(a, ptrs, 9, 4, 8, 0, 0.5, ptrs, a, a, 1 << 20, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_trainer_loss(a, ptrs, 4, 4, 8, 2, 0.5, ptrs, a, a, 1 << 20, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_trainer_loss(None, ptrs, 4, 4, 8, 0, 0.5, ptrs, a, a, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_trainer_loss(a, None, 4, 4, 8, 0, 0.5, ptrs, a, a, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_trainer_loss(a, ptrs, 4, 4, 8, 0, 0.5, None, a, a, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_trainer_loss(a, ptrs, 4, 4, 8, 0, 0.5, ptrs, None, a, 1 << 20, None) == _lib.ERR_INVALID_ARG
    holed = (P * 8)(*[4096, 0, 4096, 4096, 4096, 4096, 4096, 4096])
    assert lib.qsae_trainer_loss(a, holed, 4, 4, 8, 0, 0.5, ptrs, a, a, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_trainer_loss(a, holed, 1, 4, 8, 0, 0.5, ptrs, a, None, 0, None) == _lib.ERR_WORKSPACE   # (level 1 not read)
    assert lib.qsae_trainer_loss(a, ptrs, 4, 4, 8, 0, 0.5, ptrs, a, a, 8, None) == _lib.ERR_WORKSPACE
    assert b"qsae_trainer_loss_workspace_bytes" in lib.qsae_last_error()
    # the helper: n * ceil(B D / 4096) * 8 rounded up to 256, 0 for an invalid shape
    assert lib.qsae_trainer_loss_workspace_bytes(4, 8192, 512) == 4 * 1024 * 8
    assert lib.qsae_trainer_loss_workspace_bytes(1, 1, 1) == 256 and lib.qsae_trainer_loss_workspace_bytes(8, 257, 36) == 256
    assert lib.qsae_trainer_loss_workspace_bytes(9, 4, 8) == 0 and lib.qsae_trainer_loss_workspace_bytes(4, 4, 0) == 0


def test_op_schemas_and_fakes_are_registered():
    def written(op):
        return [a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    assert written(torch.ops.qsae.rows_nan_bitmap) == []
    assert written(torch.ops.qsae.gather_rows) == ["flag"]
    assert written(torch.ops.qsae.trainer_loss) == ["grads"]
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        chunk = torch.empty(6, 50, 64, dtype=torch.float16)
        bits = torch.ops.qsae.rows_nan_bitmap(chunk)
        assert bits.shape == (10,) and bits.dtype == torch.int32
        out = torch.ops.qsae.gather_rows(chunk, torch.empty(17, dtype=torch.int64), torch.empty(1, dtype=torch.int32))
        assert out.shape == (17, 64) and out.dtype == torch.float32
        x = torch.empty(17, 64)
        losses = torch.ops.qsae.trainer_loss(x, [x, x, x], 1, 0.5, torch.empty(3, 17, 64))
        assert losses.shape == (3,) and losses.dtype == torch.float32


@pytest.mark.parametrize("n,batch", [(23, 8), (1000, 64), (257, 256)])
def test_epoch_permutation_is_the_dataloaders_order(n, batch):
    for seed in (0, 17):
        torch.manual_seed(seed)
        theirs = [int(v) for b in DataLoader(list(range(n)), batch_size=batch, shuffle=True, num_workers=0) for v in b]
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        ours = epoch_permutation(n)
        assert ours.dtype == torch.int64 and ours.tolist() == theirs
        assert torch.equal(torch.get_rng_state(), state)                 # the default RNG is where the loader leaves it
        assert epoch_permutation(n).tolist() != theirs                   # and the next epoch is another order
    assert epoch_permutation(0).numel() == 0
    with pytest.raises(ValueError):
        epoch_permutation(-1)


def test_skip_planning_from_a_bitmap_and_a_permutation():
    n, bs = 300, 64
    bits = np.zeros(10, np.int32)
    bits[123 >> 5] |= 1 << (123 & 31)
    perm = np.arange(n)
    plan = plan_epoch(perm, bits, bs)
    assert plan.skipped == [2] and plan.batches == [(1, 0, 64), (3, 128, 192), (4, 192, 256), (5, 256, 300)]
    torch.manual_seed(1)
    perm = epoch_permutation(n).numpy()
    plan = plan_epoch(perm, bits, bs)
    where = int(np.flatnonzero(perm == 123)[0]) // bs + 1
    assert plan.skipped == [where] and [i for i, _, _ in plan.batches] == [i for i in range(1, 6) if i != where]
    assert plan.batches[-1][2] == n or where == 5
    # the sign bit of a word (row 31), the last row, several NaN rows in one batch, every batch skipped, no NaN at all
    bits = np.zeros(10, np.uint32)
    bits[0] = 1 << 31
    bits[9] = 1 << (299 & 31)
    assert plan_epoch(np.arange(n), bits.view(np.int32), bs).skipped == [1, 5]
    bits[:] = 0xFFFFFFFF
    assert plan_epoch(np.arange(n), bits, bs).batches == []
    assert plan_epoch(np.arange(n), np.zeros(10, np.int32), 300).batches == [(1, 0, 300)]
    assert plan_epoch(np.arange(0), np.zeros(0, np.int32), 8) == ([], [])
    with pytest.raises(ValueError):
        plan_epoch(np.arange(n), np.zeros(9, np.int32), bs)              # too few words
    with pytest.raises(ValueError):
        plan_epoch(np.arange(n) + 1, bits, bs)                           # not an order of the chunk's rows
    with pytest.raises(ValueError):
        plan_epoch(np.arange(n), bits, 0)


CONFIG = {"input_dim": 64, "n_bits": 4, "hidden_dim": 1024, "gamma": 1.5, "epochs": 1, "lr": 1e-4, "top_k": 32,
          "sparsity_lambda": 1.5e-3, "polarize_lambda": 1e-2, "batch_size": 64}


@pytest.mark.parametrize("sae_type", U.TYPES)
def test_model_path_is_the_references(sae_type, tmp_path):
    for rigL in (False, True):
        bits = "4_bits" if sae_type in ("b_sae", "q_sae", "rq_sae") else ""
        want = "SAEs/" + sae_type + "_1024" + ("_rigL" if rigL else "") + bits + ".pth"
        assert model_path_for("SAEs/", sae_type, CONFIG, rigL) == want
        if sae_type == "t_sae" and not rigL:
            continue
        if rigL and sae_type != "t_sae":
            continue                                                     # (model_path_for covers the name; rigL needs a decoder mask)
        t = Trainer(CONFIG, sae_type, rigL, True, dataset_dir=str(tmp_path), save_dir="SAEs/")
        assert t.model_path == want and t.chunk_files == [] and t.sae_type == sae_type and t.rigL is rigL


def test_constructor_keeps_the_references_calls_and_refuses_what_cannot_train(tmp_path):
    from quantizedsae_amd import BinarySAE
    with pytest.raises(ValueError, match="rigL"):
        Trainer(CONFIG, "t_sae", False, True, dataset_dir=str(tmp_path))
    with pytest.raises(ValueError, match="unknown sae_type"):
        Trainer(CONFIG, "x_sae", False, True, dataset_dir=str(tmp_path))
    with pytest.raises(ValueError, match="log_every"):
        Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), log_every=0)
    with pytest.raises(FileNotFoundError):
        Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path / "missing"))
    # BinarySAE(input_dim, hidden_dim, n_bits): n_bits lands in gamma, the decoder keeps its default of 8 bits
    t = Trainer(CONFIG, "b_sae", False, True, dataset_dir=str(tmp_path))
    assert t.model.n_bits == 8 and t.model.decoder.weight.shape == (1024, 64 * 8)
    assert torch.allclose(t.scale_factor.cpu(), torch.tensor([1.0, 2.0, 4.0, 8.0]) / 15)
    mine = BinarySAE(64, 1024, gamma=1.5, n_bits=4)
    assert Trainer(CONFIG, "b_sae", False, True, dataset_dir=str(tmp_path), model=mine).model is mine
    q = Trainer(CONFIG, "q_sae", False, True, dataset_dir=str(tmp_path)).model
    assert (q.n_bits, q.abs_range, q.top_k) == (4, 1.5, 32)
    # the chunk-file filter, in sorted order
    for name in ("the_pile_hidden_states_L3_10.pt", "the_pile_hidden_states_L3_2.pt", "the_pile_hidden_states_L4_1.pt",
                 "the_pile_hidden_states_L3_3.txt"):
        (tmp_path / name).write_bytes(b"")
    t = Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path))
    assert t.chunk_files == ["the_pile_hidden_states_L3_10.pt", "the_pile_hidden_states_L3_2.pt"]
    assert (t.connection_fraction_to_update, t.f_decay, t.epoch, t.no_log) == (0.3, None, 0, True)


def test_a_trainer_without_a_gpu_refuses_to_train(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    torch.save(torch.zeros(2, 8, 64, dtype=torch.float16), tmp_path / "the_pile_hidden_states_L3_0.pt")
    t = Trainer(CONFIG, "baseline_sae", False, True, dataset_dir=str(tmp_path), save_dir=str(tmp_path / "out"))
    assert t.device.type == "cpu" and len(t.chunk_files) == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.one_epoch(torch.zeros(2, 8, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.train()
    assert not (tmp_path / "out").exists()                               # nothing was saved


def test_cpu_tensors_are_refused_by_the_ops_and_the_batch_supply():
    x = torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.qsae.rows_nan_bitmap(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.qsae.gather_rows(x, torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.qsae.trainer_loss(x, [x], 0, 0.5, torch.zeros(1, 4, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer_loss("baseline_sae", (x, x.clone().requires_grad_(True)), x, CONFIG)
    with pytest.raises(ValueError, match="unknown sae_type"):
        trainer_loss("x_sae", (x, x), x, CONFIG)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ShuffledChunk(torch.zeros(2, 8, 64), 8, "cpu")
    with pytest.raises(TypeError, match="fp32, fp16 and bf16"):
        ShuffledChunk(torch.zeros(2, 8, 64, dtype=torch.float64), 8, "cuda")
    with pytest.raises(TypeError):
        ShuffledChunk([1, 2, 3], 8, "cuda")
    with pytest.raises(ValueError, match="batch_size"):
        ShuffledChunk(torch.zeros(2, 8, 64), 0, "cuda")


# ---- the restatement of the loss kernel, pinned to torch's fp64 autograd on the six recipes ---------------------------------
@pytest.mark.parametrize("sae_type", U.TYPES)
def test_the_loss_restatement_agrees_with_fp64_autograd_on_the_reference_recipe(sae_type):
    from quantizedsae_amd.training import recon_recipe
    B, D, n = 63, 36, 5 if sae_type == "rq_sae" else 4
    cfg = dict(CONFIG, n_bits=n)
    levels = n if sae_type in ("q_sae", "rq_sae") else 1
    x, recons = U.loss_case(B, D, levels, seed=21)
    mode, coef = recon_recipe(sae_type)
    assert (mode, coef) == {"q_sae": (0, 0.5), "rq_sae": (1, 0.5), "b_sae": (0, 0.5)}.get(sae_type, (0, 1.0))
    got_l, got_g = U.loss_ref(x, recons, mode, coef)
    # the recipe in torch, fp64, on the same numbers
    xb = torch.from_numpy(x).double()
    leaves = [torch.from_numpy(r).double().requires_grad_(True) for r in recons]
    groups = [torch.tensor(0.1 * (i + 1), dtype=torch.float64, requires_grad=True) for i in range(levels)]
    pol = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    if sae_type in ("q_sae", "rq_sae"):
        outputs = (groups, leaves)
    elif sae_type == "b_sae":
        outputs = (None, leaves[0], pol)
    else:
        outputs = (None, leaves[0])
    total, level_losses = U.recipe_loss(sae_type, outputs, xb, cfg)
    total.backward()
    assert np.allclose(got_l, [float(v.detach()) for v in level_losses], rtol=2.0 ** -21, atol=0)
    for i, leaf in enumerate(leaves):
        want = leaf.grad.numpy()
        # as in tests/test_trainer_gpu.py: 2^-22 relative against the level's own fp32 target; against the fp64 chain of
        # rq_sae the targets' own rounding adds 2^-24 of their size per level, bounded normwise
        atol = 2.0 ** -20 * float(np.abs(want).max()) if sae_type == "rq_sae" else 2.0 ** -149
        assert np.all(np.abs(got_g[i].astype(np.float64) - want) <= 2.0 ** -22 * np.abs(want) + atol), i
    if sae_type == "q_sae":
        assert all(abs(float(g.grad) - cfg["sparsity_lambda"]) < 1e-15 for g in groups)
    if sae_type == "rq_sae":
        assert [round(float(g.grad) / cfg["sparsity_lambda"], 9) if g.grad is not None else None for g in groups] == [1.0, 2.5, 4.0, 8.0, None]
        assert training.RQ_STAGE_WEIGHTS == U.RQ_WEIGHTS
    if sae_type == "b_sae":
        assert abs(float(pol.grad) - cfg["polarize_lambda"]) < 1e-15
    # and the order of the sum is the documented one whatever the size: against a plain fp64 sum
    big = np.abs(U.S.normal(4, (300000,), stream=6)).astype(np.float32)
    assert abs(float(U.ordered_sum(big)) - float(np.sum(big.astype(np.float64)))) <= 1e-12 * float(np.sum(big.astype(np.float64)))
