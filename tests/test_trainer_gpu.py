"""The Trainer on the GPU (quantizedsae_amd.training, csrc/trainer.hip): the three kernels against the restatements of
tests/trainer_util.py bit for bit, the shuffled batch supply against the reference's DataLoader, the absence of host reads
in a step's loop-side work, and the whole loop against tests/golden/trainer_epoch.npz (the reference's models in a restated
one_epoch, fp64, on the CPU; tools/gen_golden_trainer.py)."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import trainer_util as U
from quantizedsae_amd import torch_ops as ops
from quantizedsae_amd.data import HiddenStatesTorchDataset
from quantizedsae_amd.training import ShuffledChunk, Trainer, trainer_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """these tests run autograd; a test that ran earlier in the session may have left grad mode off"""
    with torch.enable_grad():
        yield


def _np(t):
    return t.detach().cpu().numpy()


def _off_boundary(src: torch.Tensor) -> torch.Tensor:
    """src on the device, contiguous, starting one element past a 16-byte boundary"""
    flat = torch.empty(src.numel() + 1, dtype=src.dtype, device=DEV)
    flat[1:] = src.reshape(-1).to(DEV)
    out = flat[1:].view(src.shape)
    assert out.data_ptr() % 16 == src.element_size() and out.is_contiguous()
    return out


# ---- qsae_gather_rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(U.TORCH_DTYPES))
@pytest.mark.parametrize("D", U.GATHER_D)
def test_gather_rows_equals_the_exact_widening_bit_for_bit(dtype, D):
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for n_rows in U.GATHER_ROWS:
        src = U.special_chunk(n_rows, D, dtype)
        dsrc = src.to(DEV)
        for B in U.GATHER_B:
            idx = U.gather_indices(n_rows, B)
            out = ops.gather_rows(dsrc, torch.from_numpy(idx).to(DEV), flag)
            assert out.dtype == torch.float32 and tuple(out.shape) == (B, D)
            assert U.same_bits(_np(out), U.gather_ref(src, idx)), (n_rows, B)
    assert int(flag.item()) == 0
    # a chunk that starts one element off its 16-byte boundary takes the element-wise path: the same bits
    src = U.special_chunk(300, D, dtype)
    idx = U.gather_indices(300, 64)
    assert U.same_bits(_np(ops.gather_rows(_off_boundary(src), torch.from_numpy(idx).to(DEV), flag)), U.gather_ref(src, idx))


@pytest.mark.parametrize("dtype", list(U.TORCH_DTYPES))
def test_gather_rows_writes_zero_rows_for_indices_outside_the_chunk_and_sets_the_flag(dtype):
    for D in (5, 64):
        n_rows, B = 300, 64
        src = U.special_chunk(n_rows, D, dtype)
        idx = U.gather_indices(n_rows, B)
        idx[5], idx[9], idx[63] = -1, n_rows, 2 ** 40
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = _np(ops.gather_rows(src.to(DEV), torch.from_numpy(idx).to(DEV), flag))
        assert U.same_bits(out, U.gather_ref(src, idx))
        assert not out[5].any() and not out[9].any() and not out[63].any() and int(flag.item()) == 1


# ---- qsae_rows_nan_bitmap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(U.TORCH_DTYPES))
@pytest.mark.parametrize("n_rows", U.BITMAP_ROWS)
def test_rows_nan_bitmap_marks_exactly_the_rows_with_a_nan(dtype, n_rows):
    for D in (1, 5, 64, 512):
        base = torch.from_numpy(U.S.normal(n_rows, (n_rows, D), stream=3)).to(U.TORCH_DTYPES[dtype])
        base[n_rows // 2, 0] = float("inf")                                       # inf is not NaN
        assert not _np(ops.rows_nan_bitmap(base.to(DEV))).any()
        for where in {(0, 0), (0, D - 1), (n_rows - 1, 0), (n_rows - 1, D - 1)}:
            src = base.clone()
            src[where] = float("nan")
            got = _np(ops.rows_nan_bitmap(src.to(DEV))).view(np.uint32)
            want = U.nan_bitmap_ref(src)
            assert np.array_equal(got, want) and want[where[0] >> 5] == 1 << (where[0] & 31), (D, where)
    # a 3-d chunk, and one that starts off its 16-byte boundary
    src = U.special_chunk(6 * 50, 8, dtype)
    assert np.array_equal(_np(ops.rows_nan_bitmap(src.reshape(6, 50, 8).to(DEV))).view(np.uint32), U.nan_bitmap_ref(src))
    assert np.array_equal(_np(ops.rows_nan_bitmap(_off_boundary(src))).view(np.uint32), U.nan_bitmap_ref(src))


# ---- qsae_trainer_loss ------------------------------------------------------------------------------------------------------
# (2100, 512): more than 256 workgroups, so that a thread of the final pass adds more than one partial
LOSS_CASES = [(s, n) for s in U.LOSS_SHAPES for n in U.LOSS_LEVELS] + [((2100, 512), 4)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}_n{c[1]}")
def test_trainer_loss_equals_the_restatement_and_is_close_to_fp64(case, mode):
    (B, D), n = case
    for coef, shift, equal in ((0.5, 0, None), (1.0, 1, 0)):
        x, recons = U.loss_case(B, D, n, equal_level=equal)

        def dev(a):                                          # shift = 1: the tensor starts one element off its boundary
            buf = torch.empty(a.size + shift, dtype=torch.float32, device=DEV)
            buf[shift:] = torch.from_numpy(a.reshape(-1)).to(DEV)
            return buf[shift:].view(B, D)
        dx, dr = dev(x), [dev(r) for r in recons]
        assert dx.data_ptr() % 16 == (4 * shift) % 16
        losses, grads = ops.trainer_loss(dx, dr, mode, coef)
        again_l, again_g = ops.trainer_loss(dx, dr, mode, coef)
        assert torch.equal(losses.view(torch.int32), again_l.view(torch.int32))
        assert torch.equal(grads.view(torch.int32), again_g.view(torch.int32))            # two runs: the same bits
        want_l, want_g = U.loss_ref(x, recons, mode, coef)
        l64, g64 = U.loss_f64(x, recons, mode, coef)
        got_l, got_g = _np(losses), _np(grads)
        print(f"B={B} D={D} n={n} mode={mode} coef={coef} shift={shift}: max rel loss err "
              f"{float(np.max(np.abs(got_l - l64) / np.maximum(np.abs(l64), 1e-300))):.3e}")
        assert U.same_bits(got_l, want_l), (got_l, want_l)
        for i in range(n):
            assert U.same_bits(got_g[i], want_g[i]), i
            # three roundings (the difference, s, the product), each below 2^-24 relative, or an underflow of half the
            # smallest subnormal
            assert np.all(np.abs(got_g[i].astype(np.float64) - g64[i]) <= 2.0 ** -22 * np.abs(g64[i]) + 2.0 ** -149), i
        # every term is non-negative and carries three roundings, the sum is fp64, plus the final rounding
        assert np.all(np.abs(got_l.astype(np.float64) - l64) <= 2.0 ** -21 * np.abs(l64))
        if equal is not None:
            assert got_l[0] == 0 and not got_g[0].any()


def test_trainer_loss_refuses_what_it_cannot_take():
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError, match="1 to 8"):
        ops.trainer_loss(x, [x] * 9, 0, 0.5)
    with pytest.raises(ValueError, match="mode"):
        ops.trainer_loss(x, [x], 2, 0.5)
    with pytest.raises(ValueError, match="recons\\[0\\]"):
        ops.trainer_loss(x, [torch.zeros(4, 4, device=DEV)], 0, 0.5)
    with pytest.raises(TypeError):
        ops.trainer_loss(x.double(), [x], 0, 0.5)


# ---- ShuffledChunk -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("trainer_chunk") / U.CHUNK_NAME
    torch.save(U.epoch_chunk(U.EPOCH["seed"]), path)
    return path


def test_shuffled_chunk_hands_out_the_dataloaders_batches_without_the_nan_batch(chunk_file):
    bs = U.EPOCH["batch_size"]
    ds = HiddenStatesTorchDataset(chunk_file)
    chunk = ShuffledChunk(chunk_file, bs, DEV)
    assert len(chunk) == len(ds) == 300 and chunk.nan_rows == 1 and chunk.data.dtype == torch.float16
    for seed in (11, 12):
        torch.manual_seed(seed)
        theirs = [(i, b) for i, b in enumerate(DataLoader(ds, batch_size=bs, shuffle=True, num_workers=0), 1)]
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        ours = list(chunk.epoch())
        assert torch.equal(state, torch.get_rng_state())
        kept = [(i, b) for i, b in theirs if not torch.isnan(b).any()]
        assert len(theirs) == 5 and len(kept) == 4 and theirs[-1][1].shape[0] == 300 - 4 * bs
        assert [i for i, _ in ours] == [i for i, _ in kept]                 # batch_idx counts the skipped batch too
        assert chunk.last_plan.skipped == [i for i, b in theirs if torch.isnan(b).any()]
        for (_, a), (_, b) in zip(ours, kept):
            assert a.dtype == torch.float32 and U.same_bits(_np(a), b.numpy())
    chunk.check()
    # a dataset object and a device tensor are taken as well
    assert ShuffledChunk(ds, bs, DEV).n_rows == 300 and ShuffledChunk(ds.data.to(DEV), bs).nan_rows == 1


def test_shuffled_chunk_refuses_a_chunk_that_does_not_fit(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (1000, 2000))
    with pytest.raises(ValueError, match=r"takes 4096 bytes and cuda:0 has 1000 bytes free"):
        ShuffledChunk(torch.zeros(4, 8, 64, dtype=torch.float16), 8, DEV)


# ---- no host read per step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sae_type", U.TYPES)
def test_batch_supply_and_trainer_loss_never_wait_for_the_device(chunk_file, sae_type):
    """The loop-side work of an epoch under torch's sync debug mode: a host read anywhere raises.  The outputs are leaf
    tensors in the layout of the type's forward_train (the models' own forwards are not what is under test here)."""
    cfg = U.epoch_config()
    chunk = ShuffledChunk(chunk_file, cfg["batch_size"], DEV)
    warm = torch.zeros(4, U.EPOCH["D"], device=DEV)
    trainer_loss(sae_type, U.fake_outputs(sae_type, warm, cfg["n_bits"])[0], warm, cfg)      # the cached constants exist
    torch.manual_seed(3)
    torch.cuda.synchronize()
    steps = 0
    torch.cuda.set_sync_debug_mode("error")
    try:
        for batch_idx, batch in chunk.epoch():
            outputs, reached, untouched = U.fake_outputs(sae_type, batch, cfg["n_bits"], on_device=True)
            losses = trainer_loss(sae_type, outputs, batch, cfg)
            steps += 1
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert steps == 4 and losses.is_cuda and all(t.grad is not None for t in reached) and all(t.grad is None for t in untouched)


@pytest.mark.parametrize("sae_type", U.TYPES)
def test_trainer_loss_gives_the_gradients_of_the_reference_recipe(sae_type):
    cfg = dict(U.epoch_config(), n_bits=5 if sae_type == "rq_sae" else 4)
    batch = torch.from_numpy(U.S.activations(5, 96, 64)).to(DEV)
    outputs, reached, untouched = U.fake_outputs(sae_type, batch, cfg["n_bits"], seed=2)
    losses = trainer_loss(sae_type, outputs, batch, cfg)
    o64, r64, _ = U.fake_outputs(sae_type, batch.double().cpu(), cfg["n_bits"], seed=2)
    total, levels = U.recipe_loss(sae_type, o64, batch.double().cpu(), cfg)
    total.backward()
    assert np.allclose(_np(losses), [float(v.detach()) for v in levels], rtol=1e-5, atol=0)
    for got, want in zip(reached, r64):
        # element-wise to 1e-5; in the rq_sae chain the fp32 targets carry an absolute error of 2^-24 of their own size per
        # level, and a target is no larger than the level's largest difference plus its reconstruction: normwise 2^-20
        atol = 2.0 ** -20 * float(want.grad.abs().max()) if sae_type == "rq_sae" else 1e-12
        assert torch.allclose(got.grad.double().cpu(), want.grad, rtol=1e-5, atol=atol)
    assert all(t.grad is None for t in untouched)


# ---- the Trainer against the reference's loop --------------------------------------------------------------------------------
def _build(sae_type: str, seed: int):
    from quantizedsae_amd.training.trainer import _build_model          # the reference's constructor calls
    model = _build_model(sae_type, U.epoch_config())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in U.epoch_params(sae_type, seed).items()}, strict=False)
    assert not res.unexpected_keys, res
    model = model.to(DEV)
    if sae_type == "t_sae":
        model.decoder.init_mask(U.T_SPARSITY)
    return model


def _total(sae_type: str, m: dict, n_bits: int) -> float:
    """loss_total of the reference's step from the metrics of a logging step"""
    if sae_type == "q_sae":
        return m["recon_loss_total"] + m["sparsity loss"]
    if sae_type == "rq_sae":
        return sum(m[f"recon_loss_group_{i}"] * 4 ** i for i in range(n_bits)) + m["sparsity loss"]
    return m["loss"]


def _log_keys(sae_type: str, n: int):
    if sae_type == "b_sae":
        return {"loss", "recon_loss", "polarize_loss", "activated_neurons", "mag_MSB", "mag_LSB"}
    if sae_type in ("q_sae", "rq_sae"):
        keys = {f"recon_loss_group_{i}" for i in range(n)} | {f"L0 of latent_group_{i}" for i in range(n)} | {"sparsity loss"}
        return keys | ({"recon_loss_total"} if sae_type == "q_sae" else set())
    return {"loss"}


@pytest.fixture(scope="module")
def epoch_fixture():
    return U.load_epoch_fixture()


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory, epoch_fixture):
    d = tmp_path_factory.mktemp("trainer_dataset")
    for name in (U.CHUNK_NAME, U.CHUNK_NAME_2):
        torch.save(U.epoch_chunk(epoch_fixture[0]["seed"]), d / name)
    return d


@pytest.mark.parametrize("sae_type", U.TYPES)
def test_trainer_reproduces_the_reference_loop(sae_type, epoch_fixture, dataset_dir, tmp_path):
    """train() over two chunk files against the reference's classes in the reference's loop (fp64, CPU): the same batches are
    trained on, every step's loss_total within the recorded bound = max(10 * gap, 1e-5) of the fp64 curve, the loss falls,
    the parameters are bitwise the same before a step as after the previous one (also across the skipped NaN batch), log_fn
    gets the reference's keys, and the checkpoint has the reference's state-dict keys and loads back."""
    meta, z = epoch_fixture
    rec, cfg = meta["types"][sae_type], U.epoch_config()
    model = _build(sae_type, meta["seed"])
    logs = []
    t = Trainer(cfg, sae_type, sae_type == "t_sae", True, model=model, dataset_dir=str(dataset_dir), save_dir=str(tmp_path),
                log_fn=logs.append, log_every=1)
    assert t.chunk_files == [U.CHUNK_NAME, U.CHUNK_NAME_2]
    snaps, step = [], t._step

    def snap():
        return torch.cat([p.detach().reshape(-1).view(torch.int32) for p in model.parameters()]).clone()

    def spying_step(*args):
        before = snap()
        out = step(*args)
        snaps.append((before, snap()))
        return out
    t._step = spying_step
    torch.manual_seed(meta["seed"])
    t.train()
    assert t.trained_batches == rec["batch_idx"] and all(len(e) == 4 and 5 - len(e) == 1 for e in t.trained_batches)
    losses = np.array([_total(sae_type, m, cfg["n_bits"]) for m in logs])
    want = z[f"{sae_type}.loss64"]
    assert losses.shape == want.shape == (8,)
    rel = np.abs(losses - want) / np.abs(want)
    print(f"{sae_type}: loss {losses[0]:.5f} -> {losses[-1]:.5f}  max relative deviation from fp64 {rel.max():.3g} "
          f"(reference fp32 {rec['gap']:.3g}, bound {rec['bound']:.3g})")
    assert rel.max() <= rec["bound"], f"max relative deviation {rel.max():.3g} at step {int(rel.argmax())}"
    assert losses[-1] < losses[0]
    assert all(set(m) == _log_keys(sae_type, cfg["n_bits"]) for m in logs)
    per_epoch = len(rec["batch_idx"][0])
    for k in range(1, len(snaps)):
        if k % per_epoch:                                                # within an epoch, the skipped batch included
            assert torch.equal(snaps[k - 1][1], snaps[k][0]), k
        assert not torch.equal(snaps[k][0], snaps[k][1])                 # and a step moves them
    if sae_type == "b_sae":
        w = model.decoder.weight.detach()
        assert logs[-1]["mag_MSB"] == pytest.approx(w[:, 3::4].abs().mean().item(), rel=1e-5)
        assert logs[-1]["mag_LSB"] == pytest.approx(w[:, 0::4].abs().mean().item(), rel=1e-5)
    saved = torch.load(t.model_path, map_location="cpu", weights_only=True)
    # the reference's keys; its STEWeights also registers the last batch it saw as buffers (a [B, H] tensor and a [B, D] one),
    # which this package's ternary class does not keep and whose loader passes over them: those two, and nothing else, differ
    transient = {"decoder.input_activations", "decoder.output_grad"} if sae_type == "t_sae" else set()
    assert set(meta["state_dict_keys"][sae_type]) - set(saved) == transient and set(saved) <= set(meta["state_dict_keys"][sae_type])
    fresh = _build(sae_type, meta["seed"] + 1)
    fresh.load_state_dict(saved)
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), saved[k]), k


def test_trainer_logs_every_log_every_batches(dataset_dir, epoch_fixture, tmp_path, capsys):
    meta, _ = epoch_fixture
    logs = []
    t = Trainer(U.epoch_config(), "baseline_sae", False, True, model=_build("baseline_sae", meta["seed"]),
                dataset_dir=str(dataset_dir), save_dir=str(tmp_path), log_fn=logs.append, log_every=2)
    torch.manual_seed(meta["seed"])
    t.one_epoch(str(dataset_dir / U.CHUNK_NAME))
    kept = meta["types"]["baseline_sae"]["batch_idx"][0]
    assert t.trained_batches == [kept] and len(logs) == sum(1 for i in kept if i % 2 == 0) and all(set(m) == {"loss"} for m in logs)
    skipped = sorted(set(range(1, 6)) - set(kept))
    assert f"Batch {skipped[0]} contains NaN values before forward pass!" in capsys.readouterr().out
    # without log_fn and with no_log, the reference's print lines carry the metrics
    t.log_fn = None
    torch.manual_seed(meta["seed"])
    t.one_epoch(str(dataset_dir / U.CHUNK_NAME))
    out = capsys.readouterr().out
    assert "Batch 2: Loss=" in out                                        # the reference's no_log line of baseline_sae
    lines = [ln for ln in out.splitlines() if ln.startswith("Batch ")]
    assert [int(ln.split()[1].rstrip(":")) for ln in lines] == sorted(int(ln.split()[1].rstrip(":")) for ln in lines)   # batch order


@pytest.mark.parametrize("sae_type", ["b_sae", "baseline_sae"])
def test_trainer_steps_without_the_dense_latent_follow_the_reference_loop(sae_type, epoch_fixture, dataset_dir, tmp_path):
    """The steps that log nothing -- all of them here, log_every is larger than an epoch -- ask forward_train for no dense
    latent (its first output is None).  Their losses, kept by spying on _step, stay within the fixture's bound of the
    reference's fp64 curve like the logging steps' do."""
    meta, z = epoch_fixture
    rec, cfg = meta["types"][sae_type], U.epoch_config()
    logs, kept = [], []
    t = Trainer(cfg, sae_type, False, True, model=_build(sae_type, meta["seed"]), dataset_dir=str(dataset_dir),
                save_dir=str(tmp_path), log_fn=logs.append, log_every=1000)
    step = t._step

    def spying_step(optimizer, batch, log_step):
        outputs, losses = step(optimizer, batch, log_step)
        assert not log_step and outputs[0] is None
        kept.append((losses.clone(), outputs[2].detach().clone() if sae_type == "b_sae" else None))
        return outputs, losses
    t._step = spying_step
    torch.manual_seed(meta["seed"])
    t.train()
    assert logs == [] and t.trained_batches == rec["batch_idx"]
    totals = np.array([float(l[0]) + (cfg["polarize_lambda"] * float(p) if p is not None else 0.0) for l, p in kept])
    want = z[f"{sae_type}.loss64"]
    rel = np.abs(totals - want) / np.abs(want)
    print(f"{sae_type} without the dense latent: max relative deviation from fp64 {rel.max():.3g} (bound {rec['bound']:.3g})")
    assert totals.shape == want.shape and rel.max() <= rec["bound"]


def test_trainer_loss_refuses_a_reconstruction_that_is_not_contiguous():
    x = torch.zeros(8, 16, device=DEV)
    recon = torch.zeros(16, 8, device=DEV).t().requires_grad_(True)
    with pytest.raises(ValueError, match="not contiguous"):
        trainer_loss("baseline_sae", (None, recon), x, U.epoch_config())
