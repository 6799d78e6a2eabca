"""The watch kernel on the GPU (csrc/watch.hip, quantizedsae_amd.training.watch): the cases of tests/watch_util.py through
ops.tensor_stats bit for bit against the numpy restatement and count for count against torch.histc on the CPU, the same bits
on a second call and for views off their 16-byte boundary, ModelWatch on a small BinarySAE after one training step's
backward, and the Trainer handing the distributions of the raw gradients to log_fn."""
import numpy as np
import pytest
import torch

import trainer_util as TU
import watch_util as U
from quantizedsae_amd import BinarySAE, synthetic as S
from quantizedsae_amd import torch_ops as ops
from quantizedsae_amd.training import ModelWatch, Trainer, tensor_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """these tests run autograd; a test that ran earlier in the session may have left grad mode off"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def lists():
    return U.case_lists()


@pytest.fixture(scope="module")
def wanted(lists):
    """the restatement of every run, computed once"""
    return {(name, bins): U.restate_block(lists[name], bins) for name, bins in U.RUNS}


def _block(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _off_boundary(x: np.ndarray) -> torch.Tensor:
    """x on the device, starting one element past a 16-byte boundary"""
    flat = torch.empty(x.size + 4, dtype=torch.float32, device=DEV)
    flat[1:1 + x.size] = torch.from_numpy(x)
    out = flat[1:1 + x.size]
    assert x.size == 0 or (out.data_ptr() % 16 == 4 and out.is_contiguous())
    return out


@pytest.mark.parametrize("name,bins", U.RUNS, ids=U.RUN_IDS)
def test_tensor_stats_equals_the_restatement_and_torch_histc(lists, wanted, name, bins):
    tensors = lists[name]
    dev = [torch.from_numpy(x).to(DEV) for x in tensors]
    got = _block(ops.tensor_stats(dev, bins))
    want = wanted[(name, bins)]
    assert got.shape == (len(tensors), U.HEAD + bins)
    for t, x in enumerate(tensors):
        assert np.array_equal(got[t], want[t]), (name, t, x.size, got[t][:8], want[t][:8])
        ref = U.histc_cpu(x, bins)
        counts = U.block_counts(got[t:t + 1])[0]
        assert np.array_equal(counts, ref[0] if ref is not None else np.zeros(bins, np.int64)), (name, t)
    assert np.array_equal(_block(ops.tensor_stats(dev, bins)), got)                 # the same bits on a second call
    if bins == 64 and name in ("small", "chunks"):
        assert np.array_equal(_block(ops.tensor_stats([_off_boundary(x) for x in tensors], bins)), got)   # scalar loads


def test_tensor_stats_takes_any_shape_and_parses_into_fields(lists):
    x = lists["single"][0][:1020].reshape(4, 5, 51)
    s = tensor_stats([torch.from_numpy(x).to(DEV), torch.zeros(0, 3, device=DEV)], bins=16)
    want = U.restate_one(x, 16)
    assert (s[0].lo, s[0].hi, s[0].mean, s[0].n_finite) == (float(want["lo"]), float(want["hi"]), want["mean"], 1020)
    assert s[0].counts.tolist() == want["counts"].tolist() and s[0].std == float(np.sqrt(want["m2"] / 1019))
    assert s[1].n_finite == 0 and not s[1].counts.any()
    assert ops.tensor_stats([], 64).shape == (0, 72)
    assert not ops.tensor_stats([torch.zeros(0, device=DEV)], 64).any()
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.tensor_stats([torch.zeros(4, 4, device=DEV).t()])
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.tensor_stats([torch.zeros(4, device=DEV, dtype=torch.float16)])
    with pytest.raises(ValueError, match="bins"):
        ops.tensor_stats([torch.zeros(4, device=DEV)], 0)


def _same(a, b) -> bool:
    return (a.counts.tolist(), a.lo, a.hi, a.n_finite, a.n_nonfinite, a.n_zero, a.mean) == \
           (b.counts.tolist(), b.lo, b.hi, b.n_finite, b.n_nonfinite, b.n_zero, b.mean) and \
           (a.std == b.std or (np.isnan(a.std) and np.isnan(b.std)))


def test_model_watch_collects_parameters_and_gradients_in_one_call():
    D, H, B, n_bits = 64, 256, 16, 4
    model = BinarySAE(D, H, gamma=4.0, n_bits=n_bits)
    model.k = 4 / H                                            # top-4: at most 64 of the 256 decoder rows get a gradient
    model.load_state_dict({k: torch.from_numpy(v) for k, v in S.binary_sae_params(77, D, H, n_bits, dec_bias_std=0.1).items()})
    model = model.to(DEV)
    x = torch.from_numpy(S.activations(77, B, D)).to(DEV)
    _, recon, _ = model.forward_train(x, dense_latent=False)
    torch.nn.functional.mse_loss(recon, x).backward()
    names = [n for n, _ in model.named_parameters()]
    frozen = names[-1]
    dict(model.named_parameters())[frozen].grad = None
    got = ModelWatch(model, log="all").collect()
    assert set(got) == {"parameters/" + n for n in names} | {"gradients/" + n for n in names if n != frozen}
    tensors = [p.detach() for _, p in model.named_parameters()] + [p.grad for n, p in model.named_parameters() if n != frozen]
    keys = ["parameters/" + n for n in names] + ["gradients/" + n for n in names if n != frozen]
    for key, s in zip(keys, tensor_stats(tensors)):
        assert _same(got[key], s), key
    g = model.decoder.weight.grad
    zeros = int((g == 0).sum())
    assert got["gradients/decoder.weight"].n_zero == zeros and zeros > g.numel() // 2    # mostly exact zeros
    assert got["gradients/decoder.weight"].n_finite == g.numel() and got["gradients/decoder.weight"].n_nonfinite == 0
    assert set(ModelWatch(model, log="parameters").collect()) == {"parameters/" + n for n in names}
    assert set(ModelWatch(model, log="gradients").collect()) == {"gradients/" + n for n in names if n != frozen}
    # a tensor without a finite element has no entry; a tensor that would need a copy is refused by name
    with torch.no_grad():
        model.decoder.bias.fill_(float("nan"))
    assert "parameters/decoder.bias" not in ModelWatch(model, log="parameters").collect()
    w = model.decoder.weight
    w.grad = torch.zeros(w.shape[1], w.shape[0], device=DEV).t()                    # the right shape, not contiguous
    with pytest.raises(ValueError, match="gradients/decoder.weight"):
        ModelWatch(model).collect()


def _two_batch_trainer(tmp_path, sae_type, seed, **kw):
    from test_trainer_gpu import _build
    d = tmp_path / f"data_{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    chunk = torch.from_numpy(S.activations(seed, 128, TU.EPOCH["D"])).to(torch.float16).reshape(2, 64, TU.EPOCH["D"])
    torch.save(chunk, d / TU.CHUNK_NAME)
    logs = []
    t = Trainer(TU.epoch_config(), sae_type, False, True, model=_build(sae_type, seed), dataset_dir=str(d),
                save_dir=str(tmp_path), log_fn=logs.append, **kw)
    return t, logs, str(d / TU.CHUNK_NAME)


def test_trainer_hands_over_the_histograms_of_the_raw_gradients(tmp_path):
    """q_sae: apply_secant_grad rewrites the decoder's gradient after the backward; the watch sees it before"""
    t, logs, chunk = _two_batch_trainer(tmp_path, "q_sae", 4100, watch="all", watch_freq=1, log_every=1000)
    model, raw, changed = t.model, [], []
    secant = model.decoder.apply_secant_grad

    def spying_secant():
        before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        raw.append({n: s for n, s in zip(before, tensor_stats(list(before.values())))})
        secant()
        after = dict(model.named_parameters())
        moved = [n for n, g in before.items() if not torch.equal(g, after[n].grad)]
        changed.append({n: s for n, s in zip(moved, tensor_stats([after[n].grad for n in moved]))})
    model.decoder.apply_secant_grad = spying_secant
    torch.manual_seed(5)
    t.one_epoch(chunk)
    assert t.trained_batches == [[1, 2]] and len(logs) == 2 and len(raw) == 2
    names = [n for n, _ in model.named_parameters()]
    for step, (log, before) in enumerate(zip(logs, raw)):
        assert {k for k in log if k.startswith("parameters/")} == {"parameters/" + n for n in names}
        assert {k for k in log if k.startswith("gradients/")} == {"gradients/" + n for n in before}
        assert set(log) == {k for k in log if k.startswith(("parameters/", "gradients/"))}     # a watch step alone: no metrics
        for n, s in before.items():
            assert _same(log["gradients/" + n], s), (step, n)
        assert changed[step], "apply_secant_grad is expected to change a gradient"
        assert any(not _same(log["gradients/" + n], s) for n, s in changed[step].items())      # not those of the rewritten ones
    # a step that logs and watches hands over one dictionary
    t2, logs2, chunk2 = _two_batch_trainer(tmp_path, "q_sae", 4100, watch="gradients", watch_freq=2, log_every=1)
    torch.manual_seed(5)
    t2.one_epoch(chunk2)
    assert len(logs2) == 2 and not any(k.startswith("gradients/") for k in logs2[0])
    assert "recon_loss_total" in logs2[1] and any(k.startswith("gradients/") for k in logs2[1])
    assert not any(k.startswith("parameters/") for k in logs2[1])


def test_trainer_without_watch_logs_what_it_logged_before(tmp_path, capsys):
    runs = []
    for kw in ({}, {"watch": None}):
        t, logs, chunk = _two_batch_trainer(tmp_path, "b_sae", 4100, log_every=1, **kw)
        torch.manual_seed(5)
        t.one_epoch(chunk)
        runs.append(logs)
    assert runs[0] == runs[1] and len(runs[0]) == 2 and set(runs[0][0]) == {"loss", "recon_loss", "polarize_loss",
                                                                           "activated_neurons", "mag_MSB", "mag_LSB"}
    # under no_log printing: one line per tensor after the step's metric line
    t, _, chunk = _two_batch_trainer(tmp_path, "baseline_sae", 4100, watch="all", watch_freq=2, log_every=1)
    t.log_fn = None
    torch.manual_seed(5)
    t.one_epoch(chunk)
    out = capsys.readouterr().out
    assert "Batch 2: watch" in out and "Batch 1: watch" not in out
    for n, _ in t.model.named_parameters():
        assert f"  parameters/{n}: n=" in out and f"  gradients/{n}: n=" in out
