"""Parity of the path bench.py measures, at the size it measures it: B = 65536 rows, H = 32768, D = 512.

At this batch the prefilter runs with parts = 1 (one list segment per row, 256 activation panels), the
co-resident zero-fill kernel over a 2^31-element dense latent, and the refinement kernel decodes every
row -- none of which the 4096-row tests exercise.  Reference semantics: sae/binary.py:91-103 (BinarySAE.forward),
sae/baseline.py:17-40 (BaselineSparseAutoencoder.forward).

Checks (size-independent properties + oracle rows):
  * default path (prefilter) vs the exact-fp32 fused path: idx, val, reconstruction and the WHOLE dense
    latent bit-identical;
  * (latent != 0).sum() == B * k;
  * 64 strided rows bit-exact against the CPU oracle;
  * one strided dense output (row stride > H) at this size through the C-ABI entry point.
"""
import numpy as np
import pytest
import torch

import oracle
from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, D, H, N_BITS, GAMMA = 65536, 512, 32768, 4, 4.0


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def make_binary(seed, enc_bias_std=0.02, dec_bias_std=0.1):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    model = BinarySAE(D, H, gamma=GAMMA, n_bits=N_BITS).to(DEV).eval()
    bound = (6.0 / (D + H)) ** 0.5
    with torch.no_grad():
        model.encoder[0].weight.copy_((torch.rand((H, D), device=DEV, generator=g) * 2 - 1) * bound)
        model.encoder[0].bias.copy_(torch.randn((H,), device=DEV, generator=g) * enc_bias_std)
        bits = torch.randint(0, 2, (H, D * N_BITS), device=DEV, generator=g, dtype=torch.int8)
        model.decoder.weight.copy_((bits.float() * 2 - 1) * 30.0)
        model.decoder.bias.copy_(torch.randn((D,), device=DEV, generator=g) * dec_bias_std)
    x = torch.randn((B, D), device=DEV, generator=g)
    return model, x


def test_binary_headline_default_path_equals_exact_path_and_oracle():
    model, x = make_binary(11)
    k = model.top_k
    assert k == 65
    assert model.resolved_latent_path(B) == "prefilter"
    latent, recon, pol = model(x)
    idx, val, recon_c = model.forward_compact(x)
    assert bits_equal(recon_c, recon)
    # the dense latent is exactly the scatter of (idx, val): k non-zeros per row, B * k in total
    nnz = int((latent != 0).sum())
    assert nnz == B * k
    assert bool(((latent != 0).sum(1) == k).all())
    assert bits_equal(torch.gather(latent, 1, idx.long()), val)
    # exact-fp32 fused path: every output bit-identical, including the whole 8 GiB latent
    model.latent_path = "fused"
    lat_f, rec_f, _ = model(x)
    idx_f, val_f, _ = model.forward_compact(x)
    assert torch.equal(idx_f, idx) and bits_equal(val_f, val)
    assert bits_equal(rec_f, recon)
    assert bits_equal(lat_f, latent)
    del lat_f, rec_f
    model.latent_path = "auto"
    # 64 strided rows against the CPU oracle (bit-exact)
    sel = torch.arange(0, B, B // 64, device=DEV) + 3
    want = oracle.binary_forward(host(x[sel]), host(model.encoder[0].weight), host(model.encoder[0].bias),
                                 host(model.decoder.weight), host(model.decoder.bias), n_bits=N_BITS, gamma=GAMMA, k=k)
    assert np.array_equal(host(idx[sel]), want["idx"])
    assert np.array_equal(host(val[sel]), want["val"])
    assert np.array_equal(host(recon[sel]), want["reconstruction"])
    assert np.array_equal(host(latent[sel]), want["latent"])
    assert float(pol) == pytest.approx(want["polarize_loss"], rel=1e-5, abs=1e-20)


def test_binary_headline_repeatable_and_separate_decode():
    """Two more batches through the default path: the refinement kernel's fused decode equals the stand-alone
    decode kernel, and a repeated call returns the same bits (no dependence on workspace contents)."""
    model, x = make_binary(12, enc_bias_std=0.0, dec_bias_std=0.0)       # the bench configuration: zero biases
    lat0, rec0, _ = model(x)
    model.fuse_decode = False
    lat1, rec1, _ = model(x)
    assert bits_equal(rec1, rec0) and bits_equal(lat1, lat0)
    del lat1, rec1
    model.fuse_decode = True
    x2 = torch.roll(x, 1, 0)
    lat2, rec2, _ = model(x2)
    assert bits_equal(torch.roll(rec2, -1, 0), rec0)
    assert bits_equal(lat2[1:], lat0[:-1]) and bits_equal(lat2[:1], lat0[-1:])


def test_binary_headline_unpolarised_decoder_fused_equals_separate_and_oracle():
    """Config 2 with decoder logits ~ N(0, 2^2) (not polarised): forward() follows the reference's soft-integer
    arithmetic (sae/binary.py:24-47).  At the benchmarked size the one-call form (refinement kernel decoding from the
    fp32 soft table) equals the separate decode kernel bit for bit, and 64 rows agree with the oracle's soft forward at
    1e-5 (latent bit-exact)."""
    import warnings
    model, x = make_binary(14)
    g = torch.Generator(device=DEV)
    g.manual_seed(15)
    with torch.no_grad():
        model.decoder.weight.copy_(torch.randn(model.decoder.weight.shape, device=DEV, generator=g) * 2.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert model.decoder.resolved_decode_mode() == "soft"
        latent, recon, pol = model(x)
        model.fuse_decode = False
        lat_s, rec_s, _ = model(x)
        model.fuse_decode = True
        assert bits_equal(rec_s, recon) and bits_equal(lat_s, latent)
        del lat_s, rec_s
        idx, val, rec_h = model.forward_submit(x, want_dense=False).result()
        assert bits_equal(rec_h, recon)
    sel = torch.arange(0, B, B // 64, device=DEV) + 7
    want = oracle.binary_forward(host(x[sel]), host(model.encoder[0].weight), host(model.encoder[0].bias),
                                 host(model.decoder.weight), host(model.decoder.bias), n_bits=N_BITS, gamma=GAMMA,
                                 k=model.top_k, soft=True)
    assert np.array_equal(host(latent[sel]), want["latent"])
    np.testing.assert_allclose(host(recon[sel]), want["reconstruction"], rtol=1e-5, atol=1e-5)
    assert float(pol) == pytest.approx(want["polarize_loss"], rel=1e-5, abs=1e-20)


def test_headline_strided_dense_output():
    """qsae_encode_topk_prefilter with a dense output whose row stride exceeds H (dense_ld = H + 64): the padding
    columns are untouched, the H used columns equal the contiguous result."""
    model, x = make_binary(13)
    lin = model.encoder.linear
    pw = model._prefilter_weights()
    k = model.top_k
    idx0, val0, dense0 = ops.encode_topk_prefilter(x, lin.weight.detach(), lin.bias.detach(), pw["Wq"], pw["meta"], k)
    ld = H + 64
    buf = torch.full((B, ld), -7.0, dtype=torch.float32, device=DEV)
    idx1, val1, dense1 = ops.encode_topk_prefilter(x, lin.weight.detach(), lin.bias.detach(), pw["Wq"], pw["meta"], k,
                                                   dense_out=buf)
    assert torch.equal(idx1, idx0) and bits_equal(val1, val0)
    assert dense1.stride(0) == ld
    assert bits_equal(dense1.contiguous(), dense0)
    assert bool((buf[:, H:] == -7.0).all())


def test_baseline_headline_default_path_equals_exact_path_and_oracle():
    g = torch.Generator(device=DEV)
    g.manual_seed(21)
    model = BaselineSparseAutoencoder(D, H).to(DEV).eval()
    with torch.no_grad():
        model.encoder[0].bias.copy_(torch.randn((H,), device=DEV, generator=g) * 0.05)
    x = torch.randn((B, D), device=DEV, generator=g)
    k = model.topk
    assert k == 32
    h, recon = model(x)                                      # auto -> prefilter
    assert int((h != 0).sum()) == B * k
    idx, val, recon_c = model.forward_compact(x)
    assert bits_equal(recon_c, recon)
    assert bits_equal(torch.gather(h, 1, idx.long()), val)
    model.latent_path = "fused"
    h_f, rec_f = model(x)
    assert bits_equal(rec_f, recon) and bits_equal(h_f, h)
    del h_f, rec_f
    model.latent_path = "auto"
    sel = torch.arange(0, B, B // 64, device=DEV) + 5
    want = oracle.baseline_forward(host(x[sel]), host(model.encoder[0].weight), host(model.encoder[0].bias),
                                   host(model.decoder.weight), host(model.decoder.bias), k=k)
    assert np.array_equal(host(h[sel]), want["latent"])
    assert np.array_equal(host(recon[sel]), want["reconstruction"])


def test_four_times_the_benchmarked_batch():
    """B = 262144 rows (a 32 GiB dense latent, 2^33 elements: four times the benchmarked batch; sized for the 288 GB of an
    MI355X): k non-zeros per row, the dense latent is the scatter of the compact outputs, and the two halves of the batch
    computed separately give the same bits (row independence, 64-bit addressing everywhere)."""
    model, _ = make_binary(16)
    big = 4 * B
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    x = torch.randn((big, D), device=DEV, generator=g)
    latent, recon, _ = model(x)
    k = model.top_k
    assert int((latent != 0).sum()) == big * k
    idx, val, recon_c = model.forward_compact(x)
    assert bits_equal(recon_c, recon) and bits_equal(torch.gather(latent, 1, idx.long()), val)
    del latent
    half = big // 2
    i1, v1, r1 = model.forward_compact(x[:half].contiguous())
    i2, v2, r2 = model.forward_compact(x[half:].contiguous())
    assert torch.equal(torch.cat([i1, i2]), idx) and bits_equal(torch.cat([v1, v2]), val) and bits_equal(torch.cat([r1, r2]), recon_c)


def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR` in a fresh process: one JSON line with the headline alone,
    timed over exactly 3 steps; the dumped outputs of the last step equal those of the same model's forward() on the
    same batch in this process (bench.dump_outputs over them, bit for bit), the recon-MSE that of the three batches."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path.insert(0, str(root))
    import bench
    from quantizedsae_amd import sharding
    steps = 3
    cmd = [sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(tmp_path / "bench")]
    # a child of this process (which has initialised the GPU): started, never exec'ed into; the earlier tests' cached
    # blocks are handed back first, the child holds two 8 GiB dense latents
    torch.cuda.empty_cache()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(root))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    doc = json.loads(lines[0])
    assert doc["steps"] == steps and doc["config"]["rows_per_gpu"] == B and doc["higher_is_better"] is True
    assert doc["value"] == pytest.approx(B * steps / (doc["ms_per_step"] * steps * 1e-3), rel=1e-9)
    full_only = {"roofline", "forward_blocking", "sustained", "fp32_only_path", "secondary_configs", "cpu_baseline"}
    assert not full_only & set(doc)
    # the same weights and batches here: torch.Generator(seed 1000), step i takes batch i mod 4 (bench.py)
    model = bench.build_model(torch.device(DEV))
    g = torch.Generator(device=DEV)
    g.manual_seed(1000)
    xs = [torch.randn((B, D), device=DEV, generator=g) for _ in range(4)]
    sq = torch.zeros((), dtype=torch.float64, device=DEV)
    for i in range(steps):
        latent, recon, pol = model(xs[i % 4])
        ops.sq_err_sum(recon, xs[i % 4], sq)
    bench.dump_outputs(tmp_path / "here", latent, recon, pol)
    names = sorted(p.name for p in (tmp_path / "bench").iterdir())
    assert names == ["latent.npy", "polarize_loss.npy", "reconstruction.npy"]
    for name in ("latent", "reconstruction", "polarize_loss"):
        got, want = np.load(tmp_path / "bench" / f"{name}.npy"), np.load(tmp_path / "here" / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == want.shape, name
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), name
    assert doc["recon_mse"] == pytest.approx(sharding.reduce_mse(sq, steps * B * D), rel=1e-9)
