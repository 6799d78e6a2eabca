"""Parity of the secondary configurations bench.py --full times, at the size it times them (bench.secondary_configs):

  * config 3: TernarySparseAutoencoder(512, 32768) at B = 65536 -- split (default) and fp32 decoders, opt-in emulated encoder;
  * config 4: QuantizedMatryoshkaSAE(512, 32768, n_bits=4) at B = 65536 -- encoder bias -2.5 sigma (candidate sweep + sparse
    walk, forward_submit with two slots), the same model through the dense kernels, and random init (band classification);
  * rq_sae: ResidualQuantizedSAE(512, 32768, n_bits=4, abs_range=1.5) at B = 32768;
  * the 32-bit z offset of the bf16 split decoder (qsae_decode_matryoshka_split) and its two guards;
  * the decoder choice of QuantizedMatryoshkaDecoder.decode_bits: a function of the batch alone, not of history or timing.

At this size the ternary latent is 2^31 floats (row byte offsets pass 2^32 from row 32768 on) and the matryoshka z bits are
256 MiB, flagged rows going to the exact fallback in pieces: states the 4096-row tests never reach.  Whole-batch comparisons
stay on the device, in row chunks; 8 GiB latents are freed once compared (peak below ~32 GiB).  Rows against the CPU oracle
are strided over the whole batch (offset, so not tile-aligned) plus rows B/2 - 1, B/2 and B - 1.
"""
import numpy as np
import pytest
import torch

import oracle
from golden_util import residual_clear_rows, row_rel_err
from quantizedsae_amd import QuantizedMatryoshkaSAE, ResidualQuantizedSAE, TernarySparseAutoencoder, ops
from quantizedsae_amd.sae.quantized_matryoshka import nested_sizes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, H = 512, 32768
B = 65536
B_RQ = 32768
CHUNK = 4096
RECON_TOL = 1e-5   # north_star: within 1e-5 relative on fp32 reconstructions (as test_models_gpu.py)


def host(t):
    return t.detach().cpu().numpy()


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def strided_rows(n, rows, offset):
    sel = set(range(offset, rows, rows // n)) | {rows // 2 - 1, rows // 2, rows - 1}
    return torch.tensor(sorted(sel), device=DEV)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-for-bit equality, compared in row chunks (no full-size temporaries)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return all(torch.equal(a[i:i + CHUNK], b[i:i + CHUNK]) for i in range(0, a.shape[0], CHUNK))


def levels_equal(la, lb) -> bool:
    return len(la) == len(lb) and all(bits_equal(a, b) for a, b in zip(la, lb))


def groups_equal(ga, gb) -> bool:
    return len(ga) == len(gb) and all(float(a) == float(b) for a, b in zip(ga, gb))


def row_rel_err_dev(a: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """golden_util.row_rel_err on the device: per row max |a - ref| / max |ref|, in fp64, chunked."""
    out = []
    for i in range(0, a.shape[0], CHUNK):
        x, r = a[i:i + CHUNK].double(), ref[i:i + CHUNK].double()
        out.append((x - r).abs().amax(1) / r.abs().amax(1).clamp_min(1e-30))
    return torch.cat(out)


def unpack_bits(z: torch.Tensor) -> torch.Tensor:
    """int32-packed z bits [R, words] -> uint8 [R, 32 words] (bit j of word w = unit 32 w + j)."""
    shifts = torch.arange(8, device=z.device, dtype=torch.uint8)
    return ((z.contiguous().view(torch.uint8)[..., None] >> shifts) & 1).reshape(z.shape[0], -1)


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- models, built as bench.secondary_configs builds them (weights from a seeded device generator) -----------------------
def make_ternary(seed):
    g = gen(seed)
    m = TernarySparseAutoencoder(D, H).to(DEV).eval()
    lin = m.encoder.linear
    bound = 1.0 / D ** 0.5                                    # nn.Linear's default init
    with torch.no_grad():
        lin.weight.copy_((torch.rand((H, D), device=DEV, generator=g) * 2 - 1) * bound)
        lin.bias.copy_((torch.rand((H,), device=DEV, generator=g) * 2 - 1) * bound)
        m.decoder.weight.copy_(torch.randn((D, H), device=DEV, generator=g) * 0.5)      # bench: normal_(0, 0.5)
    return m


def make_matryoshka(seed, enc_bias=0.0, hidden=H):
    g = gen(seed)
    m = QuantizedMatryoshkaSAE(D, hidden, top_k=32, abs_range=4, n_bits=4).to(DEV).eval()
    lin = m.encoder.linear
    bound = (6.0 / (D + hidden)) ** 0.5                       # xavier_uniform, gain 1
    with torch.no_grad():
        lin.weight.copy_((torch.rand((hidden, D), device=DEV, generator=g) * 2 - 1) * bound)
        lin.bias.fill_(enc_bias)
        m.decoder.weight.copy_(torch.rand((hidden, D), device=DEV, generator=g) * 2 - 1)         # bench: uniform_(-1, 1)
        m.decoder.weight_mirror.copy_(torch.rand((hidden, D), device=DEV, generator=g) * 2 - 1)
    return m


def sigma_bias(sigmas, hidden):
    """enc_bias_sigmas of synthetic.matryoshka_sae_params: -2.5 sigma at H = 32768 is bench's fill_(-0.44)."""
    return sigmas * float(np.sqrt(D) * np.sqrt(6.0 / (D + hidden)) / np.sqrt(3.0))


def make_residual(seed, stage0_bias=0.0):
    g = gen(seed)
    m = ResidualQuantizedSAE(D, H, top_k=32, abs_range=1.5, n_bits=4).to(DEV).eval()
    with torch.no_grad():
        for i, sae in enumerate(m.saes):
            h = sae.hidden_dim
            bound = (6.0 / (D + h)) ** 0.5                    # xavier_uniform on both sides, as the constructors do
            lin = sae.encoder.linear
            lin.weight.copy_((torch.rand((h, D), device=DEV, generator=g) * 2 - 1) * bound)
            lin.bias.fill_(stage0_bias if i == 0 else 0.0)
            sae.decoder.weight.copy_((torch.rand((h, D), device=DEV, generator=g) * 2 - 1) * bound)
            sae.decoder.weight_mirror.copy_((torch.rand((h, D), device=DEV, generator=g) * 2 - 1) * bound)
    return m


def row_err_vs_fp64(model, z, level_sets, chunk=2048):
    """Per row, the largest over levels of max |level - ref| / max |ref|, for each list of levels in ``level_sets``; ref is
    the matryoshka decode of the whole batch's z bits with fp64 sums on the device (the oracle's pack: scale_j * codes_j)."""
    dec = model.decoder
    codes, scale = oracle.matryoshka_pack(host(dec.weight), host(dec.weight_mirror), dec.n_bits, dec.abs_range)
    wsc = torch.from_numpy(codes).to(DEV, torch.float64) * torch.from_numpy(scale).to(DEV, torch.float64)[:, None]
    ends = np.cumsum(dec.nested_dictionary_size)
    bias = dec.bias.detach().double()
    rows = z.shape[0]
    errs = [torch.zeros(rows, dtype=torch.float64, device=DEV) for _ in level_sets]
    for r in range(0, rows, chunk):
        zf = unpack_bits(z[r:r + chunk]).double()
        ref = bias.expand(zf.shape[0], -1)
        start = 0
        for i, e in enumerate(ends):
            ref = ref + zf[:, start:e] @ wsc[start:e]
            start = e
            for k, lv in enumerate(level_sets):
                err = (lv[i][r:r + chunk].double() - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-30)
                errs[k][r:r + chunk] = torch.maximum(errs[k][r:r + chunk], err)
        del zf, ref
    return errs


def matryoshka_oracle(m, x_rows):
    lin, dec = m.encoder.linear, m.decoder
    return oracle.matryoshka_forward(host(x_rows), host(lin.weight), host(lin.bias), host(dec.weight), host(dec.weight_mirror),
                                     host(dec.bias), n_bits=m.n_bits, abs_range=m.abs_range)


# ---- a. config 3 ------------------------------------------------------------------------------------------------------
def test_ternary_config3_full_batch():
    model = make_ternary(31)
    x = torch.randn((B, D), device=DEV, generator=gen(32))
    assert model.decoder.resolved_precision(B) == "split"
    h, rec = model(x)
    model.decoder.precision = "fp32"
    rec32 = model.decoder(h)
    model.decoder.precision = "auto"

    lin = model.encoder.linear
    sel = strided_rows(64, B, 3)
    want = oracle.ternary_forward(host(x[sel]), host(lin.weight), host(lin.bias), host(model.decoder.weight))
    assert np.array_equal(host(h[sel]).view(np.int32), want["latent"].view(np.int32))
    for r in (rec, rec32):
        errs = row_rel_err(host(r[sel]), want["reconstruction"])
        assert errs.max() <= RECON_TOL, errs.max()
    errs = row_rel_err_dev(rec, rec32)
    assert float(errs.max()) <= RECON_TOL, float(errs.max())
    del rec32

    # row independence across the 2^32-byte line: two halves, and the batch rolled by one row
    half = B // 2
    for lo, hi in ((0, half), (half, B)):
        hh, rh = model(x[lo:hi])
        assert bits_equal(hh, h[lo:hi]) and bits_equal(rh, rec[lo:hi]), (lo, hi)
        del hh, rh
    free()
    hr, rr = model(torch.roll(x, 1, 0))
    assert bits_equal(hr[1:], h[:-1]) and bits_equal(hr[:1], h[-1:])
    assert bits_equal(rr[1:], rec[:-1]) and bits_equal(rr[:1], rec[-1:])
    del hr, rr, rec
    free()

    # opt-in emulated encoder: fp32-accurate against the exact chain, per row (bound of test_emulated_encoder_is_fp32_accurate)
    model.encoder.precision = "emulated"
    he, _ = model(x)
    err = []
    for i in range(0, B, CHUNK):
        a, b_ = he[i:i + CHUNK], h[i:i + CHUNK]
        err.append((a - b_).abs().amax(1).double() / b_.abs().amax(1).double().clamp_min(1e-30))
    e = float(torch.cat(err).max())
    assert e < 4e-6, e
    # ... and against an fp64 contraction on 8 strided rows
    sel8 = strided_rows(8, B, 11)
    xr = host(x[sel8]).astype(np.float64)
    pre = xr @ host(lin.weight).astype(np.float64).T + host(lin.bias).astype(np.float64)
    want64 = np.maximum(pre, 0)
    scale = np.abs(pre).max(axis=1, keepdims=True) + 1e-30
    e_emu = (np.abs(host(he[sel8]) - want64) / scale).max()
    e_f32 = (np.abs(host(h[sel8]) - want64) / scale).max()
    assert e_emu < 4e-6 and e_f32 < 4e-6 and e_emu < 1.5 * e_f32 + 2e-7, (e_emu, e_f32)
    del he, h, x, model
    free()


# ---- b. config 4 at -2.5 sigma ------------------------------------------------------------------------------------------
def test_matryoshka_config4_sparse_full_batch():
    bias = sigma_bias(-2.5, H)
    assert abs(bias + 0.44) < 0.005                          # bench's fill_(-0.44)
    model = make_matryoshka(41, bias)
    x = torch.randn((B, D), device=DEV, generator=gen(42))
    assert model.resolved_bits_path(B) == "prefilter"

    z = model.activation_bits(x, "prefilter")
    assert model.last_flagged_rows < B // 8, model.last_flagged_rows
    assert bits_equal(model.activation_bits(x, "band"), z)
    assert bits_equal(model.activation_bits(x, "dense"), z)

    g, lv = model(x)                                         # default: candidate sweep + sparse walk
    assert model.resolved_bits_path(B) == "prefilter"
    # the dense kernels only: SPARSE_MAX_ACTIVE_FRACTION = 0 keeps the decoder off the sparse walk at this density
    model.bits_path = "dense"
    model.decoder.SPARSE_MAX_ACTIVE_FRACTION = 0.0
    model.decoder.precision = "fp32"                         # the exact-fp32 MFMA chain (qsae_decode_matryoshka)
    g32, lv32 = model(x)
    assert levels_equal(lv, lv32) and groups_equal(g, g32)   # the sparse walk reproduces it bit for bit
    model.decoder.precision = "auto"                         # as bench sets it: the dense split decoder
    gs, lvs = model(x)
    del model.decoder.SPARSE_MAX_ACTIVE_FRACTION
    model.bits_path = "auto"
    assert groups_equal(gs, g32)
    assert not levels_equal(lvs, lv32)                       # (the split decoder did run: another rounding order)
    for i in range(4):
        e = float(row_rel_err_dev(lvs[i], lv32[i]).max())
        assert e <= RECON_TOL, (i, e)
    for k, err in enumerate(row_err_vs_fp64(model, z, [lvs, lv32])):
        assert float(err.max()) <= RECON_TOL, (k, float(err.max()))
    del gs, lvs, lv32

    # latent groups: float32(count_i / B), count_i an independent popcount of level i's bits
    ends = np.cumsum(model.decoder.nested_dictionary_size)
    assert model.decoder.padded_sizes == list(model.decoder.nested_dictionary_size)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    for r in range(0, B, 8192):
        bits = unpack_bits(z[r:r + 8192])
        start = 0
        for i, e in enumerate(ends):
            counts[i] += bits[:, start:e].sum(dtype=torch.int64)
            start = e
        del bits
    for i in range(4):
        assert float(g[i]) == float(np.float32(int(counts[i]) / B)), i

    # 16 strided rows against the oracle: z bits exact, levels at 1e-5
    sel = strided_rows(16, B, 5)
    want = matryoshka_oracle(model, x[sel])
    assert np.array_equal(host(unpack_bits(z[sel]))[:, :H], want["zbits"])
    for i in range(4):
        errs = row_rel_err(host(lv[i][sel]), want["reconstruction_levels"][i])
        assert errs.max() <= RECON_TOL, (i, errs.max())

    # two batches in flight: each result() equals forward() of its batch, bit for bit
    x2 = torch.randn((B, D), device=DEV, generator=gen(43))
    g2, lv2 = model(x2)
    h0 = model.forward_submit(x, slot=0)
    h1 = model.forward_submit(x2, slot=1)
    sg0, sl0 = h0.result()
    sg1, sl1 = h1.result()
    assert levels_equal(sl0, lv) and groups_equal(sg0, g)
    assert levels_equal(sl1, lv2) and groups_equal(sg1, g2)
    del x, x2, z, lv, lv2, sl0, sl1, model
    free()


# ---- c. config 4 at random init -----------------------------------------------------------------------------------------
def test_matryoshka_config4_random_init_full_batch():
    model = make_matryoshka(51, 0.0)
    x = torch.randn((B, D), device=DEV, generator=gen(52))
    assert model.resolved_bits_path(B) == "prefilter"
    g1, l1 = model(x)                                        # overflows the candidate lists: the model leaves the prefilter
    assert model.last_flagged_rows * 2 > B and model.resolved_bits_path(B) == "band"
    g2, l2 = model(x)
    assert model.last_flagged_rows <= B // 50, model.last_flagged_rows
    model.bits_path = "dense"
    g3, l3 = model(x)
    assert levels_equal(l1, l2) and levels_equal(l1, l3)
    assert groups_equal(g1, g2) and groups_equal(g1, g3)
    model.decoder.precision = "fp32"
    g4, l4 = model(x)
    assert groups_equal(g1, g4)
    # half of the units fire: sums of ~24 k cancelling terms, rounded in another order by each kernel.  Against each other the
    # two differ by up to 1.1e-5 of a row's largest output somewhere in the 65536 rows (measured), so that comparison is the
    # max-norm over the level (as test_matryoshka_prefilter_path_matches_dense_path); what bounds the error of either kernel
    # is the fp64 decode of the whole batch below: every row of both within 1e-5 of it
    for i in range(4):
        e = float((l3[i] - l4[i]).abs().max()) / float(l4[i].abs().max())
        assert e < RECON_TOL, (i, e)
    del l2

    z = model.activation_bits(x, "dense")
    assert bits_equal(model.activation_bits(x, "band"), z)
    assert bits_equal(model.activation_bits(x, "prefilter"), z)
    err_split, err_f32 = row_err_vs_fp64(model, z, [l3, l4])
    assert float(err_split.max()) <= RECON_TOL and float(err_f32.max()) <= RECON_TOL, \
        (float(err_split.max()), float(err_f32.max()))
    worst = int(err_split.argmax())
    del l3
    # 16 strided rows and the split decoder's worst row against the CPU oracle
    sel = torch.unique(torch.cat([strided_rows(16, B, 9), torch.tensor([worst], device=DEV)]))
    want = matryoshka_oracle(model, x[sel])
    assert np.array_equal(host(unpack_bits(z[sel]))[:, :H], want["zbits"])
    for lv in (l1, l4):
        for i in range(4):
            errs = row_rel_err(host(lv[i][sel]), want["reconstruction_levels"][i])
            assert errs.max() <= RECON_TOL, (i, errs.max())
    del x, z, l1, l4, model
    free()


# ---- d. rq_sae ----------------------------------------------------------------------------------------------------------
def test_residual_rq_sae_full_batch():
    model = make_residual(61)
    x = torch.randn((B_RQ, D), device=DEV, generator=gen(62))
    assert all(sae.resolved_bits_path(B_RQ) == "prefilter" for sae in model.saes)
    g1, l1 = model(x)                                        # prefilter, overflow -> exact fallback of every stage
    assert all(sae.resolved_bits_path(B_RQ) == "band" for sae in model.saes)
    g2, l2 = model(x)                                        # band classification
    assert levels_equal(l1, l2) and groups_equal(g1, g2)

    # stage by stage as _forward_eager: the band bits equal the exact bits on the stage's own residual
    residual = x
    for i, sae in enumerate(model.saes):
        zb = sae.activation_bits(residual, "band")
        assert bits_equal(zb, sae.activation_bits(residual, "dense")), i
        gi, recs = sae(residual)
        assert bits_equal(recs[-1], l1[i]) and float(gi[-1]) == float(g1[i]), i
        residual = ops.residual_update(residual, recs[-1], 2.0)

    # strided rows against the oracle: near-cutoff audit as in test_residual_sae
    sel = strided_rows(16, B_RQ, 7)
    stages = [dict(enc_w=host(s.encoder.linear.weight), enc_b=host(s.encoder.linear.bias), dec_w=host(s.decoder.weight),
                   dec_wm=host(s.decoder.weight_mirror), dec_bias=host(s.decoder.bias)) for s in model.saes]
    want = oracle.residual_forward(host(x[sel]), stages, abs_range=1.5)
    n_clear = 0
    for i in range(4):
        clear = residual_clear_rows(want["cutoff_distance"], i)
        n_clear += int(clear.sum())
        errs = row_rel_err(host(l1[i][sel]), want["reconstruction_levels"][i])
        if clear.any():
            assert errs[clear].max() < RECON_TOL, (i, errs[clear].max())
        assert errs.max() < 5e-3, i
    assert n_clear >= 4 * len(sel) // 2, n_clear
    del x, residual, l1, l2, model
    free()


# ---- e. the 32-bit z offset of the split decoder --------------------------------------------------------------------------
def test_split_decoder_z_offset_guard():
    from quantizedsae_amd._lib import ERR_UNSUPPORTED, QsaeError
    model = make_matryoshka(71, 0.0)
    dec = model.decoder
    st = dec.packed()
    assert "tq" in st and st["H"] == H
    words, ld = H // 32, 1 << 24
    buf = torch.randint(-(1 << 31), (1 << 31) - 1, (64, ld), dtype=torch.int32, device=DEV, generator=gen(72))   # 4 GiB
    bias = dec.bias.detach()
    z63 = buf[:63, :words]
    assert z63.stride(0) == ld and 63 * ld * 4 < (1 << 32)
    lv_s, c_s = ops.decode_matryoshka_split(z63, H, D, 4, st["tq"], st["s3"], bias, True, st["sizes"])
    lv_f, c_f = ops.decode_matryoshka(z63, H, D, 4, st["codes"], st["scale"], bias, True, st["sizes"])
    assert torch.equal(c_s, c_f)
    for i in range(4):
        e = float(row_rel_err_dev(lv_s[i], lv_f[i]).max())
        assert e <= RECON_TOL, (i, e)
    z64 = buf[:, :words]
    assert 64 * ld * 4 == 1 << 32
    out = None
    with pytest.raises(QsaeError, match="4 GiB") as info:
        out = ops.decode_matryoshka_split(z64, H, D, 4, st["tq"], st["s3"], bias, True, st["sizes"])
    assert info.value.code == ERR_UNSUPPORTED and out is None
    # through the model: the decoder falls back to the exact-fp32 chain
    g, lv = dec.decode_bits(z64)
    dec.precision = "fp32"
    g32, lv32 = dec.decode_bits(z64)
    dec.precision = "auto"
    assert levels_equal(lv, lv32) and groups_equal(g, g32)
    del buf, z63, z64, lv_s, lv_f, lv, lv32, model
    free()


# ---- the decoder choice depends on the batch alone ------------------------------------------------------------------------
def _run_history(model, batches, monkeypatch, stale_events):
    outs = []
    with monkeypatch.context() as mp:
        if stale_events:                                     # a GPU that has not reached any recorded event yet
            mp.setattr(torch.cuda.Event, "query", lambda self: False)
        for xb in batches:
            outs.append(model(xb))
            torch.cuda.synchronize()
    return outs


def test_decoder_choice_does_not_depend_on_timing_or_history(monkeypatch):
    """QuantizedMatryoshkaDecoder.decode_bits picks the sparse walk (bit-identical to the fp32 chain) or the bf16 split
    decoder (another rounding order).  The bits of forward(x) must be those of a fresh model's forward(x), whatever the model
    saw before and however far the GPU got: a dense batch (x_dense = 20 x, about half of the units) then the sparse one
    (x, about 0.6 %) twice."""
    bias = sigma_bias(-2.5, H)
    x = torch.randn((B, D), device=DEV, generator=gen(81))
    x_dense, x_sparse = 20.0 * x, x
    seq = [x_dense, x_sparse, x_sparse]
    fresh_dense = make_matryoshka(82, bias)(x_dense)
    fresh_sparse = make_matryoshka(82, bias)(x_sparse)
    for stale in (False, True):
        outs = _run_history(make_matryoshka(82, bias), seq, monkeypatch, stale)
        for (g, lv), (wg, wl) in zip(outs, [fresh_dense, fresh_sparse, fresh_sparse]):
            assert levels_equal(lv, wl) and groups_equal(g, wg), stale
        del outs
    del fresh_dense, fresh_sparse
    free()

    # the residual SAE: stage 0 at -2.5 sigma crosses the sparse/dense threshold between the two batches, and its
    # reconstruction feeds every later stage's threshold
    bias0 = sigma_bias(-2.5, nested_sizes(H, 4)[0])
    xr = x[:B_RQ]
    seq = [20.0 * xr, xr, xr]
    fresh_dense = make_residual(83, bias0)(seq[0])
    fresh_sparse = make_residual(83, bias0)(xr)
    for stale in (False, True):
        outs = _run_history(make_residual(83, bias0), seq, monkeypatch, stale)
        for (g, lv), (wg, wl) in zip(outs, [fresh_dense, fresh_sparse, fresh_sparse]):
            assert levels_equal(lv, wl) and groups_equal(g, wg), stale
        del outs
    del x, x_dense, xr, seq, fresh_dense, fresh_sparse
    free()
