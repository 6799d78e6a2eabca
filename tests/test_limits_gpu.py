"""GPU corners of the shape regions that tests/test_limits_host.py states: the largest D, the largest H, exactly 64 and
128 refinement slices, flagged-row lists longer than one fallback chunk, rows wider than the stand-alone top-k kernel in
the exact fallback, the z-bits sweeps at their LDS and width limits, and the refusals past each edge.

Reference for a whole batch: ops.encode_dense (the exact fmaf chain, pinned to the oracle by test_kernels_gpu.py) and a
stable descending torch.sort, i.e. the kernels' (value desc, index asc) order; the oracle itself on strided rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, QuantizedMatryoshkaSAE, _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 1024


def host(t):
    return t.detach().cpu().numpy()


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def inputs(seed, B, D, H, bias_std=0.05):
    """x ~ N(0, 1) [B, D], xavier-uniform W [H, D], bias ~ N(0, bias_std) [H], all made on the device."""
    g = gen(seed)
    x = torch.randn((B, D), device=DEV, generator=g)
    bound = (6.0 / (D + H)) ** 0.5
    W = (torch.rand((H, D), device=DEV, generator=g) * 2 - 1) * bound
    b = torch.randn((H,), device=DEV, generator=g) * bias_std
    return x, W, b


def ref_topk(x, W, b, k):
    """(idx int32, val) of the exact latent in (value desc, index asc) order, CHUNK rows at a time."""
    B = x.shape[0]
    idx = torch.empty((B, k), dtype=torch.int32, device=DEV)
    val = torch.empty((B, k), dtype=torch.float32, device=DEV)
    for r0 in range(0, B, CHUNK):
        lat = ops.encode_dense(x[r0:r0 + CHUNK], W, b, ops.ACT_NONE)
        v, i = torch.sort(lat, dim=1, descending=True, stable=True)
        idx[r0:r0 + CHUNK] = i[:, :k].int()
        val[r0:r0 + CHUNK] = v[:, :k]
        del lat, v, i
    return idx, val


def strided(n, B):
    return np.arange(n) * (B // n)


def check_oracle_rows(x, W, b, k, idx, val, n=16):
    """The oracle's encoder + top-k on n strided rows."""
    rows = strided(n, x.shape[0])
    oi, ov = oracle.topk(oracle.encode(host(x[rows]), host(W), host(b)), k)
    assert np.array_equal(host(idx[rows]), oi)
    assert np.array_equal(host(val[rows]).view(np.uint32), ov.view(np.uint32))


def assert_topk(idx, val, want_idx, want_val, nonfinite=()):
    """idx everywhere, val bit for bit on the rows with finite inputs (the rule of test_prefilter_degenerate_rows_fall_back)."""
    assert torch.equal(idx, want_idx), f"{int((idx != want_idx).any(1).sum())} rows differ"
    ok = torch.ones(idx.shape[0], dtype=torch.bool, device=DEV)
    ok[list(nonfinite)] = False
    assert torch.equal(val[ok].view(torch.int32), want_val[ok].view(torch.int32))


def assert_dense(dense, want_idx, want_val, H, nonfinite=()):
    ok = torch.ones(dense.shape[0], dtype=torch.bool, device=DEV)
    ok[list(nonfinite)] = False
    want = ops.densify(want_idx, want_val, H)
    assert torch.equal(dense[ok].view(torch.int32), want[ok].view(torch.int32))


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- debug switches (debug library only; always reset) ---------------------------------------------------------------------
@pytest.fixture()
def fused_path():
    """Route the test's calls to libqsae_hip_debug.so and force the fused / prefilter pipelines (switch 2)."""
    with _lib.use_library("debug") as lib:
        lib.qsae_debug_set_topk_path.argtypes = [C.c_int]
        lib.qsae_debug_set_topk_path(2)
        try:
            yield lib
        finally:
            lib.qsae_debug_set_topk_path(0)


@pytest.fixture()
def sliced_refinement(fused_path):
    """fused_path, with the refinement switch free to set (reset to 1 = where it pays)."""
    lib = fused_path
    lib.qsae_debug_set_refine_sliced.argtypes = [C.c_int]
    try:
        yield lib
    finally:
        lib.qsae_debug_set_refine_sliced(1)


def random_packed(seed, H, D, n_bits):
    """A packed n-bit dictionary [H, row_bytes] of random fields (every bit pattern is a valid two's-complement row)."""
    rb = int(ops.binary_row_bytes(D, n_bits))
    assert rb * 8 == D * n_bits                          # no padding bits at these shapes
    return torch.randint(0, 256, (H, rb), dtype=torch.uint8, device=DEV, generator=gen(seed))


def polarised_binary_sae(D, H, n_bits, k, W, b):
    with torch.device(DEV):
        m = BinarySAE(D, H, gamma=4.0, n_bits=n_bits).eval()
    with torch.no_grad():
        m.encoder.linear.weight.copy_(W)
        m.encoder.linear.bias.copy_(b)
        # logits of exactly +-30 (bits of 0 / 1): polarised, so the model takes the hard packed decode
        m.decoder.weight.bernoulli_(0.5, generator=gen(H + D)).mul_(60.0).sub_(30.0)
        m.decoder.bias.normal_(0.0, 0.1, generator=gen(H + D + 1))
    m.k = (k + 0.5) / H
    assert m.top_k == k and m.decoder.resolved_decode_mode() == "hard"
    return m


def want_binary_recon(m, idx, val):
    dec = m.decoder
    return ops.decode_binary_sparse(idx, val, dec.packed()["packed"], dec.out_features, dec.n_bits, dec.quantization_step,
                                    dec.bias.detach())


# ---- 1. the top-k pipeline at its corners ----------------------------------------------------------------------------------
CORNERS = [
    (2304, 2048, 32768, 65),     # the largest D; 64 slices of 512 units
    (2304, 1024, 65536, 65),     # the largest H; 64 slices of 1024 units
    (2304, 2048, 65536, 65),     # 128 slices: the sliced form must fall back to the one-launch refinement
    (2100, 1536, 40960, 100),    # D above 1024 and not a power of two, H between 32768 and 65536
]


@pytest.mark.parametrize("B,D,H,k", CORNERS, ids=[f"{b}x{d}x{h}-k{k}" for b, d, h, k in CORNERS])
def test_topk_pipeline_corners(sliced_refinement, B, D, H, k):
    lib = sliced_refinement
    x, W, b = inputs(1000 + H + D, B, D, H)
    assert ops.prefilter_supported(B, D, H, k) and ops.encode_topk_supported(B, D, H, k)
    want_idx, want_val = ref_topk(x, W, b, k)
    check_oracle_rows(x, W, b, k, want_idx, want_val)
    Wq, meta = ops.prefilter_pack_w(W, b)
    packed = random_packed(H + 1, H, D, 4)
    table = torch.randn((H, D), device=DEV, generator=gen(H + 2))
    dbias = torch.randn((D,), device=DEV, generator=gen(H + 3)) * 0.1
    want_bin = ops.decode_binary_sparse(want_idx, want_val, packed, D, 4, 0.5, dbias)
    want_tab = ops.decode_table_sparse(want_idx, want_val, table, 0.75, dbias)
    for sliced in (2, 0, 1):                                # forced, never, where it pays
        lib.qsae_debug_set_refine_sliced(sliced)
        info = {}
        idx, val, dense = ops.encode_topk_prefilter(x, W, b, Wq, meta, k, info=info)
        assert_topk(idx, val, want_idx, want_val)
        assert_dense(dense, want_idx, want_val, H)
        assert info["flagged_rows"] < B // 8, info
        idx, val, dense, recon = ops.binary_forward_prefilter(x, W, b, Wq, meta, k, packed, 4, 0.5, dbias)
        assert_topk(idx, val, want_idx, want_val)
        assert_dense(dense, want_idx, want_val, H)
        assert bits_equal(recon, want_bin), sliced
        idx, val, none, recon = ops.table_forward_prefilter(x, W, b, Wq, meta, k, table, 0.75, dbias, want_dense=False)
        assert none is None
        assert_topk(idx, val, want_idx, want_val)
        assert bits_equal(recon, want_tab), sliced
    lib.qsae_debug_set_refine_sliced(1)
    idx, val, dense = ops.encode_topk_latent(x, W, b, k)   # the exact-fp32 fused form
    assert_topk(idx, val, want_idx, want_val)
    assert_dense(dense, want_idx, want_val, H)


MODEL_CORNERS = [(4, 2304, 1024, 65536, 65), (8, 2304, 2048, 32768, 65)]


@pytest.mark.parametrize("n_bits,B,D,H,k", MODEL_CORNERS, ids=[f"n{n}-{b}x{d}x{h}" for n, b, d, h, _ in MODEL_CORNERS])
def test_binary_sae_corners(n_bits, B, D, H, k):
    x, W, b = inputs(2000 + H, B, D, H)
    m = polarised_binary_sae(D, H, n_bits, k, W, b)
    want_idx, want_val = ref_topk(x, W, b, k)
    want_recon = want_binary_recon(m, want_idx, want_val)
    for path in ("auto", "fused"):
        m.latent_path = path
        assert m.resolved_latent_path(B) == ("prefilter" if path == "auto" else "fused")
        latent, recon, _ = m(x)
        assert_dense(latent, want_idx, want_val, H)
        assert bits_equal(recon, want_recon), path
        idx, val, recon_c = m.forward_compact(x)
        assert_topk(idx, val, want_idx, want_val)
        assert bits_equal(recon_c, want_recon), path
    check_oracle_rows(x, W, b, k, want_idx, want_val, n=8)


def test_baseline_corner():
    B, D, H = 2100, 1536, 40960
    with torch.device(DEV):
        m = BaselineSparseAutoencoder(D, H).eval()
    x, W, b = inputs(3000, B, D, H)
    with torch.no_grad():
        m.encoder.linear.weight.copy_(W)
        m.encoder.linear.bias.copy_(b)
    want_idx, want_val = ref_topk(x, W, b, 32)
    want_recon = ops.decode_table_sparse(want_idx, want_val, m.decoder.weight.detach().t().contiguous(), 1.0,
                                         m.decoder.bias.detach())
    h, recon = m(x)
    assert_dense(h, want_idx, want_val, H)
    assert bits_equal(recon, want_recon)
    idx, val, recon_c = m.forward_compact(x)
    assert_topk(idx, val, want_idx, want_val)
    assert bits_equal(recon_c, want_recon)


# ---- 2. flagged rows: several fallback chunks, and rows wider than the stand-alone top-k kernel -----------------------------
@pytest.mark.parametrize("k", [200, 256])
def test_flagged_rows_span_several_fallback_chunks(k):
    """Near the refinement's 256 survivors: at k = 256 every row with a single extra unit inside the margin is flagged, so
    the exact fallback's 1024-row chunks run several times -- with the first 32 rows speculative or not."""
    B, D, H = 4100, 512, 8192
    x, W, b = inputs(4000 + k, B, D, H)
    want_idx, want_val = ref_topk(x, W, b, k)
    Wq, meta = ops.prefilter_pack_w(W, b)
    for spec in (0, 32):
        info = {}
        idx, val, dense = ops.encode_topk_prefilter(x, W, b, Wq, meta, k, info=info, spec_rows=spec)
        print(f"k = {k}, spec_rows = {spec}: {info['flagged_rows']} of {B} rows flagged")
        if k == 256:
            assert info["flagged_rows"] > 1024, info
        assert_topk(idx, val, want_idx, want_val)
        assert_dense(dense, want_idx, want_val, H)
    check_oracle_rows(x, W, b, k, want_idx, want_val, n=8)


def test_flagged_rows_wider_than_the_topk_kernel():
    """H = 65536: the exact fallback ranks rows wider than qsae_topk_rows takes (32768), through the entry points and both
    models -- rows flagged by k = 256 (too many survivors), by a NaN input and by a row whose latents all tie."""
    B, D, H, k = 2304, 512, 65536, 256
    x, W, _ = inputs(5000, B, D, H)
    b = torch.zeros((H,), device=DEV)
    nan_row, flat_row = 100, 1500
    x[nan_row, 5] = float("nan")
    x[flat_row] = 0.0                                      # every latent == bias == 0
    want_idx, want_val = ref_topk(x, W, b, k)
    rows = [nan_row, flat_row]                              # the oracle's own ranking of the two degenerate rows
    oi, ov = oracle.topk(oracle.encode(host(x[rows]), host(W), host(b)), k)
    want_idx[rows] = torch.from_numpy(oi).to(DEV)
    want_val[rows] = torch.from_numpy(ov).to(DEV)
    assert np.array_equal(oi[1], np.arange(k))
    Wq, meta = ops.prefilter_pack_w(W, b)
    for spec in (0, 32):
        info = {}
        idx, val, dense = ops.encode_topk_prefilter(x, W, b, Wq, meta, k, info=info, spec_rows=spec)
        assert info["flagged_rows"] > 2, info
        assert_topk(idx, val, want_idx, want_val, nonfinite=[nan_row])
        assert_dense(dense, want_idx, want_val, H, nonfinite=[nan_row])
    idx, val = ops.encode_topk(x, W, b, k)                 # exact-fp32 fused form, same fallback
    assert_topk(idx, val, want_idx, want_val, nonfinite=[nan_row])
    ok = torch.ones(B, dtype=torch.bool, device=DEV)
    ok[nan_row] = False
    # the models; their second call runs the speculative fallback that the first call's flagged rows switch on
    m = polarised_binary_sae(D, H, 4, k, W, b)
    want_recon = want_binary_recon(m, want_idx, want_val)
    for _ in range(2):
        idx, val, recon = m.forward_compact(x)
        assert m.last_flagged_rows > 2
        assert_topk(idx, val, want_idx, want_val, nonfinite=[nan_row])
        assert bits_equal(recon[ok], want_recon[ok])
    del m
    with torch.device(DEV):
        bl = BaselineSparseAutoencoder(D, H).eval()
    with torch.no_grad():
        bl.encoder.linear.weight.copy_(W)
        bl.encoder.linear.bias.zero_()
    w32_idx, w32_val = want_idx[:, :32].contiguous(), want_val[:, :32].contiguous()
    want_recon = ops.decode_table_sparse(w32_idx, w32_val, bl.decoder.weight.detach().t().contiguous(), 1.0,
                                         bl.decoder.bias.detach())
    for _ in range(2):
        h, recon = bl(x)
        assert bl.last_flagged_rows >= 2
        assert_dense(h, w32_idx, w32_val, H, nonfinite=[nan_row])
        assert bits_equal(recon[ok], want_recon[ok])


@pytest.mark.parametrize("D", [2112, 100])
def test_past_the_prefilter_d_limit_the_model_takes_the_fused_form(D):
    B, H, k = 2048, 8192, 65
    x, W, b = inputs(6000 + D, B, D, H)
    m = polarised_binary_sae(D, H, 4, k, W, b)
    assert not ops.prefilter_supported(B, D, H, k) and m.resolved_latent_path(B) == "fused"
    want_idx, want_val = ref_topk(x, W, b, k)
    latent, recon, _ = m(x)
    assert_dense(latent, want_idx, want_val, H)
    assert bits_equal(recon, want_binary_recon(m, want_idx, want_val))
    idx, val, _ = m.forward_compact(x)
    assert_topk(idx, val, want_idx, want_val)
    check_oracle_rows(x, W, b, k, want_idx, want_val, n=8)


def test_shapes_past_the_edges_are_refused_before_any_launch():
    def x64(B):
        return torch.randn((B, 64), device=DEV)
    with torch.device(DEV):
        wide = BinarySAE(64, 65540, gamma=4.0, n_bits=4).eval()
        mid = BinarySAE(64, 40960, gamma=4.0, n_bits=4).eval()
        big_k = BinarySAE(64, 65536, gamma=4.0, n_bits=4).eval()
        base = BaselineSparseAutoencoder(64, 40960).eval()
    big_k.k = 257.5 / 65536
    for model, B in ((wide, 2048), (mid, 100), (big_k, 4096), (base, 100)):
        with pytest.raises(ValueError):
            model(x64(B))
        with pytest.raises(ValueError):
            model.forward_compact(x64(B))
    with pytest.raises(ValueError):
        ops.encode_topk(x64(2048), torch.zeros((65540, 64), device=DEV), None, 65)
    with pytest.raises(ValueError):
        ops.encode_topk_latent(x64(100), torch.zeros((40960, 64), device=DEV), None, 65)


# ---- 3. z bits --------------------------------------------------------------------------------------------------------------
def _sigma(D, H):
    """Standard deviation of a latent for x ~ N(0, 1) and xavier-uniform W."""
    return float(np.sqrt(D) * np.sqrt(6.0 / (D + H)) / np.sqrt(3.0))


def check_bits_oracle_rows(x, W, b, z, n=8):
    gt, _ = oracle.sigmoid_cutoffs()
    H = W.shape[0]
    rows = strided(n, x.shape[0])
    lat = oracle.encode(host(x[rows]), host(W), host(b), oracle.ACT_NONE)
    bits = np.unpackbits(host(z[rows]).view(np.uint8), axis=1, bitorder="little")[:, :H]
    assert np.array_equal(bits, (lat >= gt).astype(np.uint8))


@pytest.mark.parametrize("D", [128, 512])
def test_bits_prefilter_at_its_widest_and_at_65600(D):
    B, Hmax = 2100, 245760
    lib = _lib.load()
    assert lib.qsae_encode_bits_prefilter_workspace_bytes(B, D, Hmax) > 0           # the LDS bound of the resolve kernel
    assert lib.qsae_encode_bits_prefilter_workspace_bytes(B, D, Hmax + 64) == 0
    for H in (Hmax, 65600):
        x, W, b = inputs(7000 + D + H, B, D, H, bias_std=0.05 * _sigma(D, H))
        b -= 3.0 * _sigma(D, H)                              # ~0.13 % of the units fire
        Wq, meta = ops.prefilter_pack_w(W, b)
        z, flagged = ops.encode_bits_prefilter(x, W, b, Wq, meta)
        print(f"D = {D}, H = {H}: {flagged} of {B} rows flagged")
        assert flagged < B, flagged
        assert bits_equal(z, ops.encode_bits(x, W, b))
        check_bits_oracle_rows(x, W, b, z)


def test_bits_prefilter_dense_rows_flag_in_two_fallback_chunks():
    """Half of the units fire: every row overflows its 4096 list entries, and 8200 flagged rows take the exact kernel in two
    chunks of at most 8192."""
    B, D, H = 8200, 128, 32768
    x, W, b = inputs(7100, B, D, H, bias_std=0.0)
    Wq, meta = ops.prefilter_pack_w(W, b)
    z, flagged = ops.encode_bits_prefilter(x, W, b, Wq, meta)
    assert flagged == B
    assert bits_equal(z, ops.encode_bits(x, W, b))
    check_bits_oracle_rows(x, W, b, z)


@pytest.mark.parametrize("D,H", [(64, 131072), (64, 32800), (2048, 131072), (2048, 32800)])
def test_bits_band_corners(D, H):
    """D at both ends of the band's range, H far above the sweep's 32768 and a multiple of 32 that is not one of 64."""
    B = 2100
    x, W, b = inputs(7200 + D + H, B, D, H, bias_std=0.05 * _sigma(D, H))
    b -= 2.0 * _sigma(D, H)                                  # ~2.3 % of the units fire
    assert ops.encode_bits_band_supported(B, D, H)
    Wq, meta = ops.prefilter_pack_w(W, b)
    z, flagged = ops.encode_bits_band(x, W, b, Wq, meta)
    print(f"D = {D}, H = {H}: {flagged} of {B} rows flagged")
    assert flagged < B, flagged
    assert bits_equal(z, ops.encode_bits(x, W, b))
    check_bits_oracle_rows(x, W, b, z)


def test_encoder_rows_past_4_gib_of_activations():
    """x of 4 GiB + 2 MiB: the smallest operand at which a 32-bit byte offset per lane wraps (the asm-staged loaders address
    that way, so operands of this size must take the 64-bit compiler loads).  A wrapped offset lands inside the same
    allocation, on rows 0..127, whose contents differ from the last 128 rows': the last rows of the big batch must equal
    the same rows encoded on their own, bit for bit, dense and as z bits."""
    B, D, H = 2 ** 18 + 128, 4096, 8
    g = gen(9100)
    x = torch.zeros((B, D), device=DEV)
    x[:128] = torch.randn((128, D), device=DEV, generator=g)
    x[-128:] = torch.randn((128, D), device=DEV, generator=g)
    W = torch.randn((H, D), device=DEV, generator=g) * (1.0 / 64.0)
    try:
        tail = x[-128:].contiguous()
        dense = ops.encode_dense(x, W, None)[-128:]
        bits = ops.encode_bits(x, W, None)[-128:]
        assert bits_equal(dense, ops.encode_dense(tail, W, None))
        assert bits_equal(bits, ops.encode_bits(tail, W, None))
    finally:
        del x
        torch.cuda.empty_cache()


def test_matryoshka_at_h65536_auto_equals_dense_and_fp32():
    B, D, H = 2304, 512, 65536
    with torch.device(DEV):
        m = QuantizedMatryoshkaSAE(D, H, top_k=32, abs_range=4, n_bits=4).eval()
    x, W, _ = inputs(8000, B, D, H)
    with torch.no_grad():
        m.encoder.linear.weight.copy_(W)
        m.encoder.linear.bias.fill_(-3.0 * _sigma(D, H))
    assert m.resolved_bits_path(B) == "prefilter"
    groups, levels = m(x)
    print(f"matryoshka H = {H}: {m.last_flagged_rows} of {B} rows flagged")
    assert m.last_flagged_rows * 2 <= B and m.resolved_bits_path(B) == "prefilter"
    z = m.activation_bits(x, "prefilter")
    assert bits_equal(z, m.activation_bits(x, "dense"))
    m.bits_path = "dense"
    m.decoder.precision = "fp32"
    m.decoder.SPARSE_MAX_ACTIVE_FRACTION = 0.0             # the exact-fp32 MFMA chain, not the sparse walk
    g32, l32 = m(x)
    assert all(bits_equal(a, b_) for a, b_ in zip(levels, l32))
    assert all(float(a) == float(b_) for a, b_ in zip(groups, g32))
