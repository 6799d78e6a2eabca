"""The shape contract of every fast path, stated in plain Python and checked against the library's host predicates on a grid
of shapes: every corner of each region plus one step past it.  A change that widens or narrows a region fails here and
points at the GPU corners to add (tests/test_limits_gpu.py, tests/test_train_gpu.py).

The *_workspace_bytes functions return 0 exactly where their entry point refuses the shape; the entry points are called
with a zero-byte workspace (or null buffers), so none of them gets past its argument checks -- no device is touched."""
import ctypes as C

import pytest

from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, _lib, ops

FAKE = C.c_void_p(1 << 20)          # non-null, 256-byte aligned, never dereferenced: every call below stops at a check


# ---- the regions -----------------------------------------------------------------------------------------------------------
def fused_region(B, D, H, k):
    """qsae_encode_topk's fused form (encode_topk.hip use_fused; the fp16 prefilter, prefilter_topk.hip, takes the same region) and qsae_encode_topk_latent on large batches."""
    return B >= 2048 and 8192 <= H <= 65536 and H % 4 == 0 and 1 <= k <= 256 and D > 0 and D % 4 == 0


def chunked_region(B, D, H, k):
    """qsae_encode_topk's chunked form: qsae_encode_dense + qsae_topk_rows (H <= 32768: the row lives in registers)."""
    return B > 0 and 0 < H <= 32768 and H % 4 == 0 and 1 <= k <= min(256, H) and D > 0 and D % 4 == 0


def encode_topk_region(B, D, H, k):
    return fused_region(B, D, H, k) or chunked_region(B, D, H, k)


def prefilter_region(B, D, H, k):
    """fp16-prefiltered pipeline (prefilter_shape_ok): the fused region, D % 64 == 0 and D <= 2048 (kRefMaxD)."""
    return fused_region(B, D, H, k) and D % 64 == 0 and D <= 2048


def bits_prefilter_region(B, D, H):
    """z-bits candidate sweep: the stationary sweep's D, H % 64 == 0, the resolve kernel's LDS bound
    4 (H / 8 + 10240) <= 160 KiB, i.e. H <= 245760."""
    return B > 0 and D in (128, 256, 512) and H > 0 and H % 64 == 0 and H <= 245760


def bits_band_region(B, D, H):
    return B > 0 and 0 < D <= 2048 and D % 64 == 0 and 0 < H <= (1 << 20) and H % 32 == 0


def train_region(D, k):
    return 0 < D <= 4096 and D % 4 == 0 and 0 <= k <= 256


TOPK_B = (1, 1024, 2047, 2048, 4100)
TOPK_D = (4, 48, 100, 102, 512, 1536, 2048, 2112, 4096)
TOPK_H = (4096, 8188, 8192, 32768, 32772, 32800, 40960, 65536, 65540, 65600)
TOPK_K = (1, 65, 256, 257)
BITS_B = (1, 2100, 8200)
BITS_D = (64, 100, 128, 192, 256, 512, 1024, 2048, 2112)
BITS_H = (64, 96, 32768, 32800, 65600, 131072, 245760, 245824, 1 << 20, (1 << 20) + 32)


def _grid(*axes):
    out = [()]
    for axis in axes:
        out = [t + (v,) for t in out for v in axis]
    return out


def _err(lib):
    return (lib.qsae_last_error() or b"").decode(errors="replace")


# ---- fused / chunked encoder + top-k ---------------------------------------------------------------------------------------
def test_encode_topk_workspace_is_reported_exactly_where_a_form_runs():
    lib = _lib.load()
    wrong = [(B, D, H, k) for B, D, H, k in _grid(TOPK_B, TOPK_D, TOPK_H, TOPK_K)
             if (lib.qsae_encode_topk_workspace_bytes(B, D, H, k) > 0) != encode_topk_region(B, D, H, k)]
    assert not wrong, f"{len(wrong)} shapes disagree, e.g. {wrong[:6]}"
    assert ops.encode_topk_supported(2304, 1024, 65536, 65) and not ops.encode_topk_supported(2047, 1024, 65536, 65)
    assert not ops.encode_topk_supported(2048, 512, 65540, 65) and not ops.encode_topk_supported(100, 512, 40960, 65)


def test_encode_topk_entry_point_agrees_with_its_workspace_function():
    """Where a size is reported the entry point passes every shape check (and stops at the zero-byte workspace); where
    none is, it refuses the shape before it looks at a pointer -- nothing is launched either way."""
    lib = _lib.load()
    for B, D, H, k in _grid(TOPK_B, TOPK_D, TOPK_H, TOPK_K):
        if lib.qsae_encode_topk_workspace_bytes(B, D, H, k) > 0:
            rc = lib.qsae_encode_topk(FAKE, FAKE, None, B, D, H, k, FAKE, FAKE, FAKE, 0, None)
            assert rc == _lib.ERR_WORKSPACE, ((B, D, H, k), rc, _err(lib))
        else:
            rc = lib.qsae_encode_topk(None, None, None, B, D, H, k, None, None, None, 0, None)
            assert rc == _lib.ERR_UNSUPPORTED, ((B, D, H, k), rc, _err(lib))


# ---- fp16 prefilter -------------------------------------------------------------------------------------------------------
def test_prefilter_region_and_entry_point():
    lib = _lib.load()
    for B, D, H, k in _grid(TOPK_B, TOPK_D, TOPK_H, TOPK_K):
        want = prefilter_region(B, D, H, k)
        assert (lib.qsae_encode_topk_prefilter_workspace_bytes(B, D, H, k) > 0) == want, (B, D, H, k)
        assert ops.prefilter_supported(B, D, H, k) == want
        rc = lib.qsae_encode_topk_prefilter(FAKE, FAKE, None, FAKE, FAKE, B, D, H, k, FAKE, FAKE, None, H, FAKE, 0, 0,
                                            None, None)
        assert rc == (_lib.ERR_WORKSPACE if want else _lib.ERR_UNSUPPORTED), ((B, D, H, k), rc, _err(lib))
        if want:      # the prefilter region lies inside the fused one: the models' fallback from it always exists
            assert fused_region(B, D, H, k) and lib.qsae_encode_topk_workspace_bytes(B, D, H, k) > 0


# ---- z bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["prefilter", "band"])
def test_bits_regions_and_entry_points(kind):
    lib = _lib.load()
    region = bits_prefilter_region if kind == "prefilter" else bits_band_region
    sizer = getattr(lib, f"qsae_encode_bits_{kind}_workspace_bytes")
    entry = getattr(lib, f"qsae_encode_bits_{kind}")
    supported = getattr(ops, f"encode_bits_{kind}_supported")
    for B, D, H in _grid(BITS_B, BITS_D, BITS_H):
        want = region(B, D, H)
        assert (sizer(B, D, H) > 0) == want, (B, D, H)
        assert supported(B, D, H) == want
        rc = entry(FAKE, FAKE, None, FAKE, FAKE, B, D, H, FAKE, (H + 31) // 32, FAKE, 0, None, None)
        if want:      # past the shape check: refused for the zero-byte workspace
            assert rc == _lib.ERR_INVALID_ARG and "workspace" in _err(lib), ((B, D, H), rc, _err(lib))
        else:
            assert rc == _lib.ERR_UNSUPPORTED, ((B, D, H), rc, _err(lib))
    assert sizer(0, 512, 32768) == 0


# ---- training backward ----------------------------------------------------------------------------------------------------
def test_train_region_and_entry_points():
    lib = _lib.load()
    for D in (4, 50, 64, 512, 2048, 4096, 4100, 8192):
        for k in (0, 1, 65, 256, 257):
            want = train_region(D, k)
            assert ops.train_supported(D, k) == want, (D, k)
            assert (lib.qsae_train_unit_grad_workspace_bytes(64, k, 1024, D) > 0) == train_region(D, 0), (D, k)
            # shapes are checked before pointers: refused, or stopped at the first null buffer
            rc = lib.qsae_train_row_grad(None, 64, k, None, 1024, D, 0.5, None, None, 0, None, None, None, None)
            assert rc == (_lib.ERR_UNSUPPORTED if not want else (_lib.OK if k == 0 else _lib.ERR_INVALID_ARG)), (D, k, rc)
            rc = lib.qsae_train_unit_grad(None, None, None, None, 64, k, None, None, None, 1024, D, 4, 0.5, None, None, None,
                                          None, None, 0, None)
            assert rc == (_lib.ERR_INVALID_ARG if train_region(D, 0) else _lib.ERR_UNSUPPORTED), (D, k, rc)


# ---- the models refuse on the host -----------------------------------------------------------------------------------------
def test_binary_sae_refuses_shapes_no_path_takes():
    m = BinarySAE(64, 65540, gamma=4.0, n_bits=4)                # k = 131; H past the fused form's 65536
    for rows in (100, 2048, 4100):
        with pytest.raises(ValueError):
            m._check_limits(m.resolved_latent_path(rows), rows)
    m = BinarySAE(64, 40960, gamma=4.0, n_bits=4)                # H between 32768 and 65536
    assert m.resolved_latent_path(100) == "inplace" and m.resolved_latent_path(2048) == "prefilter"
    with pytest.raises(ValueError, match="32768"):
        m._check_limits("inplace", 100)
    m._check_limits(m.resolved_latent_path(2048), 2048)          # the fused / prefilter forms take it
    m = BinarySAE(64, 65536, gamma=4.0, n_bits=4)
    m.k = 257.5 / 65536
    with pytest.raises(ValueError, match="limit of 256"):
        m._check_limits(m.resolved_latent_path(4096), 4096)
    m.k = 256.5 / 65536
    m._check_limits(m.resolved_latent_path(4096), 4096)
    m = BinarySAE(102, 8192, gamma=4.0, n_bits=4)                # input_dim not a multiple of 4
    with pytest.raises(ValueError, match="multiples of 4"):
        m._check_limits(m.resolved_latent_path(4096), 4096)


def test_baseline_refuses_shapes_no_path_takes():
    m = BaselineSparseAutoencoder(64, 40960)
    with pytest.raises(ValueError):
        m._check_limits(100)
    m._check_limits(2048)
    m.latent_path = "inplace"
    with pytest.raises(ValueError):
        m._check_limits(2048)
    m = BaselineSparseAutoencoder(64, 65540)
    with pytest.raises(ValueError):
        m._check_limits(2048)
    BaselineSparseAutoencoder(64, 65536)._check_limits(2048)
    BaselineSparseAutoencoder(64, 32768)._check_limits(0)        # an empty batch is legal everywhere


def test_k_interleaved_encoder_operands_of_4_gib_are_refused_before_any_launch():
    """The K-interleaved loaders address an operand with one 32-bit byte offset per lane and have no form with 64-bit addresses:
    an operand of 4 GiB or more is refused where the offsets would wrap (natural-order operands of that size take the K-tail
    loaders instead: tests/test_limits_gpu.py).  x is 4 GiB + 2 MiB, then W."""
    lib = _lib.load()
    B, D, H = 2 ** 18 + 128, 4096, 8
    assert lib.qsae_encode_dense_kperm(FAKE, FAKE, None, B, D, H, ops.ACT_NONE, FAKE, H, None) == _lib.ERR_UNSUPPORTED
    assert lib.qsae_encode_dense_kperm(FAKE, FAKE, None, H, D, B, ops.ACT_NONE, FAKE, B, None) == _lib.ERR_UNSUPPORTED
    assert b"below 4 GiB" in lib.qsae_last_error()
