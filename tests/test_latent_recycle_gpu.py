"""Recycled dense latents on the GPU (include/qsae_recycle.h, the pool of ops.py): every output of a loop that takes dropped
latents back equals, bit for bit as int32, what the same model returns with ops.LATENT_RECYCLE = False -- so that a -0.0 or a
value left behind by the buffer's previous batch cannot pass.  Shapes: B = 2048, H = 8192, k = 16, the smallest the prefilter
admits; D = 512 (zeros from the co-resident fill kernel) and D = 256 (zeros from the sweep's own waves), through the product
library; the sliced three-launch refinement through the debug library's switch, as tests/test_kernels_gpu.py forces it."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, K = 2048, 8192, 16
DIMS = (512, 256)
DEV = "cuda:0"


def _ops():
    from quantizedsae_amd import ops
    return ops


def _binary(D, seed=11):
    from quantizedsae_amd import BinarySAE, synthetic as S
    model = BinarySAE(D, H, gamma=4.0, n_bits=4)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in S.binary_sae_params(seed, D, H, 4, dec_bias_std=0.1).items()})
    assert model.top_k == K
    return model.to(DEV).eval()


def _baseline(D, topk=K, seed=12):
    from quantizedsae_amd import BaselineSparseAutoencoder, synthetic as S
    model = BaselineSparseAutoencoder(D, H)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in S.baseline_sae_params(seed, D, H, bias_std=0.05).items()})
    model.topk = topk
    return model.to(DEV).eval()


_MODELS = {}


def model_of(kind, D):
    if (kind, D) not in _MODELS:
        _MODELS[kind, D] = (_binary if kind == "binary" else _baseline)(D)
    return _MODELS[kind, D]


def batches(n, D, rows=B, seed=5):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + D)
    return [torch.randn((rows, D), device=DEV, generator=g) for _ in range(n)]


def bits(*tensors):
    """clones, as int32: what a comparison looks at"""
    return tuple(t.clone().view(torch.int32) for t in tensors)


def same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, want))


@pytest.fixture(autouse=True)
def fresh_pool():
    ops = _ops()
    ops.release_workspaces()
    assert ops.LATENT_RECYCLE is True
    yield
    ops.LATENT_RECYCLE = True
    ops.release_workspaces()


class switched_off:
    """the reference of every comparison: the same model, every latent from torch.empty with all its zeros written"""

    def __enter__(self):
        _ops().LATENT_RECYCLE = False

    def __exit__(self, *exc):
        _ops().LATENT_RECYCLE = True
        assert not _ops()._latent_pool                  # the switch keeps no record either
        return False


def hits():
    return _ops().latent_pool_stats["hits"]


# ---- the two loops ------------------------------------------------------------------------------------------------------
def bench_loop(model, xs):
    """submit i, result i - 1, outputs dropped late (bench.py's loop) -> per step (latent, idx, val, reconstruction) as bits and
    whether the step's submit took a latent from the pool"""
    outs, took = [], []
    pending = None
    for i, x in enumerate(xs):
        h0 = hits()
        h = model.forward_submit(x, slot=i % 2)
        took.append(hits() - h0)
        if pending is not None:
            _lat, rec = pending.result()[:2]
            idx, val = pending._outs[:2]
            outs.append(bits(_lat, idx, val, rec))
        pending = h
    _lat, rec = pending.result()[:2]
    idx, val = pending._outs[:2]
    outs.append(bits(_lat, idx, val, rec))
    return outs, took


def blocking_loop(model, xs, after=None):
    """lat, rec, ... = model(x) per batch; after(i, lat) may do something to the latent before its name is rebound"""
    outs, took = [], []
    for i, x in enumerate(xs):
        h0 = hits()
        lat, rec = model(x)[:2]
        took.append(hits() - h0)
        outs.append(bits(lat, rec))
        if after is not None:
            after(i, lat)
    return outs, took


@pytest.mark.parametrize("D", DIMS)
def test_bench_shaped_loop_equals_the_loop_without_recycling(D):
    model, xs = model_of("binary", D), batches(8, D)
    with switched_off():
        want, took0 = bench_loop(model, xs)
    assert took0 == [0] * 8
    got, took = bench_loop(model, xs)
    assert took == [0, 0, 0] + [1] * 5                  # the latent of step i - 2 is still bound when step i is submitted
    for i in range(8):
        assert same(got[i], want[i]), i
    assert all(int((w[0] != 0).sum()) == B * K for w in want)


@pytest.mark.parametrize("kind", ["binary", "baseline"])
@pytest.mark.parametrize("D", DIMS)
def test_blocking_loop_equals_the_loop_without_recycling(kind, D):
    model, xs = model_of(kind, D), batches(6, D)
    with switched_off():
        want, _ = blocking_loop(model, xs)
    got, took = blocking_loop(model, xs)
    assert took == [0, 0, 1, 1, 1, 1]
    for i in range(6):
        assert same(got[i], want[i]), i


def test_baseline_model_in_the_bench_shaped_loop():
    model, xs = model_of("baseline", 512), batches(6, 512)
    with switched_off():
        want, _ = bench_loop(model, xs)
    got, took = bench_loop(model, xs)
    assert took == [0, 0, 0, 1, 1, 1]
    for i in range(6):
        assert same(got[i], want[i]), i


def test_sliced_refinement_writes_into_a_recycled_latent():
    from quantizedsae_amd import _lib
    model, xs = model_of("binary", 512), batches(5, 512)
    with _lib.use_library("debug") as lib:
        lib.qsae_debug_set_refine_sliced.argtypes = [C.c_int]
        lib.qsae_debug_set_refine_sliced(2)
        try:
            with switched_off():
                want, _ = blocking_loop(model, xs)
            got, took = blocking_loop(model, xs)
        finally:
            lib.qsae_debug_set_refine_sliced(1)
    assert took == [0, 0, 1, 1, 1]
    for i in range(5):
        assert same(got[i], want[i]), i


# ---- what the previous batch may have left ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_a_batch_with_nan_inf_and_tied_rows_before_the_reuse(D):
    model = model_of("binary", D)                       # encoder bias 0: an all-zero row ties every latent at +0
    clean = batches(4, D, seed=21)
    dirty = clean[0].clone()
    dirty[3:40:7] = float("nan")
    dirty[100, 5] = float("nan")
    dirty[200:230:3] = float("inf")
    dirty[300, 0] = float("inf")
    dirty[400:420] = 0.0
    xs = [dirty, clean[1], clean[2], dirty, clean[3], clean[0]]
    flagged = []
    with switched_off():
        want, _ = blocking_loop(model, xs, after=lambda i, lat: flagged.append(int(model.last_flagged_rows)))
    assert flagged[0] >= 20 and flagged[3] >= 20 and flagged[1] < 20          # the tied rows took the exact fallback
    got, took = blocking_loop(model, xs)
    assert took == [0, 0, 1, 1, 1, 1]                   # calls 2 and 5 write into what the dirty batches left
    for i in range(6):
        assert same(got[i], want[i]), i


@pytest.mark.parametrize("how", ["view", "detach"])
def test_a_latent_somebody_holds_is_left_alone(how):
    model, xs = model_of("binary", 512), batches(4, 512)
    lat = model(xs[0])[0]
    holder = lat[:, :7] if how == "view" else lat.detach()
    want, ptr = lat.clone(), lat.data_ptr()
    del lat                                             # from here on `holder` alone keeps it alive
    h0 = hits()
    for i in range(10):
        out = model(xs[1 + i % 3])[0]
        assert out.data_ptr() != ptr
    assert hits() - h0 == 8                             # the loop itself recycled from its third call on
    whole = holder._base if how == "view" else holder
    assert whole.data_ptr() == ptr and torch.equal(whole.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("edit", ["add_", "densify"])
def test_a_latent_edited_in_place_is_not_taken(edit):
    ops = _ops()
    model, xs = model_of("binary", 512), batches(5, 512)
    other = torch.randint(0, H, (B, K), device=DEV, dtype=torch.int32)

    def after(i, lat):
        if i == 0:
            if edit == "add_":
                lat.add_(1)
            else:
                ops.densify(other, torch.ones((B, K), device=DEV), H, out=lat)     # a write torch's version counter cannot see

    with switched_off():
        want, _ = blocking_loop(model, xs)
    got, took = blocking_loop(model, xs, after=after)
    assert took == [0, 0, 0, 1, 1]                      # call 2 would have taken the edited latent of call 0
    for i in range(1, 5):
        assert same(got[i], want[i]), i


def test_shape_changes_and_a_second_model_on_the_stream():
    model, wide = model_of("binary", 512), _baseline(512, topk=32)
    rows = [B, B, B, 2 * B, 2 * B, 2 * B, B, B]
    xs = [batches(1, 512, rows=r, seed=40 + i)[0] for i, r in enumerate(rows)]

    def loop():
        outs, took = [], []
        for x in xs:
            h0 = hits()
            lat, rec = model(x)[:2]
            took.append(hits() - h0)
            assert lat.shape == (x.shape[0], H)
            h0 = hits()
            lat2, rec2 = wide(x)
            took.append(hits() - h0)
            outs.append(bits(lat, rec, lat2, rec2))
        return outs, took

    with switched_off():
        want, _ = loop()
    got, took = loop()
    # per (rows, k): the third call of a key in a row is its first hit; four records per device, so the 4096-row calls push the
    # 2048-row records out and the last two steps start over -- nothing is ever served across keys
    assert took == [0, 0, 0, 0, 1, 1] + [0, 0, 0, 0, 1, 1] + [0, 0, 0, 0]
    for i in range(len(xs)):
        assert same(got[i], want[i]), i


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_c_level_stale_list_with_entries_out_of_range_and_a_padded_latent(D):
    from quantizedsae_amd import _lib
    ops = _ops()
    lib = _lib.load()
    model, x = model_of("binary", D), batches(1, D, seed=60)[0]
    xf, W, b, Wq, meta = model._prefilter_operands(x)
    dec = model.decoder
    packed, step, dbias = dec.packed()["packed"], float(dec.quantization_step), dec.bias.detach()
    with switched_off():
        want = bits(*ops.binary_forward_prefilter(xf, W, b, Wq, meta, K, packed, dec.n_bits, step, dbias))
    need = int(lib.qsae_encode_topk_prefilter_workspace_bytes(B, D, H, K))
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    ld, SK, SENTINEL = H + 64, 8, 12345.0
    g = torch.Generator(device=DEV)
    g.manual_seed(61)
    stale = torch.randint(0, H, (B, SK), device=DEV, dtype=torch.int32, generator=g)
    stale[:, 1], stale[:, 3], stale[:, 5] = -1, H, 2 ** 31 - 1
    stale[7, :] = -1                                    # a row that lists nothing
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(buf, stale_ptr, sk):
        idx = torch.full((B, K), -7, dtype=torch.int32, device=DEV)
        val = torch.full((B, K), -7.0, device=DEV)
        rec = torch.full((B, D), -7.0, device=DEV)
        flagged = C.c_int(-1)
        rc = lib.qsaer_binary_forward_prefilter(xf.data_ptr(), W.data_ptr(), b.data_ptr(), Wq.data_ptr(), meta.data_ptr(), B, D, H,
                                                K, packed.data_ptr(), dec.n_bits, step, dbias.data_ptr(), idx.data_ptr(),
                                                val.data_ptr(), buf.data_ptr(), ld, rec.data_ptr(), ws.data_ptr(), need, 0,
                                                C.byref(flagged), stream, stale_ptr, sk)
        torch.cuda.synchronize()
        return rc, idx, val, rec

    # zeros, the sentinel in the pad columns, and something left behind at every listed position that is inside the row
    buf = torch.zeros((B, ld), device=DEV)
    buf[:, H:] = SENTINEL
    r = torch.arange(B, device=DEV)
    for j, junk in ((0, float("nan")), (2, -0.0), (4, 3.5), (6, float("inf")), (7, 1e-30)):
        ok = stale[:, j] >= 0
        buf[r[ok], stale[ok, j].long()] = junk
    rc, idx, val, rec = call(buf, stale.data_ptr(), SK)
    assert rc == _lib.OK
    assert torch.equal(buf[:, H:], torch.full((B, 64), SENTINEL, device=DEV))          # no pad column touched
    assert same(bits(idx, val, buf[:, :H].contiguous(), rec), want)
    # the promise is taken at its word: an unlisted cell keeps what it held -- the zeros were not written again
    free = want[2][9] == 0
    free[stale[9][(stale[9] >= 0) & (stale[9] < H)].long()] = False
    victim = int(torch.nonzero(free)[0])
    buf[9, victim] = 2.5
    rc, idx, val, rec = call(buf, stale.data_ptr(), SK)
    assert rc == _lib.OK and float(buf[9, victim]) == 2.5
    buf[9, victim] = 0.0
    assert same(bits(idx, val, buf[:, :H].contiguous(), rec), want)
    # without a list the call is its namesake: everything is written
    buf[:, :H] = 7.0
    rc, idx, val, rec = call(buf, None, 0)
    assert rc == _lib.OK and same(bits(idx, val, buf[:, :H].contiguous(), rec), want)
    assert torch.equal(buf[:, H:], torch.full((B, 64), SENTINEL, device=DEV))
    # a list needs a width
    for sk in (0, -1, 1025):
        assert call(buf, stale.data_ptr(), sk)[0] == _lib.ERR_INVALID_ARG
    assert b"stale_k" in lib.qsae_last_error()
