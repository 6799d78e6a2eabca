"""The slab selection without a GPU: the arithmetic of qsaew_slab_plan against its restatement and its stated properties; the
ledger of include/qsae_wide.h -- every function declared there is bound in _lib.WIDE_SIGNATURES with as many arguments as it
declares, exported by the product and the debug library as qsaew_*, and is the host-only plan, a *_bytes sizer or driven
between guards in tests/test_wide_gpu.py; the calls of the C ABI that return before any launch, in the order the header
states; op schemas, fakes and the host-tensor refusal; and the models' path rules: "auto" never resolves to "slabs", and
``_check_limits`` takes a wide model only with it."""
import ctypes as C
import re

import pytest
import torch

import test_wide_gpu as G
import wide_util as U
from quantizedsae_amd import BaselineSparseAutoencoder, BinarySAE, _lib, build, ops, torch_ops
from emu_util import ROOT

HEADER = ROOT / "include" / "qsae_wide.h"


def _plan(H, k, slab):
    starts = (C.c_int * (U.MAX_SLABS + 1))()
    S = _lib.load().qsaew_slab_plan(H, k, slab, starts)
    return S, [starts[s] for s in range(max(S, 0) + 1)]


# ---- the plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,k,slab", [(65540, 65, 32768), (69632, 139, 32768), (131072, 256, 32768), (1 << 20, 256, 32768),
                                       (1 << 20, 1, 32768), (20480, 41, 8192), (20480, 41, 4096), (32768, 65, 8192),
                                       (40960, 32, 32768), (65532, 65, 32768), (8192, 16, 256), (260, 4, 256), (4, 4, 256)])
def test_plan_arithmetic(H, k, slab):
    S, starts = _plan(H, k, slab)
    assert S == -(-H // slab) and 1 <= S <= U.MAX_SLABS and H <= U.MAX_H
    assert starts == U.plan(H, k, slab) == ops.wide_plan(H, k, slab)
    assert starts[0] == 0 and starts[-1] == H and len(starts) == S + 1
    assert all(h % 256 == 0 for h in starts[:-1])                                  # ascending multiples of 256
    widths = [b - a for a, b in zip(starts, starts[1:])]
    assert all(w >= k and w > 0 for w in widths)                                   # every slab is at least k wide
    assert all(w <= slab for w in widths)                                          # ... and fits the kernel the slab width names
    assert max(widths) - min(widths) < 256 * S                                     # balanced: no short tail
    if S > 1:
        assert min(widths) > slab // 2 - 256 * S
    assert _lib.load().qsaew_slab_plan(H, k, slab, None) == S                     # starts may be NULL


def test_plan_refusals_in_the_documented_order():
    lib, err = _lib.load(), _lib.load().qsae_last_error
    plan = lambda H, k, slab: lib.qsaew_slab_plan(H, k, slab, None)                 # noqa: E731
    assert plan((1 << 20) + 4, 300, 100) == _lib.ERR_UNSUPPORTED and b"2^20" in err() and b"qsaew_slab_plan" in err()
    assert plan(1 << 20, 300, 100) == _lib.ERR_UNSUPPORTED and b"256" in err()
    assert plan(65538, 65, 100) == _lib.ERR_UNSUPPORTED and b"multiple of 4" in err()
    assert plan(65540, 65, 100) == _lib.ERR_UNSUPPORTED and b"slab" in err()
    assert plan(65540, 65, 65536) == _lib.ERR_UNSUPPORTED and b"slab" in err()
    assert plan(65540, 65, 1024) == _lib.ERR_UNSUPPORTED and b"32 slabs" in err()    # 65 slabs
    assert plan(300, 200, 256) == _lib.ERR_UNSUPPORTED and b"narrower" in err()      # 256 and a tail of 44
    assert plan(520, 200, 256) == _lib.ERR_UNSUPPORTED and b"narrower" in err()      # 256, 256, 8: a tail below k
    # operands that are not positive are the argument group's
    for bad in ((0, 1, 256), (-4, 1, 256), (1024, 0, 256), (1024, 2048, 256), (1024, 8, 0), (1024, 8, -256)):
        assert plan(*bad) == _lib.ERR_INVALID_ARG and b"qsaew_slab_plan" in err(), bad
    with pytest.raises(ValueError, match="32 slabs"):
        ops.wide_plan(65540, 65, 1024)


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 6 and sorted(declared) == sorted(_lib.WIDE_SIGNATURES)
    assert all(n.startswith("qsaew_") for n in declared)
    others = [t for name, t in vars(_lib).items() if name.endswith("SIGNATURES") and name != "WIDE_SIGNATURES"]
    assert len(others) >= 12
    assert not any(n.startswith("qsaew_") for t in others for n in t)
    for name, n_params in declared.items():
        assert len(_lib.WIDE_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaew_")) == sorted(declared)
    for header in (ROOT / "include").glob("*.h"):
        if header.name != "qsae_wide.h":
            assert "qsaew_" not in header.read_text(), header.name
    sizers = {n for n in declared if n.endswith("_bytes")}
    host_only = {"qsaew_slab_plan"}                          # launches nothing: test_plan_* above
    assert sizers | host_only | set(G.GUARDED) == set(declared)
    assert not (sizers | host_only) & set(G.GUARDED)
    assert "wide.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in HEADER.read_text()
    assert "qsae_wide.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()
    # qsae.h and its functions do not change
    assert {"qsae_encode_topk", "qsae_encode_topk_latent", "qsae_encode_topk_prefilter"} <= set(_lib.SIGNATURES)
    assert _lib.load().qsae_encode_topk_workspace_bytes(2048, 512, 65540, 65) == 0
    assert _lib.load().qsae_encode_topk_workspace_bytes(100, 64, 40960, 32) == 0


# ---- calls that need no device ----------------------------------------------------------------------------------------
def test_calls_that_return_before_any_launch_in_the_documented_order():
    lib = _lib.load()
    fake, odd = C.c_void_p(4096), C.c_void_p(4100)           # non-null addresses that are never looked at
    err = lib.qsae_last_error
    INV, UNS, WSP = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE

    def enc(pref, x=fake, W=fake, Wq=fake, meta=fake, B=8, D=64, H=65540, k=65, slab=32768, idx=fake, val=fake, dense=None,
            ld=65540, ws=fake, ws_bytes=1 << 40):
        if pref:
            flagged = C.c_int(-7)
            rc = lib.qsaew_encode_topk_prefilter(x, W, None, Wq, meta, B, D, H, k, slab, idx, val, dense, ld, ws, ws_bytes, 0,
                                                 C.byref(flagged), None)
            return rc, flagged.value
        return lib.qsaew_encode_topk(x, W, None, B, D, H, k, slab, idx, val, dense, ld, ws, ws_bytes, None), None

    for pref, name in ((False, b"qsaew_encode_topk"), (True, b"qsaew_encode_topk_prefilter")):
        # 1. unsupported shapes, ahead of arguments that are wrong as well (B < 0, null pointers)
        for kw, word in ((dict(H=(1 << 20) + 4), b"2^20"), (dict(k=300), b"256"), (dict(H=65538), b"multiple of 4"),
                         (dict(slab=1000), b"slab"), (dict(slab=65536), b"slab"), (dict(H=65540, slab=1024), b"32 slabs"),
                         (dict(H=520, k=200, slab=256), b"narrower"), (dict(D=62), b"input_dim")):
            assert enc(pref, B=-1, x=None, **kw)[0] == UNS and word in err() and name in err(), kw
        # 2. arguments
        for kw in (dict(B=-1), dict(D=0), dict(H=0), dict(k=0), dict(k=65541), dict(slab=0)):
            assert enc(pref, x=None, **kw)[0] == INV and name in err(), kw
        # 3. the empty batch, ahead of pointers and workspace
        rc, flagged = enc(pref, B=0, x=None, W=None, idx=None, val=None, ws=None, ws_bytes=0)
        assert rc == 0 and flagged in (None, 0)
        # 4. pointers, alignment, the dense latent, the workspace
        for kw in (dict(x=None), dict(W=None), dict(idx=None), dict(val=None), dict(ws=None)):
            assert enc(pref, **kw)[0] == INV and b"null" in err(), kw
        if pref:
            assert enc(pref, Wq=None)[0] == INV and enc(pref, meta=None)[0] == INV
            assert enc(pref, Wq=odd)[0] == INV and b"alignment" in err()
        for kw in (dict(x=odd), dict(W=odd), dict(ws=odd)):
            assert enc(pref, **kw)[0] == INV and b"alignment" in err(), kw
        for kw in (dict(dense=odd), dict(dense=fake, ld=65536), dict(dense=fake, ld=65542)):
            assert enc(pref, **kw)[0] == INV and b"dense" in err(), kw
        sizer = lib.qsaew_encode_topk_prefilter_workspace_bytes if pref else lib.qsaew_encode_topk_workspace_bytes
        need = sizer(8, 64, 65540, 65, 32768)
        assert need > 0 and enc(pref, ws_bytes=need - 1)[0] == WSP and b"workspace" in err()

    # -- qsaew_merge_topk: limits, arguments, the empty batch, pointers
    def merge(pidx=fake, pval=fake, S=2, B=4, k=8, starts=(0, 256, 512), idx=fake, val=fake, dense=None, ld=512):
        arr = (C.c_int * (len(starts)))(*starts) if starts is not None else None
        return lib.qsaew_merge_topk(pidx, pval, S, B, k, arr, idx, val, dense, ld, None)

    assert merge(S=33, starts=None) == UNS and b"qsaew_merge_topk" in err()
    assert merge(B=1 << 30, k=2, pidx=None) == UNS and b"2^31" in err()
    for kw in (dict(S=0), dict(B=-1), dict(k=0), dict(starts=None), dict(starts=(-256, 0, 256)), dict(starts=(0, 256, 260))):
        assert merge(pidx=None, **kw) == INV, kw
    assert merge(B=0, pidx=None, pval=None, idx=None, val=None) == 0
    for kw in (dict(pidx=None), dict(pval=None), dict(idx=None), dict(val=None)):
        assert merge(**kw) == INV and b"null" in err(), kw
    assert merge(val=C.c_void_p(4098)) == INV and b"alignment" in err()
    assert merge(dense=fake, ld=511) == INV and b"dense_ld" in err()


def test_workspace_sizes():
    """the part lists twice, each padded to 256 bytes, plus the largest slab's own need; 0 where the call would refuse"""
    lib = _lib.load()
    B, D, k = 2048, 64, 65
    starts = U.plan(65540, k, 32768)
    part = -(-len(starts[:-1]) * B * k * 4 // 256) * 256
    exact = max(lib.qsae_encode_topk_workspace_bytes(B, D, b - a, k) for a, b in zip(starts, starts[1:]))
    pre = max(lib.qsae_encode_topk_prefilter_workspace_bytes(B, D, b - a, k) or lib.qsae_encode_topk_workspace_bytes(B, D, b - a, k)
              for a, b in zip(starts, starts[1:]))
    assert exact > 0 and pre > 0
    assert lib.qsaew_encode_topk_workspace_bytes(B, D, 65540, k, 32768) == 2 * part + exact
    assert lib.qsaew_encode_topk_prefilter_workspace_bytes(B, D, 65540, k, 32768) == 2 * part + pre
    for bad in ((0, D, 65540, k, 32768), (B, 62, 65540, k, 32768), (B, D, 65538, k, 32768), (B, D, 65540, 257, 32768),
                (B, D, 65540, k, 1024), (B, D, (1 << 20) + 4, k, 32768)):
        assert lib.qsaew_encode_topk_workspace_bytes(*bad) == 0 and lib.qsaew_encode_topk_prefilter_workspace_bytes(*bad) == 0
    assert ops.encode_topk_wide_supported(100, 64, 1 << 20, 256) and not ops.encode_topk_wide_supported(100, 64, 65540, 65, 1024)


# ---- the dispatcher surface ---------------------------------------------------------------------------------------------
def test_ops_have_schemas_fakes_and_refuse_host_tensors():
    for name in ("merge_topk_parts", "encode_topk_wide"):
        assert str(getattr(torch.ops.qsae, name).default._schema).startswith(f"qsae::{name}(")
    assert "Tensor(a3!)? dense" in str(torch.ops.qsae.merge_topk_parts.default._schema)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        B, D, H, k = 96, 64, 65540, 8
        x, W, b = torch.empty(B, D), torch.empty(H, D), torch.empty(H)
        idx, val, dense, words = torch.ops.qsae.encode_topk_wide(x, W, b, k, None, None, True, 32768, 0)
        assert idx.shape == (B, k) and idx.dtype == torch.int32 and val.shape == (B, k) and dense.shape == (B, H)
        assert words.shape == (2,) and words.device.type == "cpu"
        assert torch.ops.qsae.encode_topk_wide(x, W, b, k, None, None, False, 32768, 0)[2].shape == (0, H)
        idx, val = torch.ops.qsae.merge_topk_parts(torch.empty(3, B, k, dtype=torch.int32), torch.empty(3, B, k), [0, 256, 512, 768], None)
        assert idx.shape == (B, k) and idx.dtype == torch.int32 and val.shape == (B, k) and val.dtype == torch.float32
    x, W, b = torch.zeros(4, 64), torch.zeros(1024, 64), torch.zeros(1024)
    for fn in (ops.encode_topk_wide, torch_ops.encode_topk_wide):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, W, b, 8, slab=256)
    for fn in (ops.merge_topk_parts, torch_ops.merge_topk_parts):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(2, 4, 8, dtype=torch.int32), torch.zeros(2, 4, 8), [0, 256, 512])


# ---- the models' path rules ---------------------------------------------------------------------------------------------
def test_auto_never_resolves_to_slabs_and_slabs_is_opt_in():
    for H in (1024, 20480, 40960, 65536, 65540, 131072):
        models = [BinarySAE(64, H, gamma=4.0, n_bits=4)]
        if H <= 65540:
            models.append(BaselineSparseAutoencoder(64, H))
        for m in models:
            for path in ("auto", "fused", "inplace", "prefilter"):
                m.latent_path = path
                assert all(m.resolved_latent_path(rows) != "slabs" for rows in (0, 1, 100, 2047, 2048, 65536)), (H, path)
            m.latent_path = "slabs"
            assert all(m.resolved_latent_path(rows) == "slabs" for rows in (0, 1, 100, 2048, 65536))
            assert m.slab_width == 32768
    with pytest.raises(ValueError, match="slabs"):
        m = BinarySAE(64, 1024, gamma=4.0, n_bits=4)
        m.latent_path = "slab"
        m.resolved_latent_path(8)


def test_check_limits_takes_wide_models_only_with_slabs():
    m = BinarySAE(64, 65540, gamma=4.0, n_bits=4)
    for rows in (0, 100, 2048):
        with pytest.raises(ValueError, match="slabs"):       # today's refusal, which now points at the way out
            m._check_limits(m.resolved_latent_path(rows), rows)
    m.latent_path = "slabs"
    for rows in (0, 100, 2048):
        m._check_limits("slabs", rows)
        assert m._select_path(rows, 256, "t") == "slabs"
    m.slab_width = 1024                                      # 65 slabs
    with pytest.raises(ValueError, match="slab_width = 1024"):
        m._check_limits("slabs", 100)
    with pytest.raises(ValueError, match="slab_width = 1024"):
        m._select_path(100, 16, "t")
    m.slab_width = 32768

    wide = BinarySAE(64, 131072, gamma=4.0, n_bits=4)        # int(131072 * 0.002) = 262
    wide.latent_path = "slabs"
    with pytest.raises(ValueError, match="limit of 256.*lower model.k"):
        wide._check_limits("slabs", 2048)
    wide.k = 0.001
    wide._check_limits("slabs", 2048)
    assert BinarySAE(64, 128499, gamma=4.0, n_bits=4).top_k == 256 and BinarySAE(64, 128500, gamma=4.0, n_bits=4).top_k == 257

    b = BaselineSparseAutoencoder(64, 40960)
    with pytest.raises(ValueError, match="32768"):
        b._check_limits(100)
    b.latent_path = "slabs"
    b._check_limits(100)
    b._check_limits(0)
    b.topk = 257
    with pytest.raises(ValueError, match="slab selection"):
        b._check_limits(100)


def test_forward_submit_is_not_built_for_slabs():
    for m in (BinarySAE(64, 1024, gamma=4.0, n_bits=4), BaselineSparseAutoencoder(64, 1024)):
        m.latent_path = "slabs"
        with pytest.raises(ValueError, match="forward_submit.*not built for latent_path = 'slabs'"):
            m.forward_submit(torch.zeros(4, 64))
