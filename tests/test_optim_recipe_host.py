"""The recipe around the Adam step without a GPU: the ledger of include/qsae_optim.h -- every function declared there is bound
in _lib.OPTIM_SIGNATURES with as many arguments as it declares, exported by the product and the debug library as qsaeo_*, and
is either a *_bytes sizer or driven between guards in tests/test_optim_recipe_gpu.py; the calls of the C ABI that return
before any launch, in the order the header states; workspace sizes; op schemas and fakes; the constructor rejections of
optim.Adam and Trainer; state dicts in both directions with a real CPU step of torch.optim.Adam; and the numpy restatements
of tests/optim_recipe_util.py pinned against torch on the CPU."""
import copy
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import optim_recipe_util as R
import optim_util as U
import test_optim_recipe_gpu as G
from quantizedsae_amd import _lib, build, ops, torch_ops
from quantizedsae_amd.optim import Adam, ClipReport
from quantizedsae_amd.sae import BaselineSparseAutoencoder, BinarySAE
from quantizedsae_amd.training import Trainer
from emu_util import CSRC, ROOT

SC = U.scalars()


# ---- the ledger of the header -----------------------------------------------------------------------------------------
def _declared():
    """name -> number of parameters of every function declared in include/qsae_optim.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "qsae_optim.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_every_declared_function_is_bound_exported_and_guarded():
    declared = _declared()
    assert len(declared) == 5 and sorted(declared) == sorted(_lib.OPTIM_SIGNATURES)
    assert all(n.startswith("qsaeo_") for n in declared)
    others = [t for name, t in vars(_lib).items() if name.endswith("SIGNATURES") and name != "OPTIM_SIGNATURES"]
    assert len(others) >= 11
    assert not any(n.startswith("qsaeo_") for t in others for n in t)
    for name, n_params in declared.items():
        assert len(_lib.OPTIM_SIGNATURES[name][1]) == n_params, name
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert sorted(s for s in build.exported_symbols(path) if s.startswith("qsaeo_")) == sorted(declared)
    # no other header declares the prefix
    for header in (ROOT / "include").glob("*.h"):
        if header.name != "qsae_optim.h":
            assert "qsaeo_" not in header.read_text(), header.name
    sizers = {n for n in declared if n.endswith("_bytes")}
    assert sizers | set(G.GUARDED) == set(declared) and not sizers & set(G.GUARDED)
    assert "optim_recipe.hip" in build.SOURCES and _lib.ABI_VERSION == 4
    assert "join qsae.h" in (ROOT / "include" / "qsae_optim.h").read_text()
    assert "qsae_optim.h" in (ROOT / "quantizedsae_amd" / "build.py").read_text()
    assert ops.GRAD_NORM_HEAD == torch_ops.GRAD_NORM_HEAD == R.HEAD
    # qsae.h's own step keeps its symbols
    assert {"qsae_adam_step", "qsae_adam_step_prefilter", "qsae_normalize_columns_table"} <= set(_lib.SIGNATURES)


def test_the_element_step_has_one_text_in_both_sources():
    """csrc/adam_elem.h repeats AdamScalars, adam_elem and block_max3 of csrc/optim.hip (whose host emulation compiles that
    file alone): token for token"""
    a, b = (CSRC / "optim.hip").read_text(), (CSRC / "adam_elem.h").read_text()
    for start in ("struct AdamScalars {", "__device__ __forceinline__ void adam_elem(", "__device__ __forceinline__ void block_max3("):
        end = "\n};\n" if start.startswith("struct") else "\n}\n"
        assert a[a.index(start):a.index(end, a.index(start))] == b[b.index(start):b.index(end, b.index(start))], start


# ---- calls that need no device ----------------------------------------------------------------------------------------
def test_calls_that_return_before_any_launch_in_the_documented_order():
    lib = _lib.load()
    fake = C.c_void_p(4096)                                    # a non-null, 16-byte aligned address that is never looked at
    err = lib.qsae_last_error

    # -- qsaeo_project_columns: sizes, zero sizes, H % 4, ld, null, alignment, W != G
    proj = lib.qsaeo_project_columns
    assert proj(None, None, -1, 8, 8, None) == _lib.ERR_INVALID_ARG and b"qsaeo_project_columns" in err()
    assert proj(None, None, 4, -4, 8, None) == _lib.ERR_INVALID_ARG
    assert proj(None, None, 0, 6, 2, None) == _lib.OK and proj(None, None, 5, 0, 0, None) == _lib.OK       # nothing launched
    assert proj(None, None, 5, 6, 2, None) == _lib.ERR_UNSUPPORTED and b"multiple of 4" in err()          # H before ld
    assert proj(None, None, 5, 8, 4, None) == _lib.ERR_INVALID_ARG and b"ld" in err()                     # ld before null
    assert proj(None, None, 5, 8, 10, None) == _lib.ERR_INVALID_ARG and b"ld" in err()
    assert proj(None, fake, 5, 8, 8, None) == _lib.ERR_INVALID_ARG and b"non-null" in err()
    assert proj(C.c_void_p(4100), fake, 5, 8, 8, None) == _lib.ERR_INVALID_ARG and b"aligned" in err()
    assert proj(fake, fake, 5, 8, 8, None) == _lib.ERR_INVALID_ARG and b"different" in err()

    # -- qsaeo_grad_norm: T, limit, T == 0, null lists, per tensor, limits, max_norm, coef / report, workspace
    norm = lib.qsaeo_grad_norm
    one = (C.c_int64 * 1)(5)
    ptr = (C.c_void_p * 1)(4096)
    assert norm(None, None, -1, 1.0, None, None, None, 0, None) == _lib.ERR_INVALID_ARG and b"qsaeo_grad_norm" in err()
    assert norm(None, None, 65537, 1.0, None, None, None, 0, None) == _lib.ERR_UNSUPPORTED and b"65536" in err()
    assert norm(None, None, 0, -1.0, None, None, None, 0, None) == _lib.OK                               # T == 0 first
    assert norm(None, None, 1, 1.0, None, None, None, 0, None) == _lib.ERR_INVALID_ARG and b"null pointer" in err()
    assert norm(ptr, (C.c_int64 * 1)(-1), 1, -1.0, None, None, None, 0, None) == _lib.ERR_INVALID_ARG and b"negative" in err()
    assert norm((C.c_void_p * 1)(0), one, 1, -1.0, None, None, None, 0, None) == _lib.ERR_INVALID_ARG and b"null tensor" in err()
    assert norm((C.c_void_p * 1)(4098), one, 1, -1.0, None, None, None, 0, None) == _lib.ERR_INVALID_ARG and b"4-byte" in err()
    assert norm(ptr, (C.c_int64 * 1)((1 << 40) + 1), 1, -1.0, None, None, None, 0, None) == _lib.ERR_UNSUPPORTED   # before max_norm
    for bad in (-1.0, float("nan")):
        assert norm(ptr, one, 1, bad, None, None, None, 0, None) == _lib.ERR_INVALID_ARG and b"max_norm" in err()
    assert norm(ptr, one, 1, 1.0, None, fake, None, 0, None) == _lib.ERR_INVALID_ARG and b"coef" in err()
    assert norm(ptr, one, 1, 1.0, fake, C.c_void_p(4100), None, 0, None) == _lib.ERR_INVALID_ARG and b"report" in err()
    assert norm(ptr, one, 1, 1.0, fake, fake, None, 0, None) == _lib.ERR_WORKSPACE
    assert norm(ptr, one, 1, 1.0, fake, fake, fake, 8, None) == _lib.ERR_WORKSPACE and b"workspace" in err()

    # -- qsaeo_adam_step: n, n == 0, null, coef alignment
    step = lib.qsaeo_adam_step
    assert step(None, None, None, None, -1, *SC, None, None, 0.0, None) == _lib.ERR_INVALID_ARG and b"qsaeo_adam_step" in err()
    assert step(None, None, None, None, 0, *SC, C.c_void_p(2), None, 0.0, None) == _lib.OK                  # nothing launched
    assert step(fake, None, fake, fake, 8, *SC, C.c_void_p(2), None, 0.0, None) == _lib.ERR_INVALID_ARG and b"non-null" in err()
    assert step(fake, fake, fake, fake, 8, *SC, C.c_void_p(2), None, 0.0, None) == _lib.ERR_INVALID_ARG and b"coef" in err()

    # -- qsaeo_adam_step_prefilter: the namesake's checks first, then coef, then the averages
    pref = lib.qsaeo_adam_step_prefilter

    def call(W=fake, bias=fake, gb=fake, H=4, D=4, coef=None, emaW=None, emab=None, Wq=fake):
        return pref(W, fake, fake, fake, bias, gb, fake if bias else None, fake if bias else None, H, D, *SC, coef, emaW, emab,
                    0.0, Wq, fake, None)
    assert call(H=0, coef=C.c_void_p(2)) == _lib.ERR_INVALID_ARG and b"H > 0" in err()
    assert call(gb=None, coef=C.c_void_p(2)) == _lib.ERR_INVALID_ARG and b"bias" in err()
    assert call(W=C.c_void_p(4100), coef=C.c_void_p(2)) == _lib.ERR_INVALID_ARG and b"16-byte" in err()
    assert call(coef=C.c_void_p(2), emab=fake) == _lib.ERR_INVALID_ARG and b"coef" in err()               # coef before emab
    assert call(emab=fake) == _lib.ERR_INVALID_ARG and b"emab" in err()                                    # emab without emaW
    assert call(emaW=fake) == _lib.ERR_INVALID_ARG and b"emab" in err()                                    # emaW, bias, no emab
    assert call(bias=None, gb=None, emaW=fake, emab=fake) == _lib.ERR_INVALID_ARG and b"emab" in err()     # emab without bias


def test_workspace_sizes():
    size = _lib.load().qsaeo_grad_norm_workspace_bytes

    def of(*counts):
        return size((C.c_int64 * len(counts))(*counts), len(counts))
    assert of(0) == 256 and of(1) == 256 and of(8192 * 32) == 256 and of(8192 * 32 + 1) == 512          # 8 bytes per chunk
    assert of(*R.NORM_COUNTS) == 256 and of(0, 0, 0) == 256
    assert of(8192 * 33, 1, 8193) == 512                                                                 # 33 + 1 + 2 chunks
    assert of(-1) == 0 and of((1 << 40) + 1) == 0 and of(1 << 40) == 8 << 27
    assert size(None, 1) == 0 and size((C.c_int64 * 1)(1), 0) == 0 and size((C.c_int64 * 1)(1), 65537) == 0
    assert size((C.c_int64 * 9000)(*([1 << 40] * 9000)), 9000) == 0                                      # more than 2^30 chunks


# ---- ops ----------------------------------------------------------------------------------------------------------------
def test_op_schemas_fakes_and_cpu_refusals():
    def written(op):
        return [a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    assert written(torch.ops.qsae.project_columns) == ["G"]
    assert written(torch.ops.qsae.grad_norm) == ["coef", "report"]
    assert written(torch.ops.qsae.adam_step_clipped) == ["p", "m", "v", "ema"]
    assert written(torch.ops.qsae.adam_step_prefilter_clipped) == ["W", "mW", "vW", "bias", "mb", "vb", "emaW", "emab", "Wq", "meta"]
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        t, c = torch.empty(8, 64), torch.empty(1)
        assert torch.ops.qsae.project_columns(t, torch.empty(8, 64)) is None
        assert torch.ops.qsae.grad_norm([t, t], 1.0, c, torch.empty(6, dtype=torch.int64)) is None
        assert torch.ops.qsae.adam_step_clipped(t, t, t, t, 0.1, 0.999, 0.001, 0.05, 1e-8, 1e-3, c, None, 0.0) is None
        assert torch.ops.qsae.adam_step_prefilter_clipped(t, t, t, t, None, None, None, None, 0.1, 0.999, 0.001, 0.05, 1e-8, 1e-3,
                                                          None, t, None, 0.001, torch.empty(8, 64, dtype=torch.float16),
                                                          torch.empty(4)) is None
    z = torch.zeros(8, 8)
    for mod in (ops, torch_ops):
        for call in (lambda: mod.project_columns(z, torch.zeros(8, 8)), lambda: mod.grad_norm([z], 1.0),
                     lambda: mod.adam_step_clipped(z, z, z, z, *SC, coef=torch.ones(1)),
                     lambda: mod.adam_step_prefilter_clipped(z, z, z, z, None, None, None, None, *SC, emaW=z)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    with pytest.raises(ValueError, match="at least one|1 to"):
        ops.grad_norm([], 1.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            ops.grad_norm([z], bad)
    assert ops.project_columns_supported(8) and not ops.project_columns_supported(6) and not ops.project_columns_supported(0)


# ---- constructors -------------------------------------------------------------------------------------------------------
def test_adam_constructor_rejections_and_group_keys():
    w = torch.nn.Parameter(torch.zeros(4, 4))
    for bad in (0.0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Adam([w], max_grad_norm=bad)
    for bad in (1.0, -0.1, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="ema_decay"):
            Adam([w], ema_decay=bad)
    with pytest.raises(ValueError, match="ema_state"):
        Adam([w], ema_decay=0.9, ema_state=[])
    with pytest.raises(ValueError, match="ema_state needs ema_decay"):
        Adam([w], ema_state={})
    opt = Adam([w], max_grad_norm=2.0, ema_decay=0.0)
    g = opt.param_groups[0]
    assert g["max_grad_norm"] == 2.0 and g["ema_decay"] == 0.0 and opt.last_clip is None and opt.clip_report() is None
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
    assert opt.param_groups[1]["max_grad_norm"] == 2.0 and opt.param_groups[1]["ema_decay"] == 0.0
    # the defaults leave torch's keys alone
    plain = Adam([w])
    assert "max_grad_norm" not in plain.param_groups[0] and "ema_decay" not in plain.param_groups[0]
    assert set(plain.state_dict()["param_groups"][0]) == set(torch.optim.Adam([w]).state_dict()["param_groups"][0])
    # one clip value for the whole optimizer: a differing group is refused at the step, before anything runs
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "max_grad_norm": 3.0})
    with pytest.raises(ValueError, match="one number for the whole optimizer"):
        opt.step()
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "max_grad_norm": -3.0})
    assert ClipReport._fields == ("norm", "coef", "clipped", "per_tensor")


def test_trainer_constructor_rejections(tmp_path):
    config = {"input_dim": 4, "n_bits": 4, "hidden_dim": 32, "gamma": 4.0, "epochs": 1, "lr": 1e-3, "top_k": 2,
              "sparsity_lambda": 1e-4, "polarize_lambda": 1e-3, "batch_size": 8}

    def trainer(sae_type="baseline_sae", **kw):
        return Trainer(config, sae_type, sae_type == "t_sae", True, dataset_dir=str(tmp_path), save_dir=str(tmp_path), **kw)
    for bad in (0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="grad_clip"):
            trainer(grad_clip=bad)
    for bad in (1.0, -0.5, float("nan"), "x", True):
        with pytest.raises(ValueError, match="ema_decay"):
            trainer(ema_decay=bad)
    for st in ("b_sae", "q_sae", "rq_sae", "t_sae", "bl_sae"):
        with pytest.raises(ValueError, match=f"decoder_grad_projection.*{st}"):
            trainer(st, decoder_grad_projection=True)
        t = trainer(st, grad_clip=1.5, ema_decay=0.99)                     # the clip and the average work for every type
        assert t.grad_clip == 1.5 and t.ema_decay == 0.99 and t.ema_state == {}
    t = trainer(grad_clip=2, decoder_grad_projection=True)
    assert t.decoder_grad_projection is True and t.ema_state is None and t.ema_path.endswith("baseline_sae_32_ema.pth")
    d = trainer()
    assert d.grad_clip is None and d.decoder_grad_projection is False and d.ema_decay is None and d.ema_state is None
    with pytest.raises(ValueError, match="ema_decay"):
        d.ema_state_dict()
    # without a gradient the projection does nothing, on any device
    m = BaselineSparseAutoencoder(4, 32)
    m.project_decoder_grad()
    assert m.decoder.weight.grad is None
    assert not hasattr(BinarySAE(4, 32), "project_decoder_grad")


def test_project_decoder_grad_torch_composition_on_the_cpu():
    """Shapes the kernel refuses (here: a CPU model) go through the torch composition"""
    m = BaselineSparseAutoencoder(6, 12)
    m.normalize_decoder_weights()
    g = torch.randn(6, 12)
    m.decoder.weight.grad = g.clone()
    m.project_decoder_grad()
    w = m.decoder.weight.detach()
    want = g - (g * w).sum(0, keepdim=True) * w
    assert torch.allclose(m.decoder.weight.grad, want, atol=1e-6)
    assert float((m.decoder.weight.grad * w).sum(0).abs().max()) < 1e-6


# ---- state dicts ----------------------------------------------------------------------------------------------------------
def test_state_dicts_go_both_ways_with_a_real_cpu_step():
    params = [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]
    ours = Adam(params, lr=1e-2, max_grad_norm=1.0, ema_decay=0.99)
    # ours -> torch: the extra group keys and the extra per-parameter "ema" load, and torch's Adam steps
    for p in params:
        st = ours._state_of(p)
        st["step"] += 1
        st["exp_avg"].fill_(0.25)
        st["exp_avg_sq"].fill_(0.5)
        ours._ema_of(p, st)
    sd = copy.deepcopy(ours.state_dict())
    assert sd["param_groups"][0]["max_grad_norm"] == 1.0 and sd["param_groups"][0]["ema_decay"] == 0.99
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
    theirs = torch.optim.Adam(params, lr=7.0)
    theirs.load_state_dict(sd)
    before = [p.detach().clone() for p in params]
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, 0.5 + i)
    theirs.step()
    assert float(theirs.state[params[0]]["step"]) == 2.0 and not torch.equal(before[0], params[0])
    assert theirs.param_groups[0]["lr"] == 1e-2
    assert torch.equal(theirs.state[params[0]]["ema"], before[0])                 # carried along, not touched
    # torch -> ours: a dict without the keys loads, and this optimizer keeps its own options
    plain = torch.optim.Adam(params, lr=3e-3)
    plain.step()
    back = Adam(params, lr=5.0, max_grad_norm=2.0, ema_decay=0.5)
    back.load_state_dict(copy.deepcopy(plain.state_dict()))
    g = back.param_groups[0]
    assert g["lr"] == 3e-3 and g["max_grad_norm"] == 2.0 and g["ema_decay"] == 0.5
    assert set(back.state[params[0]]) == {"step", "exp_avg", "exp_avg_sq"} and float(back.state[params[0]]["step"]) == 1.0
    # ours -> ours keeps the averages and the keys
    again = Adam(params, lr=5.0)
    again.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert again.param_groups[0]["max_grad_norm"] == 1.0 and torch.equal(again.state[params[0]]["ema"], before[0])
    # ema_state: the dict owns the tensors across optimizers
    shared = {}
    first = Adam(params, ema_decay=0.9, ema_state=shared)
    e = first._ema_of(params[0], first._state_of(params[0]))
    second = Adam(params, ema_decay=0.9, ema_state=shared)
    assert second._ema_of(params[0], second._state_of(params[0])) is e and shared[params[0]] is e


# ---- the restatements against torch on the CPU -------------------------------------------------------------------------------
def test_the_norm_restatement_is_as_close_to_the_exact_norm_as_clip_grad_norm():
    ts = R.norm_case("bulk")
    exact = R.exact_norm(ts)
    for max_norm in (0.5 * exact, 2.0 * exact):
        coef, words = R.grad_norm(ts, max_norm)
        ours = float(np.float32(words.view(np.float64)[1]))
        params = [torch.nn.Parameter(torch.zeros(t.size)) for t in ts]
        for p, t in zip(params, ts):
            p.grad = torch.from_numpy(t.copy())
        theirs = float(torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False))
        print(f"exact {exact!r}: |restatement - exact| = {abs(ours - exact):.3e}, |torch - exact| = {abs(theirs - exact):.3e}")
        assert abs(ours - exact) <= abs(theirs - exact)
        # the coefficient: torch's formula on torch's own norm gives the clamp of max_norm / (norm + 1e-6)
        want = min(max_norm / (exact + 1e-6), 1.0)
        assert abs(float(coef) - want) <= 2.0 ** -23 * want
        scaled = params[5].grad.numpy()
        mine = R.clip_grad(ts[5], coef)
        # torch scaled its gradients by its own fp32 norm: apart by that norm's relative error and a rounding or two
        apart = abs(theirs - exact) / exact + 2.0 ** -22
        assert np.abs(scaled.astype(np.float64) - mine.astype(np.float64)).max() <= apart * np.abs(mine).max()
    # the corners go where clip_grad_norm_ takes them
    for kind, check in (("zeros", lambda c: c == 1.0), ("inf", lambda c: c == 0.0), ("nan", math.isnan)):
        ts = R.norm_case(kind)
        coef, _ = R.grad_norm(ts, 1.0)
        p = torch.nn.Parameter(torch.zeros(ts[5].size + ts[4].size))
        p.grad = torch.from_numpy(np.concatenate([ts[4], ts[5]]))
        total = torch.nn.utils.clip_grad_norm_([p], 1.0)
        theirs = float(torch.clamp(1.0 / (total + 1e-6), max=1.0))
        assert check(float(coef)) and check(theirs), (kind, coef, theirs)


def test_the_clipped_element_is_mul_then_the_adam_restatement():
    p, g, m, v = U.adam_case(1029)
    for coef in (1.0, 0.25, 0.0, float("nan"), 0.3333):
        scaled = torch.from_numpy(g.copy()).mul(torch.tensor(coef, dtype=torch.float32)).numpy()
        assert U.same_bits(R.clip_grad(g, coef), scaled)
        want = U.adam_f32(p, scaled, m, v, SC)
        got = R.recipe_f32(p, g, m, v, SC, coef)
        assert all(U.same_bits(a, b) for a, b in zip(got[:3], want)) and got[3] is None
    assert all(U.same_bits(a, b) for a, b in zip(R.recipe_f32(p, g, m, v, SC)[:3], U.adam_f32(p, g, m, v, SC)))
    finite = np.isfinite(g)
    assert U.same_bits(R.clip_grad(g, 1.0)[finite], g[finite])                     # 1.0 leaves every finite g as it is


def test_the_ema_restatement_is_as_close_to_fp64_as_torch_lerp():
    n, steps = 65536, 20
    rng = np.random.default_rng(21)
    e0 = rng.normal(0, 0.05, n).astype(np.float32)
    ps = [(e0 + rng.normal(0, 1e-3, n)).astype(np.float32) for _ in range(steps)]
    for decay in (0.999, 0.9):
        omd = R.one_minus(decay)
        e32, e64, et = e0, e0.astype(np.float64), torch.from_numpy(e0.copy())
        for p in ps:
            e32 = R.ema_f32(e32, p, omd)
            e64 = R.ema_f64(e64, p, float(omd))
            et = torch.lerp(et, torch.from_numpy(p), float(omd))
        ours = float(np.abs(e32.astype(np.float64) - e64).max())
        theirs = float(np.abs(et.numpy().astype(np.float64) - e64).max())
        print(f"decay {decay}: max |restatement - fp64| = {ours:.3e}, max |torch.lerp - fp64| = {theirs:.3e}")
        assert theirs > 0 and ours <= 1.25 * theirs
