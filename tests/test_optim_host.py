"""The optimizer's host surface; runs without a GPU: the two new C-ABI entry points and their argument checks, the dispatcher
schemas, quantizedsae_amd.optim.Adam's constructor, state dicts going back and forth with torch.optim.Adam, the refusal of
CPU parameters, and the restatement the GPU and emulation tests compare against, pinned to torch's own Adam."""
import copy
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import optim_util as U
from quantizedsae_amd import BinarySAE, TernarySparseAutoencoder, _lib
from quantizedsae_amd import torch_ops  # noqa: F401  (registers torch.ops.qsae.*)
from quantizedsae_amd.optim import Adam

ROOT = Path(__file__).resolve().parents[1]
P = ctypes.c_void_p


def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("qsae_adam_step", "qsae_adam_step_prefilter"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.load().qsae_abi_version() == _lib.ABI_VERSION == 4
    assert "optim.hip" in __import__("quantizedsae_amd.build", fromlist=["SOURCES"]).SOURCES


def test_invalid_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    s = (0.1, 0.999, 0.001, 0.05, 1e-8, 1e-3)
    a, b = P(4096), P(4096 + 4)
    assert lib.qsae_adam_step(None, a, a, a, 8, *s, None) == _lib.ERR_INVALID_ARG
    assert b"invalid argument" in lib.qsae_last_error() and b"qsae_adam_step" in lib.qsae_last_error()
    assert lib.qsae_adam_step(a, None, a, a, 8, *s, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_adam_step(a, a, None, a, 8, *s, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_adam_step(a, a, a, None, 8, *s, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_adam_step(a, a, a, a, -1, *s, None) == _lib.ERR_INVALID_ARG
    assert lib.qsae_adam_step(a, a, a, a, 0, *s, None) == _lib.OK             # nothing to do, nothing launched
    assert lib.qsae_adam_step(None, None, None, None, 0, *s, None) == _lib.OK  # an empty tensor's pointers are null
    assert lib.qsae_adam_step(None, None, None, None, -1, *s, None) == _lib.ERR_INVALID_ARG

    def pref(W=a, gW=a, mW=a, vW=a, bias=a, gb=a, mb=a, vb=a, H=8, D=64, Wq=a, meta=a):
        return lib.qsae_adam_step_prefilter(W, gW, mW, vW, bias, gb, mb, vb, H, D, *s, Wq, meta, None)
    assert pref(H=0) == _lib.ERR_INVALID_ARG and pref(D=0) == _lib.ERR_INVALID_ARG
    for name in ("W", "gW", "mW", "vW", "Wq", "meta"):
        assert pref(**{name: None}) == _lib.ERR_INVALID_ARG, name
    for name in ("bias", "gb", "mb", "vb"):                                     # a half-null bias quadruple
        assert pref(**{name: None}) == _lib.ERR_INVALID_ARG, name
        assert b"all null or all non-null" in lib.qsae_last_error()
    assert pref(Wq=b) == _lib.ERR_INVALID_ARG and b"16-byte aligned" in lib.qsae_last_error()
    assert pref(W=b) == _lib.ERR_INVALID_ARG


def test_op_schemas_list_the_mutated_arguments():
    def written(op):
        return [a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    assert written(torch.ops.qsae.adam_step) == ["p", "m", "v"]
    assert written(torch.ops.qsae.adam_step_prefilter) == ["W", "mW", "vW", "bias", "mb", "vb", "Wq", "meta"]
    # fake registrations: the ops trace without a device
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        t = torch.empty(8, 64)
        assert torch.ops.qsae.adam_step(t, t, t, t, 0.1, 0.999, 0.001, 0.05, 1e-8, 1e-3) is None
        assert torch.ops.qsae.adam_step_prefilter(t, t, t, t, None, None, None, None, 0.1, 0.999, 0.001, 0.05, 1e-8, 1e-3,
                                                  torch.empty(8, 64, dtype=torch.float16), torch.empty(4)) is None


def test_constructor_rejections_name_the_option():
    w = torch.nn.Parameter(torch.zeros(4, 4))
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(capturable=True),
               dict(differentiable=True), dict(fused=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Adam([w], **kw)
    with pytest.raises(ValueError, match="weight_decay"):
        Adam([{"params": [w], "weight_decay": 0.1}])
    assert Adam([w], foreach=True).param_groups[0]["foreach"] is True      # kept as given: there is one implementation
    assert Adam([w], fused=False, weight_decay=0.0).param_groups[0]["fused"] is False
    with pytest.raises(ValueError, match="fp32"):
        Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        Adam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError):
        Adam([w], lr=-1.0)
    opt = Adam([w], lr=3e-4, betas=(0.8, 0.99), eps=1e-6)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"]) == (3e-4, (0.8, 0.99), 1e-6)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "amsgrad": True})
    assert len(opt.param_groups) == 1
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "lr": 1.0})
    assert [g["lr"] for g in opt.param_groups] == [3e-4, 1.0]
    # model= takes any model; only the top-k classes have the encoder state the fused route installs
    assert Adam(TernarySparseAutoencoder(16, 64).parameters(), model=TernarySparseAutoencoder(16, 64))._model is None
    m = BinarySAE(16, 64, gamma=4.0, n_bits=4)
    assert Adam(m.parameters(), model=m)._model is m


def _stepped_torch_adam(params):
    opt = torch.optim.Adam(params, lr=1e-2)
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, 0.5 + i)
    opt.step()
    return opt


def _assert_same_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (k, name)


def test_state_dict_round_trips_with_torch_adam_on_the_cpu():
    params = [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]
    theirs = _stepped_torch_adam(params)                       # a real CPU step makes the state
    ours = Adam(params, lr=5.0)
    ours.load_state_dict(copy.deepcopy(theirs.state_dict()))   # (load_state_dict keeps same-device tensors as they are)
    _assert_same_state(ours.state_dict(), theirs.state_dict())
    assert ours.param_groups[0]["lr"] == 1e-2
    step = ours.state[params[0]]["step"]
    assert step.dtype == torch.float32 and step.device.type == "cpu" and float(step) == 1.0
    back = torch.optim.Adam(params, lr=7.0)
    back.load_state_dict(copy.deepcopy(ours.state_dict()))
    _assert_same_state(back.state_dict(), theirs.state_dict())
    before = [p.detach().clone() for p in params]
    back.step()                                                # and torch's Adam continues from it
    assert float(back.state[params[0]]["step"]) == 2.0 and not torch.equal(before[0], params[0])
    # a fresh one of ours has the group keys torch's Adam reads
    assert set(Adam(params).state_dict()["param_groups"][0]) == set(torch.optim.Adam(params).state_dict()["param_groups"][0])


def test_cpu_parameters_raise_at_step():
    p = torch.nn.Parameter(torch.zeros(8))
    opt = Adam([p])
    opt.step()                                                 # nothing has a gradient: nothing to do, as in torch
    assert len(opt.state) == 0
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert not p.detach().any() and len(opt.state) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.qsae.adam_step(p.detach(), p.grad, torch.zeros(8), torch.zeros(8), 0.1, 0.999, 0.001, 0.05, 1e-8, 1e-3)
    opt.zero_grad()
    assert p.grad is None
    calls = []
    assert opt.step(lambda: calls.append(torch.is_grad_enabled()) or 1.5) == 1.5 and calls == [True]


def _multi_step_grads(n, steps):
    rng = np.random.default_rng(11)
    out = []
    for _ in range(steps):
        g = U.bulk_grad(rng, n)
        U.plant(g, np.zeros(n, np.float32), np.zeros(n, np.float32), plants=("zero", "tiny", "negzero"))
        out.append(g)
    return out


@pytest.fixture(scope="module")
def pinned():
    """20 steps over 65536 elements: the fp32 restatement and the fp64 ruler, computed once."""
    n, steps, lr = 65536, 20, 1e-3
    p0 = np.random.default_rng(10).normal(0, 0.05, n).astype(np.float32)
    grads = _multi_step_grads(n, steps)
    z = np.zeros(n, np.float32)
    r32, r64 = (p0, z, z), (p0.astype(np.float64), z.astype(np.float64), z.astype(np.float64))
    for t, g in enumerate(grads, 1):
        sc = U.scalars(lr=lr, t=t)
        r32 = U.adam_f32(r32[0], g, r32[1], r32[2], sc)
        r64 = U.adam_f64(r64[0], g, r64[1], r64[2], sc)
    return p0, grads, lr, r32[0], r64[0]


@pytest.mark.parametrize("foreach", [False, True])
def test_the_restatement_is_as_close_to_fp64_as_torch_adam_on_the_cpu(pinned, foreach):
    p0, grads, lr, r32, r64 = pinned
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=lr, foreach=foreach)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    ours = float(np.abs(r32.astype(np.float64) - r64).max())
    theirs = float(np.abs(p.detach().numpy().astype(np.float64) - r64).max())
    differ = float((p.detach().numpy().view(np.uint32) != r32.view(np.uint32)).mean())
    print(f"foreach={foreach}: max |restatement - fp64| = {ours:.3e}, max |torch - fp64| = {theirs:.3e}, "
          f"ratio {ours / theirs:.3f}, elements that differ from torch {differ:.2%}")
    assert np.isfinite(r32).all() and theirs > 0
    assert ours <= 1.25 * theirs
