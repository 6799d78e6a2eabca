"""The recipe kernels' own source, run on the CPU: csrc/optim_recipe.hip is compiled for the host against the stand-in runtime
of tests/emu and compared with the numpy restatements of tests/optim_recipe_util.py, bit for bit -- once plain and once as a
stand-alone AddressSanitizer executable.  The grid of the flat step is capped at 8 workgroups; guard bytes surround every
buffer, and the driver also checks that read-only operands kept their bytes.  This checks what a GPU-less machine can: the
chunk table and the tails of the norm, the fp64 order, the coefficient's corners, the strips, chains and join of the
projection, both load widths and the tail of the step with either stream, and the encoder pair's hand-over to pack_w."""
import numpy as np
import pytest

import optim_recipe_util as R
import optim_util as U
from emu_util import CSRC, compile_emu, run_emu

SC = U.scalars()
OMD = R.one_minus(R.DECAY)


def _bits(x):
    return str(int(np.float32(x).view(np.uint32)))


def _scalar_bits(sc):
    return [_bits(s) for s in sc]


def _coef_arg(coef):
    return "null" if coef is None else _bits(coef)


class Emu:
    def __init__(self, d, exe):
        self.d, self.exe = d, exe

    def run(self, cmd):
        run_emu(self.exe, cmd, self.d, 900)

    def norm(self, tensors, max_norm, shifted=R.NORM_SHIFTED):
        T = len(tensors)
        np.concatenate([np.asarray(t, np.float32).reshape(-1) for t in tensors]).tofile(self.d / "in.bin")
        self.run(["norm", T, shifted, repr(float(max_norm)), ",".join(str(t.size) for t in tensors), "in.bin", "out.bin"])
        raw = (self.d / "out.bin").read_bytes()
        assert len(raw) == 4 + 8 * (R.HEAD + T)
        return np.frombuffer(raw, np.float32, 1)[0], np.frombuffer(raw, np.int64, R.HEAD + T, 4)

    def project(self, W, G, H):
        D, ld = W.shape
        np.concatenate([W.reshape(-1), G.reshape(-1)]).astype(np.float32).tofile(self.d / "in.bin")
        self.run(["proj", D, H, ld, "in.bin", "out.bin"])
        return np.fromfile(self.d / "out.bin", np.float32).reshape(D, ld)

    def adam(self, p, g, m, v, sc, coef=None, ema=None, omd=OMD, shift_p=0, shift_g=0):
        n = p.size
        np.concatenate([p, g, m, v] + ([ema] if ema is not None else [])).astype(np.float32).tofile(self.d / "in.bin")
        self.run(["adam", n, shift_p, shift_g] + _scalar_bits(sc) + [_coef_arg(coef), int(ema is not None), _bits(omd),
                                                                   "in.bin", "out.bin"])
        out = np.fromfile(self.d / "out.bin", np.float32)
        assert out.size == (4 if ema is not None else 3) * n
        return tuple(out[i * n:(i + 1) * n] for i in range(out.size // n)) + ((None,) if ema is None else ())

    def pref(self, w, b, sc, coef=None, ema=None, omd=OMD):
        """ema: (eW, eb or None) or None -> (W', mW', vW'), (b', mb', vb') or None, (eW', eb') or None, Wq, meta"""
        H, D = w[0].shape
        parts = [a.reshape(-1) for a in w] + ([a.reshape(-1) for a in b] if b is not None else [])
        if ema is not None:
            parts += [ema[0].reshape(-1)] + ([ema[1]] if b is not None else [])
        np.concatenate(parts).astype(np.float32).tofile(self.d / "in.bin")
        self.run(["pref", H, D, int(b is not None)] + _scalar_bits(sc) + [_coef_arg(coef), int(ema is not None), _bits(omd),
                                                                         "in.bin", "out.bin"])
        raw = (self.d / "out.bin").read_bytes()
        nw, nb = H * D * 4, (H * 4 if b is not None else 0)
        ne = (nw + nb) if ema is not None else 0
        assert len(raw) == 3 * nw + 3 * nb + ne + H * D * 2 + 16
        f = lambda off, count: np.frombuffer(raw, np.float32, count, off)          # noqa: E731
        wout = tuple(f(i * nw, H * D).reshape(H, D) for i in range(3))
        bout = tuple(f(3 * nw + i * nb, H) for i in range(3)) if b is not None else None
        at = 3 * nw + 3 * nb
        eout = None
        if ema is not None:
            eout = (f(at, H * D).reshape(H, D), f(at + nw, H) if b is not None else None)
        Wq = np.frombuffer(raw, np.float16, H * D, at + ne).reshape(H, D)
        return wout, bout, eout, Wq, f(at + ne + H * D * 2, 4)


@pytest.fixture(scope="module", params=["plain", "asan"])
def emu(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("optim_recipe_emu_" + request.param)
    exe = compile_emu(d, "optim_recipe_emu.cpp", "optim_recipe_emu", include=(CSRC,), defines=("QSAE_ADAM_MAX_BLOCKS=8",),
                      asan=request.param == "asan")
    return Emu(d, exe)


@pytest.fixture(scope="module")
def plain_adam(tmp_path_factory):
    """qsae_adam_step of csrc/optim.hip on the same runtime (the driver of tests/test_optim_emu_host.py)"""
    d = tmp_path_factory.mktemp("optim_emu_for_recipe")
    src = (CSRC / "optim.hip").read_text()
    (d / "optim_emu.hip").write_text(src.replace('#include "prefilter_common.h"', f'#include "{CSRC / "prefilter_common.h"}"'))
    exe = compile_emu(d, "optim_emu.cpp", "optim_emu", include=(d,), defines=("QSAE_ADAM_MAX_BLOCKS=8",))

    def adam(p, g, m, v, sc, shift_p=0, shift_g=0):
        n = p.size
        np.concatenate([p, g, m, v]).astype(np.float32).tofile(d / "in.bin")
        run_emu(exe, ["adam", n, shift_p, shift_g] + _scalar_bits(sc) + ["in.bin", "out.bin"], d, 600)
        return (d / "out.bin").read_bytes()
    return adam


# ---- the norm ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bulk_norm():
    ts = R.norm_case("bulk")
    return ts, float(R.grad_norm(ts, 1.0)[1].view(np.float64)[1])


@pytest.mark.parametrize("side", ["below", "above"])
def test_grad_norm_source_on_the_host_equals_the_restatement(emu, bulk_norm, side):
    ts, norm = bulk_norm
    max_norm = norm * (0.5 if side == "below" else 2.0)
    coef, words = emu.norm(ts, max_norm)
    want_coef, want = R.grad_norm(ts, max_norm)
    assert R.same_report(words, want)
    assert U.same_bits(np.float32(coef), want_coef)
    f = words.view(np.float64)
    assert f[R.HEAD] == 0.0 and f[R.HEAD + 1] == float(ts[1][0]) ** 2       # the empty tensor, the tensor of one element
    if side == "below":
        assert words[3] == 1 and abs(coef - 0.5) < 1e-6
    else:
        assert words[3] == 0 and coef == 1.0
    # the tensor that starts off its boundary is read element by element: the same bits as on the boundary
    _, aligned = emu.norm(ts, max_norm, shifted=-1)
    assert np.array_equal(aligned, words)


@pytest.mark.parametrize("kind", ["zeros", "inf", "nan"])
def test_grad_norm_corners_on_the_host(emu, kind):
    ts = R.norm_case(kind)
    coef, words = emu.norm(ts, 1.0)
    want_coef, want = R.grad_norm(ts, 1.0)
    assert R.same_report(words, want) and U.same_bits(np.float32(coef), want_coef)
    f = words.view(np.float64)
    if kind == "zeros":
        assert f[1] == 0.0 and coef == 1.0 and words[3] == 0
    elif kind == "inf":
        assert np.isinf(f[1]) and coef == 0.0 and words[3] == 1
    else:
        assert np.isnan(f[1]) and np.isnan(coef) and words[3] == 1


# ---- the projection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PROJECT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_project_columns_source_on_the_host_equals_the_restatement(emu, case):
    D, H, ld = case
    W, G = R.project_case(D, H, ld)
    got = emu.project(W, G, H)
    want = R.project_columns(W, G, H)
    assert U.same_bits(got, want)
    assert np.array_equal(got[:, H:].view(np.uint32), G[:, H:].view(np.uint32))          # ld > H: not touched
    for col in (2, 3):                                                                # the zero columns keep their bits
        assert np.array_equal(got[:, col].view(np.uint32), G[:, col].view(np.uint32))
    if H >= 8:
        assert np.isnan(got[:, 5]).all() and not np.isnan(got[:, [4, 6]]).any()      # the NaN stays in its column
    # a unit-norm column comes out orthogonal to its atom, to rounding
    rel = abs(np.dot(got[:, 0].astype(np.float64), W[:, 0])) / max(np.abs(G[:, 0]).sum(), 1e-30)
    assert rel < 1e-5


# ---- the step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", U.ADAM_SIZES)
def test_recipe_step_source_on_the_host_equals_the_restatement(emu, plain_adam, n):
    p, g, m, v = U.adam_case(n)
    e = R.ema_case(n)
    for coef in R.COEFS:
        for with_ema in (False, True):
            want = R.recipe_f32(p, g, m, v, SC, coef, e if with_ema else None, OMD)
            # all pointers aligned (16-byte loads); p one element off (element-wise loads): the same bits
            for shift_p in (0, 1):
                got = emu.adam(p, g, m, v, SC, coef, e if with_ema else None, shift_p=shift_p)
                for name, a, b in zip("pmve", got, want):
                    assert (a is None and b is None) or U.same_bits(a, b), (n, coef, with_ema, shift_p, name)
    # neither stream: qsae_adam_step's output byte for byte, in both load widths
    for shift_p, shift_g in ((0, 0), (0, 1)):
        got = emu.adam(p, g, m, v, SC, shift_p=shift_p, shift_g=shift_g)
        assert np.concatenate(got[:3]).tobytes() == plain_adam(p, g, m, v, SC, shift_p, shift_g)


@pytest.mark.parametrize("case", U.PREF_CASES, ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}")
def test_recipe_pair_source_on_the_host_equals_the_step_then_pack_w(emu, case):
    H, D, variant = case
    w, b = U.pref_case(H, D, variant)
    eW = R.ema_case(H * D).reshape(H, D)
    eb = R.ema_case(H) if b is not None else None
    for coef, with_ema in ((None, False), (0.25, False), (None, True), (0.25, True), (float("nan"), True)):
        W2, mW2, vW2, eW2 = R.recipe_f32(*w, SC, coef, eW if with_ema else None, OMD)
        b2 = R.recipe_f32(*b, SC, coef, eb if with_ema else None, OMD) if b is not None else None
        Wq_want, meta_want = U.pack_w(W2, b2[0] if b2 is not None else None)
        wgot, bgot, egot, Wq, meta = emu.pref(w, b, SC, coef, (eW, eb) if with_ema else None)
        for name, a, c in zip(("W", "mW", "vW"), wgot, (W2, mW2, vW2)):
            assert U.same_bits(a, c), (coef, with_ema, name)
        if b is not None:
            for name, a, c in zip(("bias", "mb", "vb"), bgot, b2[:3]):
                assert U.same_bits(a, c), (coef, with_ema, name)
        if with_ema:
            assert U.same_bits(egot[0], eW2)
            assert b is None or U.same_bits(egot[1], b2[3])
        assert U.same_bits(Wq, Wq_want), (coef, with_ema)
        for i in range(4):
            assert U.same_bits(meta[i:i + 1], meta_want[i:i + 1]), (coef, with_ema, i, meta, meta_want)
