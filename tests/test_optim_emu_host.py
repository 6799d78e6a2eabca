"""The optimizer kernels' own source, run on the CPU: csrc/optim.hip (with csrc/prefilter_common.h, which it shares with
qsae_prefilter_pack_w) is compiled for the host against the stand-in runtime of tests/emu (threads as lanes, real
barriers, the float shuffle with its width argument, the 32-bit atomicMax) and compared with the numpy restatement
of tests/optim_util.py, bit for bit.  Guard bytes around every buffer the entry points write show that nothing is written
outside them.  This checks what a GPU-less machine can: the indexing of both load widths and of the tail, the grid-stride
trips (the emulated grid is capped at 8 workgroups), the lane chains and their join, the workgroup maxima with idle waves
and idle lanes, and the hand-over of max |W'| through meta[0].  The source compiles for the host as it stands."""
import numpy as np
import pytest

import optim_util as U
from emu_util import CSRC, compile_emu, run_emu

SC = U.scalars()


def _scalar_bits(sc):
    return [str(int(np.float32(s).view(np.uint32))) for s in sc]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("optim_emu")
    src = (CSRC / "optim.hip").read_text()
    assert src.count('#include "prefilter_common.h"') == 1
    (d / "optim_emu.hip").write_text(src.replace('#include "prefilter_common.h"',
                                                 f'#include "{CSRC / "prefilter_common.h"}"'))
    exe = compile_emu(d, "optim_emu.cpp", "optim_emu", include=(d,), defines=("QSAE_ADAM_MAX_BLOCKS=8",))

    def run(cmd):
        run_emu(exe, cmd, d, 600)

    def adam(p, g, m, v, sc, shift_p=0, shift_g=0):
        n = p.size
        np.concatenate([p, g, m, v]).astype(np.float32).tofile(d / "in.bin")
        run(["adam", n, shift_p, shift_g] + _scalar_bits(sc) + ["in.bin", "out.bin"])
        out = np.fromfile(d / "out.bin", np.float32)
        assert out.size == 3 * n
        return out[:n], out[n:2 * n], out[2 * n:]

    def pref(w, b, sc):
        H, D = w[0].shape
        parts = [a.reshape(-1) for a in w] + ([a.reshape(-1) for a in b] if b is not None else [])
        np.concatenate(parts).astype(np.float32).tofile(d / "in.bin")
        run(["pref", H, D, int(b is not None)] + _scalar_bits(sc) + ["in.bin", "out.bin"])
        raw = (d / "out.bin").read_bytes()
        nw, nb = H * D * 4, (H * 4 if b is not None else 0)
        assert len(raw) == 3 * nw + 3 * nb + H * D * 2 + 16
        f = lambda off, count: np.frombuffer(raw, np.float32, count, off)          # noqa: E731
        wout = tuple(f(i * nw, H * D).reshape(H, D) for i in range(3))
        bout = tuple(f(3 * nw + i * nb, H) for i in range(3)) if b is not None else None
        Wq = np.frombuffer(raw, np.float16, H * D, 3 * nw + 3 * nb).reshape(H, D)
        meta = f(3 * nw + 3 * nb + H * D * 2, 4)
        return wout, bout, Wq, meta
    return adam, pref


@pytest.mark.parametrize("n", U.ADAM_SIZES)
def test_adam_step_source_on_the_host_equals_the_restatement(emu, n):
    p, g, m, v = U.adam_case(n)
    want = U.adam_f32(p, g, m, v, SC)
    if n >= 5:
        assert np.isnan(want[0]).sum() == 1 and np.isnan(want[1]).sum() == 1 and np.isnan(want[2]).sum() == 1
        huge = g == np.float32(1e20)
        assert huge.sum() == 1 and np.array_equal(want[0][huge], p[huge]) and np.isinf(want[2][huge]).all()
    # all pointers aligned (16-byte loads), p one element off, g one element off (element-wise loads): the same bits
    for shift_p, shift_g in ((0, 0), (1, 0), (0, 1)):
        got = emu[0](p, g, m, v, SC, shift_p, shift_g)
        for name, a, b in zip("pmv", got, want):
            assert U.same_bits(a, b), (n, shift_p, shift_g, name)


@pytest.mark.parametrize("case", U.PREF_CASES, ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}")
def test_adam_step_prefilter_source_on_the_host_equals_adam_then_pack_w(emu, case):
    H, D, variant = case
    w, b = U.pref_case(H, D, variant)
    wwant, bwant, Wq_want, meta_want = U.pref_expected(w, b, SC)
    wgot, bgot, Wq, meta = emu[1](w, b, SC)
    for name, a, c in zip(("W", "mW", "vW"), wgot, wwant):
        assert U.same_bits(a, c), name
    if b is not None:
        for name, a, c in zip(("bias", "mb", "vb"), bgot, bwant):
            assert U.same_bits(a, c), name
    assert U.same_bits(Wq, Wq_want)
    for i in range(4):
        assert U.same_bits(meta[i:i + 1], meta_want[i:i + 1]), (i, meta, meta_want)
    if variant == "zero":
        assert meta.tolist() == [1.0, 0.0, 0.0, 0.0] and not Wq.any()
    elif variant == "nan":
        # what pack_w makes of a NaN weight: no usable scale, a NaN norm, no measured distance, and a NaN copy
        assert meta[0] == 0 and np.isnan(meta[1]) and meta[3] == 0 and np.isnan(Wq).sum() >= 1
    else:
        assert meta[0] > 0 and meta[1] > 0 and meta[3] > 0 and (meta[2] > 0) == (b is not None)
