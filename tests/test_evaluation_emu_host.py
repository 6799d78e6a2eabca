"""The evaluation kernels' own source, run on the CPU: csrc/evaluation.hip is compiled for the host against the stand-in
runtime of tests/emu (threads as lanes, real barriers, the wave shuffles of floats, doubles and 64-bit keys) and
compared with the numpy restatement of tests/evaluation_util.py: the hard side, the counts and the moments for equality,
the soft side (which goes through this machine's expf) within the derived eps.  Guard bytes around the result block,
unit_err_sq, the running state and the workspace show that nothing is written outside them.  This checks what a GPU-less
machine can: the indexing of both load widths, the lane chains and their join, the per-quantity rows of the workspace, the
group cut, the NaN flags and the order of every sum.  The source compiles for the host as it stands."""
import numpy as np
import pytest

import evaluation_util as U
from emu_util import CSRC, compile_emu, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("evaluation_emu")
    src = (CSRC / "evaluation.hip").read_text()
    assert src.count('#include "common.h"') == 1
    (d / "evaluation_emu.hip").write_text(src.replace('#include "common.h"', f'#include "{CSRC / "common.h"}"'))
    exe = compile_emu(d, "evaluation_emu.cpp", "evaluation_emu", include=(d,))

    def run(cmd):
        run_emu(exe, cmd, d, 600)

    def quant(logits, D, n, step, shift=0):
        logits.tofile(d / "logits.bin")
        run(["qerr", "logits.bin", logits.shape[0], D, n, repr(step), repr(U.MARGIN), shift, "result.bin", "unit.bin"])
        return U.parse_block(np.fromfile(d / "result.bin", np.float64)), np.fromfile(d / "unit.bin", np.float64)

    def moments(x, recon, group_rows, cuts, state=None):
        B, D = x.shape
        x.tofile(d / "x.bin")
        if recon is not None:
            recon.tofile(d / "recon.bin")
        init = np.zeros(3 * D + 2, np.float64)
        if state is not None:
            init[:3 * D] = state[0].reshape(-1)
            init[3 * D:] = np.array(state[1:], np.int64).view(np.float64)
        init.tofile(d / "state.bin")
        dtype = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.uint16): 2}[x.dtype]
        run(["mom", "x.bin", dtype, B, D, group_rows, "recon.bin" if recon is not None else "-", "state.bin", "out.bin"] + cuts)
        out = np.fromfile(d / "out.bin", np.float64)
        kept, skipped = out[3 * D:].view(np.int64)
        return out[:3 * D].reshape(3, D), int(kept), int(skipped)
    return quant, moments


EMU_QUANT = [(c, v) for c in U.QUANT_CASES for v in ("plain", "tie", "nan")]


@pytest.mark.parametrize("case,variant", EMU_QUANT, ids=["x".join(map(str, c)) + "_" + v for c, v in EMU_QUANT])
def test_quantization_error_source_on_the_host(emu, case, variant):
    H, D, n = case
    step = U.step_of(n)
    logits = U.quant_logits(H, D, n, variant)
    got, unit = emu[0](logits, D, n, step)
    U.check_quant(got, unit, logits, D, n, step)
    if variant != "nan" and n > 1:
        assert got["flat"] == 3                            # the planted maximum; of two identical tuples the lower index


def test_the_scalar_loads_of_a_misaligned_n4_and_n8_matrix_give_the_same_bits(emu):
    for H, D, n in [(5, 20, 4), (8, 36, 8)]:
        logits = U.quant_logits(H, D, n)
        a, ua = emu[0](logits, D, n, U.step_of(n))
        b, ub = emu[0](logits, D, n, U.step_of(n), shift=1)
        assert a["key"] == b["key"] and np.array_equal(ua, ub)
        for name in ("sums", "abs", "pol", "und", "entry_logits"):
            assert np.array_equal(a[name], b[name])


def _moment_case(B, D, dtype, with_recon):
    x = U.moment_rows(B, D, dtype)
    xf = U.moments_as_f32(x)
    recon = (xf * np.float32(0.75) + np.float32(0.125)).astype(np.float32) if with_recon else None
    if B == 3000:
        xf[1500, 7] = np.nan                               # group 1 of 1024-row groups
        x = xf
    return x, xf, recon


@pytest.mark.parametrize("with_recon", [False, True], ids=["x", "x_recon"])
@pytest.mark.parametrize("case", U.MOMENT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dataset_moments_source_on_the_host_equals_the_restatement(emu, case, with_recon):
    B, D, dtype = case
    x, xf, recon = _moment_case(B, D, dtype, with_recon)
    group_rows = 1024
    want = U.moments_restate(xf, recon, group_rows)
    got = emu[1](x, recon, group_rows, [0, B])
    assert np.array_equal(got[0][:3 if with_recon else 2], want[0][:3 if with_recon else 2]) and got[1:] == want[1:]
    assert not got[0][2].any() or with_recon               # without recon the third row is not touched
    if B == 3000:
        assert got[1:] == (3000 - 1024, 1024)
    if B > 1024:
        cuts = sorted({0, min(group_rows, B), min(2 * group_rows, B), B})      # cut at multiples of group_rows: the same bits
        again = emu[1](x, recon, group_rows, cuts)
        assert np.array_equal(again[0], got[0]) and again[1:] == got[1:]


def test_moments_continue_a_state_and_take_odd_widths_and_cuts(emu):
    B, D = 70, 7                                           # D % 4 != 0: one column per thread
    x = U.moment_rows(B, D, "float32", seed=1)
    x[5, 2] = np.inf
    recon = (x * np.float32(0.5)).astype(np.float32)
    recon[5, 2] = 0.0
    first = U.moments_restate(x[:33], recon[:33], 16)
    got = emu[1](x[33:], recon[33:], 16, [0, 10, 37], state=first)     # rows 33.., cut off the vector boundary
    want = U.moments_restate(x[33:], recon[33:], 16, cuts=[0, 10, 37], state=first)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] == (70, 0)
    assert np.isinf(got[0][0][2]) and np.isinf(got[0][1][2])           # inf is summed, not skipped
