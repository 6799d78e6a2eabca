"""The trainer kernels' own source, run on the CPU: csrc/trainer.hip is compiled for the host against the stand-in runtime
of tests/emu (threads as lanes, real barriers) and compared with the restatements of tests/trainer_util.py, bit
for bit, at the kernel shapes of the GPU tests.  Guard bytes around every buffer show that nothing is written outside them.
This checks what a GPU-less machine can: the indexing of both load widths (a base pointer moved off its 16-byte boundary
takes the element-wise path), rows past the end of the last bitmap word, indices outside the chunk, the tail of the last
slab, the lane / wave / workgroup joins of the loss sum and the chain of the rq_sae targets.  The source compiles for the
host as it stands."""
import numpy as np
import pytest
import torch

import trainer_util as U
from emu_util import CSRC, compile_emu, run_emu


def _raw(t: torch.Tensor) -> bytes:
    t = t.contiguous()
    return (t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)).numpy().tobytes()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("trainer_emu")
    src = (CSRC / "trainer.hip").read_text()
    assert src.count('#include "common.h"') == 1
    (d / "trainer_emu.hip").write_text(src.replace('#include "common.h"', f'#include "{CSRC / "common.h"}"'))
    exe = compile_emu(d, "trainer_emu.cpp", "trainer_emu", include=(d,))

    def run(cmd, payload: bytes) -> bytes:
        (d / "in.bin").write_bytes(payload)
        run_emu(exe, list(cmd) + ["in.bin", "out.bin"], d, 600)
        return (d / "out.bin").read_bytes()
    return run


BITMAP_D = (1, 5, 64, 512)


@pytest.mark.parametrize("dtype", list(U.TORCH_DTYPES))
@pytest.mark.parametrize("n_rows", U.BITMAP_ROWS)
def test_rows_nan_bitmap_source_on_the_host(emu, dtype, n_rows):
    """BITMAP_ROWS x D in {1, 5, 64, 512} x the three dtypes: no NaN (an inf instead), and a NaN in the first or last column
    of the first or last row; D = 8 also one element off its 16-byte boundary (whole pieces per row, element-wise path)."""
    for D, shift in [(D, 0) for D in BITMAP_D] + [(8, 1)]:
        corners = sorted({(0, 0), (0, D - 1), (n_rows - 1, 0), (n_rows - 1, D - 1)})
        for where in corners + [None]:
            src = torch.from_numpy(U.S.normal(n_rows, (n_rows, D), stream=3)).to(U.TORCH_DTYPES[dtype])
            src[src.numel() // 2 // D, 0] = float("inf")                        # inf is not NaN
            if where is not None:
                src[where] = float("nan")
            got = np.frombuffer(emu(["nan", U.DTYPE_CODES[dtype], n_rows, D, shift], _raw(src)), np.uint32)
            want = U.nan_bitmap_ref(src)
            assert np.array_equal(got, want), (D, shift, where)
            assert int(sum(bin(int(w)).count("1") for w in got)) == (0 if where is None else 1)


@pytest.mark.parametrize("dtype", list(U.TORCH_DTYPES))
@pytest.mark.parametrize("D", U.GATHER_D)
def test_gather_rows_source_on_the_host(emu, dtype, D):
    """GATHER_ROWS x GATHER_D x GATHER_B x the three dtypes, aligned; (300, 64) also one element off the 16-byte boundary
    and with indices -1 and n_rows."""
    cases = [(n_rows, B, 0) for n_rows in U.GATHER_ROWS for B in U.GATHER_B] + [(300, 64, 1)]
    for n_rows, B, shift in cases:
        src = U.special_chunk(n_rows, D, dtype)
        idx = U.gather_indices(n_rows, B)
        raw = emu(["gather", U.DTYPE_CODES[dtype], n_rows, D, B, shift], _raw(src) + idx.tobytes())
        out = np.frombuffer(raw, np.float32, B * D).reshape(B, D)
        assert U.same_bits(out, U.gather_ref(src, idx)), (n_rows, B, shift)
        assert np.frombuffer(raw, np.uint32, 1, B * D * 4)[0] == 0
        if (n_rows, B) == (300, 64):                                             # indices -1 and n_rows: zero rows, flag set
            idx[5], idx[9] = -1, n_rows
            raw = emu(["gather", U.DTYPE_CODES[dtype], n_rows, D, B, shift], _raw(src) + idx.tobytes())
            out = np.frombuffer(raw, np.float32, B * D).reshape(B, D)
            assert U.same_bits(out, U.gather_ref(src, idx)) and not out[5].any() and not out[9].any()
            assert np.frombuffer(raw, np.uint32, 1, B * D * 4)[0] == 1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", U.LOSS_LEVELS)
@pytest.mark.parametrize("shape", U.LOSS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_trainer_loss_source_on_the_host(emu, shape, n, mode):
    B, D = shape
    for coef, shift, equal in ((0.5, 0, None), (1.0, 1, 0)):
        x, recons = U.loss_case(B, D, n, equal_level=equal)
        raw = emu(["loss", n, B, D, mode, coef, shift], b"".join(a.tobytes() for a in [x] + recons))
        grads = np.frombuffer(raw, np.float32, n * B * D).reshape(n, B, D)
        losses = np.frombuffer(raw, np.float32, n, n * B * D * 4)
        want_l, want_g = U.loss_ref(x, recons, mode, coef)
        assert U.same_bits(losses, want_l), (coef, shift, losses, want_l)
        for i in range(n):
            assert U.same_bits(grads[i], want_g[i]), (coef, shift, i)
        if equal is not None:
            assert losses[0] == 0 and not grads[0].any()
