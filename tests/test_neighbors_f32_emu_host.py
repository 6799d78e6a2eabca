"""The fp32 nearest-atom kernel's own source, run on the CPU: csrc/dictionary_neighbors_f32.hip, csrc/gemm_mfma_f32.h
and csrc/topk_lists.h are compiled for the host against the stand-in runtime of tests/emu (threads as lanes, real
barriers, the fp32 MFMA computed from the lane maps the source states) and must reproduce the numpy
restatement bit for bit.  This checks what a GPU-less machine can: indexing, both loaders' addressing, the LDS layout
with the append buffer in the freed staging buffer, the four merge rounds, the candidate split and the merge kernel,
and that nothing is written outside `keys` and the workspace.  Lines of the source that cannot compile for a host are
rewritten here: the dynamic-LDS declaration becomes a pointer to the emulator's array, the asm-staged global load
becomes the plain load of the same address (base + 32-bit byte offset), the counted waits disappear, the register
constraint "v" becomes "x"; the merge kernel's __shared__ array becomes static."""
import re

import numpy as np
import pytest

import neighbors_f32_util as U
from emu_util import CSRC, compile_emu, rewrite, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("nearest_atoms_f32_emu")
    gemm = (CSRC / "gemm_mfma_f32.h").read_text()
    gemm = rewrite(gemm, 'asm volatile("s_nop 4\\n\\tglobal_load_dwordx4 %0, %1, %2" : "=v"(r[P][i]) : "v"(voff[i]), "s"(base) : "memory");',
                    "r[P][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + voff[i]);")
    gemm = rewrite(gemm, "extern __shared__ __attribute__((aligned(16))) float smem[];", "float* smem = reinterpret_cast<float*>(g_lds);")
    gemm, n = re.subn(r'asm volatile\("s_waitcnt vmcnt\((?:%0|0)\)" ::[^;]*;', ";", gemm)
    assert n == 5
    assert gemm.count('"+v"') == 3
    gemm = gemm.replace('"+v"', '"+x"')
    gemm = rewrite(gemm, '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    hdr = (CSRC / "topk_lists.h").read_text()
    hdr = rewrite(hdr, "    __shared__ unsigned long long keys", "    static unsigned long long keys")
    hdr = rewrite(hdr, '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    (d / "gemm_mfma_f32.h").write_text(gemm)
    (d / "topk_lists.h").write_text(hdr)
    (d / "dictionary_neighbors_f32_emu.hip").write_text((CSRC / "dictionary_neighbors_f32.hip").read_text())
    exe = compile_emu(d, "nearest_atoms_f32_emu.cpp", "nearest_atoms_f32_emu", include=(d,))

    def run(a, b, k, exclude_self=False, pad=0):
        D = a.shape[1]
        ld = D + pad

        def dump(x, name):
            w = np.full((x.shape[0], ld), np.nan, np.float32)       # NaN between D and ld
            w[:, :D] = x
            w.tofile(d / name)
        dump(a, "a.bin")
        if b is not None:
            dump(b, "b.bin")
        run_emu(exe, ["a.bin", a.shape[0], "-" if b is None else "b.bin", 0 if b is None else b.shape[0],
                      D, ld, k, int(exclude_self), "keys.bin"], d, 600)
        return np.fromfile(d / "keys.bin", np.int64).reshape(a.shape[0], k)
    return run


def _ordered():
    Nb = 1025
    x = (np.arange(Nb, dtype=np.float64) + 1) / (Nb + 1)
    b = np.zeros((Nb, 32), dtype=np.float32)
    b[:, 0], b[:, 1] = x, np.sqrt(1 - x * x)
    a = np.zeros((3, 32), dtype=np.float32)
    a[:, 0] = (1, 2, 3)
    return a, b


def _zeros():
    a = U.gaussian(8, 257, 8).copy()
    a[[3, 128, 129, 256]] = 0
    return a


CASES = {
    "cross_129x300_k_tail_three_splits": (lambda: (U.gaussian(5, 129, 36), U.gaussian(6, 300, 36)), 10, False, 12),
    "cross_5x1_d4": (lambda: (U.gaussian(2, 5, 4), U.gaussian(3, 1, 4)), 3, False, 0),
    "self_130_k64_exclude_self_asm_loader_form": (lambda: (U.gaussian(4, 130, 64), None), 64, True, 0),
    "ordered_3x1025_two_tiles_per_split": (_ordered, 10, False, 0),
    "identical_140_k64": (lambda: (np.repeat(U.gaussian(3, 1, 32), 140, 0), None), 64, False, 4),
    "self_257_zero_atoms_k7": (lambda: (_zeros(), None), 7, False, 0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_source_on_the_host_equals_the_restatement(emu, case):
    make, k, excl, pad = CASES[case]
    a, b = make()
    assert np.array_equal(emu(a, b, k, excl, pad), U.reference_keys(a, b, k, excl))
