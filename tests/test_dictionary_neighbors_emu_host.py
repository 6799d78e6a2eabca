"""The nearest-atom kernels' own source, run on the CPU: csrc/dictionary_neighbors.hip and csrc/topk_lists.h are compiled
for the host against the stand-in runtime of tests/emu (tests/emu_util.py: threads as lanes, real barriers, the MFMA
computed from the lane maps the source states) and must reproduce the numpy restatement bit for bit.  This checks what a GPU-less machine can:
indexing, the LDS layout, the append / merge rounds, the column split and the merge kernel, duplicate_of.  Two lines
of the source cannot compile for a host and are rewritten here: the dynamic-LDS declaration becomes a pointer to the
emulator's array, and the inline-asm register constraint "v" becomes "r"; the merge kernel's __shared__ array becomes
static."""
import numpy as np
import pytest

import dictionary_neighbors_util as U
from emu_util import CSRC, compile_emu, rewrite, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("nearest_atoms_emu")
    src = (CSRC / "dictionary_neighbors.hip").read_text()
    src = rewrite(src, "extern __shared__ __attribute__((aligned(16))) unsigned char lds[];", "unsigned char* lds = g_lds;")
    src = rewrite(src, '"+v"(rlh)', '"+r"(rlh)')
    src = rewrite(src, '#include "topk_lists.h"', '#include "topk_lists_emu.h"')
    hdr = (CSRC / "topk_lists.h").read_text()
    hdr = rewrite(hdr, "    __shared__ unsigned long long keys", "    static unsigned long long keys")
    hdr = rewrite(hdr, '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    (d / "dictionary_neighbors_emu.hip").write_text(src)
    (d / "topk_lists_emu.h").write_text(hdr)
    exe = compile_emu(d, "nearest_atoms_emu.cpp", "nearest_atoms_emu", include=(d,))

    def run(a, b, k, exclude_self=False, pad=0):
        D = a.shape[1]
        ld = D + pad

        def dump(x, name):
            w = np.full((x.shape[0], ld), 77, np.int8)          # garbage between D and ld
            w[:, :D] = x
            w.tofile(d / name)
        dump(a, "a.bin")
        if b is not None:
            dump(b, "b.bin")
        run_emu(exe, ["a.bin", a.shape[0], "-" if b is None else "b.bin", 0 if b is None else b.shape[0],
                      D, ld, k, int(exclude_self), int(b is None), "keys.bin", "dup.bin"], d, 600)
        keys = np.fromfile(d / "keys.bin", np.int64).reshape(a.shape[0], k)
        return keys, np.fromfile(d / "dup.bin", np.int32)
    return run


def _zeros_and_duplicates():
    z = U.ternary(8, 270, 32).copy()
    z[[3, 128, 129, 260]] = 0
    z[257] = z[5]
    return z


CASES = {
    "self_300_two_splits_merge_kernel": (lambda: U.ternary(5, 300, 64), None, 10, False, 48),
    "cross_33x65_int8": (lambda: U.full_int8(2, 33, 64), lambda: U.full_int8(3, 65, 64), 10, False, 16),
    "self_129_k64_exclude_self": (lambda: U.nbit(4, 129, 96), None, 64, True, 0),
    "identical_140_k64": (lambda: np.repeat(U.ternary(3, 1, 32), 140, 0), None, 64, False, 0),
    "zeros_and_duplicates_270": (_zeros_and_duplicates, None, 10, False, 0),
    "cross_3x2305_two_tiles_per_split": (lambda: U.nbit(11, 3, 32), lambda: U.nbit(12, 2305, 32), 10, False, 0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_source_on_the_host_equals_the_restatement(emu, case):
    fa, fb, k, excl, pad = CASES[case]
    a, b = fa(), (None if fb is None else fb())
    keys, dup = emu(a, b, k, excl, pad)
    assert np.array_equal(keys, U.reference_keys(a, b, k, excl))
    if b is None:
        assert np.array_equal(dup, U.reference_duplicate_of(a))
