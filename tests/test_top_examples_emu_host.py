"""The top-examples kernels' own source, run on the CPU: csrc/top_examples.hip with csrc/topk_lists.h and
csrc/csr_lists.h is compiled for the host against the stand-in runtime of tests/emu (threads as lanes, real
barriers, __syncthreads_or) and must reproduce the numpy restatement bit for bit, fed in uneven batches through
one workspace, with guard words around keys, the workspace and the decoded outputs.  This checks what a GPU-less machine
can: the mark / count / scan / fill indexing, the per-wave rounds with their ballot compaction, rank merge and running
threshold, the dense form's LDS lists, row split and partial-list join, and the bounds of every write.  One line of the
source cannot compile for a host and is rewritten here: the dynamic-LDS declaration becomes a pointer to the emulator's
array."""
import numpy as np
import pytest

import top_examples_util as U
from emu_util import CSRC, compile_emu, rewrite, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("top_examples_emu")
    src = (CSRC / "top_examples.hip").read_text()
    src = rewrite(src, "extern __shared__ __attribute__((aligned(16))) unsigned char lds[];", "unsigned char* lds = g_lds;")
    for h in ("csr_lists.h", "topk_lists.h"):
        (d / h).write_text(rewrite((CSRC / h).read_text(), '#include "common.h"', f'#include "{CSRC / "common.h"}"'))
    (d / "top_examples_emu.hip").write_text(src)
    exe = compile_emu(d, "top_examples_emu.cpp", "top_examples_emu", include=(d,))

    def run(kind, head, H, n, floor, base, state, cuts):
        (np.zeros((H, n), np.uint64) if state is None else state).tofile(d / "state.bin")
        run_emu(exe, [kind] + list(head) + [H, n, repr(float(floor)), base, "state.bin", "out"] + cuts, d, 900)
        keys = np.fromfile(d / "out_keys.bin", np.uint64).reshape(H, n)
        got = (np.fromfile(d / "out_values.bin", np.float32).reshape(H, n), np.fromfile(d / "out_positions.bin", np.int64).reshape(H, n),
               np.fromfile(d / "out_counts.bin", np.int32))
        want = U.decode(keys)
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        return keys

    def compact(idx, val, H, n, cuts, floor=0.0, base=0, state=None):
        idx.tofile(d / "idx.bin")
        if val is not None:
            val.tofile(d / "val.bin")
        return run("compact", ["idx.bin", "-" if val is None else "val.bin", idx.shape[0], idx.shape[1]], H, n, floor, base, state, cuts)

    def dense(lat, H, n, cuts, floor=0.0, base=0, state=None):
        lat.tofile(d / "latent.bin")
        return run("dense", ["latent.bin", lat.shape[1], lat.shape[0]], H, n, floor, base, state, cuts)
    return compact, dense


# The GPU cases, with 300 x 65 x 1024 cut to 70 x 65 x 202 (k = 65 kept, three bitmap words, H no multiple of 4): a
# thread per lane makes the emulator's time grow with the number of workgroups, about 100 s for the full shape.
EMU_COMPACT_CASES = [c if c != (300, 65, 1024, 16) else (70, 65, 202, 16) for c in U.COMPACT_CASES]


@pytest.mark.parametrize("case", EMU_COMPACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_compact_source_on_the_host_equals_the_restatement(emu, case):
    B, k, H, n = case
    idx, val = U.compact_case(11 + B, B, k, H)
    want = U.restate(H, n, *U.candidates_compact(idx, val, H))
    assert np.array_equal(emu[0](idx, val, H, n, [0, B]), want)
    if 1 < B <= 300:
        assert np.array_equal(emu[0](idx, val, H, n, U.splits(B, 4)), want)      # uneven batches, one workspace


def test_compact_without_values_high_base_and_a_continued_state(emu):
    B, k, H, n = 70, 4, 40, 5
    idx, val = U.compact_case(5, B, k, H)
    base = 2 ** 32 - B
    got = emu[0](idx, None, H, n, [0, 1, 33, B], base=base)
    want = U.restate(H, n, *U.candidates_compact(idx, None, H, base))
    assert np.array_equal(got, want)
    idx2, val2 = U.compact_case(6, B, k, H)
    got2 = emu[0](idx2, val2, H, n, [0, B], floor=0.25, base=7, state=want)
    assert np.array_equal(got2, U.restate(H, n, *U.candidates_compact(idx2, val2, H, 7, 0.25), old=want))


@pytest.mark.parametrize("case", U.DENSE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dense_source_on_the_host_equals_the_restatement(emu, case):
    B, H, ld, n = case
    lat = U.dense_case(21 + B, B, H, ld)
    want = U.restate(H, n, *U.candidates_dense(lat, H))
    assert np.array_equal(emu[1](lat, H, n, [0, B]), want)                       # B > 64: rows split, partial lists joined
    if B > 1:
        assert np.array_equal(emu[1](lat, H, n, U.splits(B, 3)), want)


def test_dense_floor_high_base_and_a_continued_state(emu):
    B, H, ld, n = 150, 130, 136, 6
    lat = U.dense_case(9, B, H, ld)
    base = 2 ** 32 - B
    got = emu[1](lat, H, n, [0, 70, B], floor=0.5, base=base)
    want = U.restate(H, n, *U.candidates_dense(lat, H, base, 0.5))
    assert np.array_equal(got, want)
    assert (want[H - 1] == 0).all() and (want[:, -1] == 0).any()                  # an empty column; lists with a 0 tail
    lat2 = U.dense_case(10, B, H, ld)
    got2 = emu[1](lat2, H, n, [0, B], floor=-0.5, base=0, state=want)
    assert np.array_equal(got2, U.restate(H, n, *U.candidates_dense(lat2, H, 0, -0.5), old=want))
