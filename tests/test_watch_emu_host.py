"""The watch kernels' own source, run on the CPU: csrc/watch.hip is compiled for the host against the stand-in runtime of
tests/emu (threads as lanes, real barriers, the 64-bit integer add on global memory) and compared with the
numpy restatement of tests/watch_util.py: every count, lo, hi and every fp64 word bit for bit.  Guard bytes around the
result block, the workspace and every tensor show that nothing is written outside them.  This checks what a GPU-less
machine can: the (tensor, chunk) table and its search, lists longer than one table, both load widths and the tail, the
ballot that joins the lanes of a bin, the LDS histogram and its flush, the order of every sum and the widened range.  The
source compiles for the host as it stands."""
import numpy as np
import pytest

import watch_util as U
from emu_util import CSRC, compile_emu, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("watch_emu")
    src = (CSRC / "watch.hip").read_text()
    assert src.count('#include "common.h"') == 1
    (d / "watch_emu.hip").write_text(src.replace('#include "common.h"', f'#include "{CSRC / "common.h"}"'))
    exe = compile_emu(d, "watch_emu.cpp", "watch_emu", include=(d,))

    def run(tensors, bins, shift=0):
        T = len(tensors)
        meta = np.array([[t.size, shift] for t in tensors], np.int64).reshape(-1)
        payload = np.array([T, bins], np.int64).tobytes() + meta.tobytes() + b"".join(np.ascontiguousarray(t, np.float32).tobytes() for t in tensors)
        (d / "in.bin").write_bytes(payload)
        run_emu(exe, ["in.bin", "out.bin"], d, 600)
        return np.fromfile(d / "out.bin", np.uint64).reshape(T, U.HEAD + bins)
    return run


@pytest.fixture(scope="module")
def lists():
    return U.case_lists()


@pytest.mark.parametrize("name,bins", U.RUNS, ids=U.RUN_IDS)
def test_tensor_stats_source_on_the_host_equals_the_restatement(emu, lists, name, bins):
    tensors = lists[name]
    got, want = emu(tensors, bins), U.restate_block(tensors, bins)
    for t in range(len(tensors)):
        assert np.array_equal(got[t], want[t]), (name, t, tensors[t].size, got[t][:8], want[t][:8])


def test_views_one_element_off_the_boundary_give_the_same_bits(emu, lists):
    for name in ("small", "chunks"):                           # (the aligned runs above equal the same restatement)
        assert np.array_equal(emu(lists[name], 64, shift=1), U.restate_block(lists[name], 64))


def test_no_tensor_and_no_element_launch_nothing(emu):
    assert emu([], 64).size == 0
    got = emu([np.zeros(0, np.float32)] * 3, 64)
    assert not got.any()
