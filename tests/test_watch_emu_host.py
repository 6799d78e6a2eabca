"""The watch kernels' own source, run on the CPU: csrc/watch.hip is compiled for the host against the stand-in runtime of
tests/emu_trainer (threads as lanes, real barriers; tests/emu_watch adds the 64-bit integer add) and compared with the
numpy restatement of tests/watch_util.py: every count, lo, hi and every fp64 word bit for bit.  Guard bytes around the
result block, the workspace and every tensor show that nothing is written outside them.  This checks what a GPU-less
machine can: the (tensor, chunk) table and its search, lists longer than one table, both load widths and the tail, the
ballot that joins the lanes of a bin, the LDS histogram and its flush, the order of every sum and the widened range.  The
source compiles for the host as it stands."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import watch_util as U
from test_dictionary_neighbors_emu_host import _clangxx

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "quantizedsae_amd" / "csrc"
EMU = ROOT / "tests" / "emu_watch"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("watch_emu")
    src = (CSRC / "watch.hip").read_text()
    assert src.count('#include "common.h"') == 1
    (d / "watch_emu.hip").write_text(src.replace('#include "common.h"', f'#include "{CSRC / "common.h"}"'))
    exe = d / "watch_emu"
    r = subprocess.run([_clangxx(), "-O1", "-std=c++17", "-ffp-contract=off", "-x", "c++", f"-I{EMU}", f"-I{d}", "-pthread",
                        str(EMU / "watch_emu.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(tensors, bins, shift=0):
        T = len(tensors)
        meta = np.array([[t.size, shift] for t in tensors], np.int64).reshape(-1)
        payload = np.array([T, bins], np.int64).tobytes() + meta.tobytes() + b"".join(np.ascontiguousarray(t, np.float32).tobytes() for t in tensors)
        (d / "in.bin").write_bytes(payload)
        r = subprocess.run([str(exe), "in.bin", "out.bin"], cwd=d, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
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
