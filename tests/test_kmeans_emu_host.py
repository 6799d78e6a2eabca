"""The k-means kernels' own source, run on the CPU: csrc/kmeans.hip with csrc/gemm_mfma_f32.h and csrc/csr_lists.h is
compiled for the host against the stand-in runtime of tests/emu (threads as lanes, real barriers, the fp32 MFMA as an
fmaf chain, the wave shuffles and integer atomics these kernels use) and must reproduce
the numpy restatement bit for bit.  This checks what a GPU-less machine can: indexing, both loaders' addressing, the
per-lane running keys and their join, the center split with the atomicMax join, the member lists, the chunk plan and
both summation orders, and that nothing is written outside the outputs and the workspace.  Lines of the source that
cannot compile for a host are rewritten as in tests/test_neighbors_f32_emu_host.py."""
import re

import numpy as np
import pytest

import kmeans_util as U
from emu_util import CSRC, compile_emu, rewrite, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmeans_emu")
    gemm = (CSRC / "gemm_mfma_f32.h").read_text()
    gemm = rewrite(gemm, 'asm volatile("s_nop 4\\n\\tglobal_load_dwordx4 %0, %1, %2" : "=v"(r[P][i]) : "v"(voff[i]), "s"(base) : "memory");',
                    "r[P][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + voff[i]);")
    gemm = rewrite(gemm, "extern __shared__ __attribute__((aligned(16))) float smem[];", "float* smem = reinterpret_cast<float*>(g_lds);")
    gemm, n = re.subn(r'asm volatile\("s_waitcnt vmcnt\((?:%0|0)\)" ::[^;]*;', ";", gemm)
    assert n == 5
    assert gemm.count('"+v"') == 3
    gemm = gemm.replace('"+v"', '"+x"')
    gemm = rewrite(gemm, '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    csr = rewrite((CSRC / "csr_lists.h").read_text(), '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    (d / "gemm_mfma_f32.h").write_text(gemm)
    (d / "csr_lists.h").write_text(csr)
    (d / "kmeans_emu.hip").write_text((CSRC / "kmeans.hip").read_text())
    exe = compile_emu(d, "kmeans_emu.cpp", "kmeans_emu", include=(d,))

    def dump(x, name, pad):
        w = np.full((x.shape[0], x.shape[1] + pad), np.nan, np.float32)     # NaN between D and ld
        w[:, :x.shape[1]] = x
        w.tofile(d / name)

    def run(cmd):
        run_emu(exe, cmd, d, 600)

    def assign(a, c, metric, pad=0):
        dump(a, "a.bin", pad)
        dump(c, "c.bin", pad)
        run(["assign", "a.bin", a.shape[0], "c.bin", c.shape[0], a.shape[1], a.shape[1] + pad, U.METRICS[metric], "keys.bin"])
        return np.fromfile(d / "keys.bin", np.int64)

    def update(a, labels, old, pad=0):
        dump(a, "a.bin", pad)
        dump(old, "old.bin", pad)
        labels.astype(np.int32).tofile(d / "labels.bin")
        C, D = old.shape
        run(["update", "a.bin", a.shape[0], D, D + pad, "labels.bin", C, "old.bin", "new.bin", "counts.bin", "stats.bin"])
        return (np.fromfile(d / "new.bin", np.float32).reshape(C, D), np.fromfile(d / "counts.bin", np.int32),
                np.fromfile(d / "stats.bin", np.float64))
    return assign, update


def _zeros():
    a = U.gaussian(8, 257, 64).copy()
    a[[3, 128, 129, 256]] = 0
    c = U.gaussian(9, 5, 64).copy()
    c[2] = 0
    return a, c


ASSIGN = {
    "129x300_d36_k_tail_three_splits": (lambda: (U.gaussian(5, 129, 36), U.gaussian(6, 300, 36)), 12),
    "5x1_d4": (lambda: (U.gaussian(2, 5, 4), U.gaussian(3, 1, 4)), 0),
    "identical_centers_140x9": (lambda: (U.gaussian(4, 140, 32), np.repeat(U.gaussian(3, 1, 32), 9, 0)), 4),
    "zero_atoms_and_a_zero_center_asm_loader_form": (_zeros, 0),
}


@pytest.mark.parametrize("metric", sorted(U.METRICS))
@pytest.mark.parametrize("case", sorted(ASSIGN))
def test_assign_source_on_the_host_equals_the_restatement(emu, case, metric):
    make, pad = ASSIGN[case]
    a, c = make()
    keys = emu[0](a, c, metric, pad)
    assert np.array_equal(keys, U.assign_keys(a, c, metric))
    if case.startswith("identical"):
        assert (U.labels_of(keys) == 0).all()                  # equal bits go to the lowest center
    if case.startswith("zero") and metric == "cosine":
        assert (U.labels_of(keys)[[3, 128, 129, 256]] == 0).all()   # cosine +0 with every center


def _big_cluster():
    n_big = 2 * U.KMEANS_CHUNK + 3
    # -1 and 4 lie outside [0, C): skipped
    labels = np.concatenate([np.zeros(n_big), np.full(40, 2), np.full(29, 3), [-1, -1, 4]]).astype(np.int32)
    labels = labels[np.argsort(U.S.uniform01(17, labels.size, stream=46), kind="stable")]
    return U.gaussian(12, labels.size, 36), labels, U.gaussian(13, 4, 36)


UPDATE = {
    "big_cluster_empty_cluster_skipped_labels": (_big_cluster, 4),
    "c1_n5_d4": (lambda: (U.gaussian(14, 5, 4), np.zeros(5, np.int32), U.gaussian(15, 1, 4)), 0),
    "d260_two_slabs": (lambda: (U.gaussian(16, 70, 260), (np.arange(70) % 3).astype(np.int32), U.gaussian(17, 3, 260)), 0),
}


@pytest.mark.parametrize("case", sorted(UPDATE))
def test_update_source_on_the_host_equals_the_restatement(emu, case):
    make, pad = UPDATE[case]
    a, labels, old = make()
    new, counts, stats = emu[1](a, labels, old, pad)
    rnew, rcounts, rstats = U.update(a, labels, old)
    assert np.array_equal(counts, rcounts)
    assert np.array_equal(new.view(np.int32), rnew.view(np.int32))
    assert np.array_equal(stats, rstats)
    if case.startswith("big"):
        assert counts[0] == 2 * U.KMEANS_CHUNK + 3 and counts[1] == 0 and stats[1] == 1
        assert np.array_equal(new[1], old[1])                  # an empty cluster keeps its center
