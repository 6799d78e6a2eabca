"""The AuxK kernels' own source, run on the CPU: csrc/auxk.hip, csrc/gemm_mfma_f32.h and csrc/topk_lists.h are compiled for
the host against the stand-in runtime of tests/emu (threads as lanes, real barriers, the fp32 MFMA, the
shuffle of doubles) and must reproduce the numpy restatements of tests/auxk_util.py bit for bit.  This
checks what a GPU-less machine can: the loader's addressing through the unit list, the bias seed of the accumulators, the
candidate split and the merge, the key decode, the loss kernels' indexing and summation order, and that nothing is written
outside the outputs and the workspace (which arrives poisoned and is used twice).  The case whose list holds an entry below
0 and one at or above H runs here only, in a build with AddressSanitizer on top (a stand-alone host program): every operand
is a heap block of exactly its size, so a read outside W, bias, x or the list would stop it.  The source lines that cannot
compile for a host are rewritten as in tests/test_neighbors_f32_emu_host.py."""
import re
from pathlib import Path

import numpy as np
import pytest

import auxk_util as U
from emu_util import CSRC, ROOT, compile_emu, rewrite, run_emu


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("auxk_emu")
    gemm = (CSRC / "gemm_mfma_f32.h").read_text()
    gemm = rewrite(gemm, 'asm volatile("s_nop 4\\n\\tglobal_load_dwordx4 %0, %1, %2" : "=v"(r[P][i]) : "v"(voff[i]), "s"(base) : "memory");',
                    "r[P][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + voff[i]);")
    gemm = rewrite(gemm, "extern __shared__ __attribute__((aligned(16))) float smem[];", "float* smem = reinterpret_cast<float*>(g_lds);")
    gemm, n = re.subn(r'asm volatile\("s_waitcnt vmcnt\((?:%0|0)\)" ::[^;]*;', ";", gemm)
    assert n == 5
    assert gemm.count('"+v"') == 3
    gemm = gemm.replace('"+v"', '"+x"')
    gemm = rewrite(gemm, '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    hdr = rewrite((CSRC / "topk_lists.h").read_text(), '#include "common.h"', f'#include "{CSRC / "common.h"}"')
    src = rewrite((CSRC / "auxk.hip").read_text(), '#include "../../include/qsae_ext.h"',
                   f'#include "{ROOT / "include" / "qsae_ext.h"}"')
    (d / "gemm_mfma_f32.h").write_text(gemm)
    (d / "topk_lists.h").write_text(hdr)
    (d / "auxk_emu.hip").write_text(src)
    return d


def _run_topk(exe: Path, d: Path, x, W, bias, units, k, pad_x=0, pad_w=0):
    B, D = x.shape
    H = W.shape[0]

    def dump(a, pad, name):
        w = np.full((a.shape[0], D + pad), np.nan, np.float32)      # NaN between D and the row stride
        w[:, :D] = a
        w.tofile(d / name)
    dump(x, pad_x, "x.bin")
    dump(W, pad_w, "w.bin")
    if bias is not None:
        np.ascontiguousarray(bias, dtype=np.float32).tofile(d / "bias.bin")
    np.ascontiguousarray(units, dtype=np.int32).tofile(d / "units.bin")
    run_emu(exe, ["topk", "x.bin", B, "w.bin", H, "-" if bias is None else "bias.bin", "units.bin", len(units), D, D + pad_x,
                  D + pad_w, k, "idx.bin", "val.bin"], d, 900)
    return np.fromfile(d / "idx.bin", np.int32).reshape(B, k), np.fromfile(d / "val.bin", np.float32).reshape(B, k)


@pytest.fixture(scope="module")
def emu(build_dir):
    return compile_emu(build_dir, "auxk_emu.cpp", "auxk_emu", include=(build_dir,))


@pytest.fixture(scope="module")
def emu_asan(build_dir):
    return compile_emu(build_dir, "auxk_emu.cpp", "auxk_emu_asan", include=(build_dir,), asan=True)


def _same(got, want):
    gi, gv = got
    wi, wv = want
    assert np.array_equal(gi, wi)
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32))


@pytest.mark.parametrize("name", sorted(U.TOPK_SHAPES))
def test_subset_topk_source_on_the_host_equals_the_restatement(emu, build_dir, name):
    x, W, bias, units, k = U.topk_case(name)
    pad = 4 if name == "two_panels_k_tail_split_2" else 0          # row strides beyond D on both operands
    _same(_run_topk(emu, build_dir, x, W, bias, units, k, pad, 2 * pad), U.subset_topk(x, W, bias, units, k))


def test_subset_topk_without_a_bias(emu, build_dir):
    x, W, _, units, k = U.topk_case("k_equals_n")
    _same(_run_topk(emu, build_dir, x, W, None, units, k), U.subset_topk(x, W, None, units, k))


def test_entries_outside_the_dictionary_are_skipped_and_nothing_out_of_range_is_read(emu_asan, build_dir):
    """One entry below 0 and one at or above H, in a list that spans two candidate tiles: both are skipped, the result is the
    top-k of the entries inside, and the sanitizer saw no access outside an operand."""
    B, D, H, k = 5, 36, 160, 7
    x, W, bias = U.gaussian(1, B, D), U.gaussian(2, H, D), U.gaussian(3, 1, H)[0]
    units = np.concatenate([[-3], U.pick_units(4, H, 130, (0, H - 1)), [H + 5]]).astype(np.int32)
    got = _run_topk(emu_asan, build_dir, x, W, bias, units, k)
    _same(got, U.subset_topk(x, W, bias, units, k))
    assert got[0].min() >= 0 and got[0].max() < H


def test_fewer_entries_inside_than_k_leaves_minus_one_and_zero(emu_asan, build_dir):
    x, W, bias = U.gaussian(5, 3, 4), U.gaussian(6, 8, 4), U.gaussian(7, 1, 8)[0]
    units = np.array([-1, 2, 5, 8], dtype=np.int32)
    idx, val = _run_topk(emu_asan, build_dir, x, W, bias, units, 3)
    _same((idx, val), U.subset_topk(x, W, bias, units, 3))
    assert (idx[:, 2] == -1).all() and (val[:, 2].view(np.uint32) == 0).all()


LOSS_CASES = {"one_element_zero_denominator": (1, 1, 0), "3x5_off_alignment": (3, 5, 1), "257x36": (257, 36, 0), "2x300_two_column_blocks": (2, 300, 0)}


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_loss_source_on_the_host_equals_the_restatement(emu, build_dir, name):
    B, D, off = LOSS_CASES[name]
    d = build_dir
    x, recon, aux = U.gaussian(11, B, D), U.gaussian(12, B, D), U.gaussian(13, B, D)
    for a, f in ((x, "lx.bin"), (recon, "lr.bin"), (aux, "la.bin")):
        a.tofile(d / f)
    coef = 1 / 32
    run_emu(emu, ["loss", "lx.bin", "lr.bin", "la.bin", B, D, repr(coef), off, "loss.bin", "grad.bin", "sums.bin"], d, 900)
    loss, grad, sums = U.auxk_loss(x, recon, aux, coef)
    assert np.array_equal(np.fromfile(d / "sums.bin", np.float64), sums)
    assert np.fromfile(d / "loss.bin", np.uint32)[0] == np.float32(loss).view(np.uint32)
    assert np.array_equal(np.fromfile(d / "grad.bin", np.uint32), grad.view(np.uint32).reshape(-1))
    if name == "one_element_zero_denominator":
        assert sums[1] == 0.0 and loss == 0.0 and not grad.any()
