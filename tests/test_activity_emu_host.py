"""The activity kernels' own source, run on the CPU: csrc/activity.hip is compiled for the host against the stand-in runtime
of tests/emu (threads as lanes, real barriers, the leading-zero count and the integer atomics) and compared with the
numpy restatement of tests/activity_util.py at the shapes the GPU tests use, bit for bit, with guard bytes around every
buffer.  This checks what a GPU-less machine can: indexing, both load widths and the tails, the joins in LDS, the segment
search, the prefix counts that place the dead list.  The source compiles for the host as it stands."""
import numpy as np
import pytest

import activity_util as U
from emu_util import CSRC, compile_emu, run_emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("activity_emu")
    src = (CSRC / "activity.hip").read_text()
    assert src.count('#include "common.h"') == 1
    (d / "activity_emu.hip").write_text(src.replace('#include "common.h"', f'#include "{CSRC / "common.h"}"'))
    exe = compile_emu(d, "activity_emu.cpp", "activity_emu", include=(d,))

    def run(head, arrays):
        head = list(head) + [0] * (8 - len(head))
        (d / "in.bin").write_bytes(np.array(head, np.int64).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
        run_emu(exe, ["in.bin", "out.bin"], d, 600)
        return (d / "out.bin").read_bytes()
    return run


def _state(H, seed):
    fired, _, last = U.state_case(H, seed=seed)
    return fired, last


def _pair(raw, H):
    a = np.frombuffer(raw, np.int64)
    assert a.size == 2 * H
    return a[:H], a[H:]


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("shape", [(1, 1, 1), (257, 65, 1000)], ids=["minimal", "tails"])
def test_compact_source_on_the_host(emu, shape):
    B, k, H = shape
    idx, val = U.compact_case(B, k, H, specials=B > 1)
    fired, last = _state(H, 1)
    for has_val in (1, 0):
        got = _pair(emu([0, B, k, H, 9, has_val], [fired, last, idx, val]), H)
        _same(got, U.add_compact(idx, val if has_val else None, H, 9, fired, last))


def test_bits_source_on_the_host(emu):
    for B, words, ld, H, with_index in ((1, 1, 1, 32, False), (130, 5, 7, 140, True), (1100, 70, 70, 2240, False)):
        z = U.bits_case(B, words, ld, density=0.1 if B > 1000 else 0.3)
        index = U.padded_index(32 * words, H) if with_index else np.zeros(32 * words, np.int32)
        fired, last = _state(H, 2)
        got = _pair(emu([1, B, words, ld, H, 9, int(with_index)], [fired, last, z, index]), H)
        _same(got, U.add_bits(z, 32 * words, index if with_index else None, H, 9, fired, last))


@pytest.mark.parametrize("shape", [(1, 1, 1, 0), (67, 1029, 1040, 0), (67, 1029, 1029, 0), (67, 1029, 1040, 1), (1030, 300, 300, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_dense_source_on_the_host(emu, shape):
    B, H, ld, shift = shape
    x = U.dense_case(B, H, ld, specials=B > 1)
    fired, last = _state(H, 3)
    got = _pair(emu([2, B, H, ld, 9, shift], [fired, last, x]), H)
    _same(got, U.add_dense(x, H, 9, fired, last))
    if B > 1:
        assert got[0][5] == fired[5] and got[1][5] == last[5]


@pytest.mark.parametrize("advance", [0, 1])
@pytest.mark.parametrize("case", [(1, []), (2500, []), (2500, [2500]), (2500, [37, 1203, 1, 1259]), (1024, [0, 1024])],
                         ids=lambda c: f"H{c[0]}_seg{len(c[1])}")
def test_summary_source_on_the_host(emu, case, advance):
    H, sizes = case
    fired, base, last = U.state_case(H, seed=4)
    if H > 17:
        fired[17], base[17] = 2 ** 32 + 5, 0
    for has_base, want_dead in ((1, 1), (0, 1), (1, 0)):
        raw = emu([3, H, 5000, 700, len(sizes), advance, has_base, want_dead], [fired, base, last, np.array(sizes, np.int32)])
        n = (1 + len(sizes)) * U.WORDS
        result = np.frombuffer(raw[:8 * n], np.int64).reshape(-1, U.WORDS)
        new_base = np.frombuffer(raw[8 * n:8 * n + 8 * H], np.int64)
        dead_out = np.frombuffer(raw[8 * n + 8 * H:], np.int32)
        want, want_dead_list = U.summary(fired, base if has_base else None, last, 5000, 700, sizes)
        assert np.array_equal(result, want)
        assert np.array_equal(new_base, fired if (advance and has_base) else base)
        k = want_dead_list.size if want_dead else 0
        assert np.array_equal(dead_out[:k], want_dead_list[:k]) and (dead_out[k:] == U.DEAD_POISON).all()
