"""The token-list entry points without a GPU: declared, bound and exported, the workspace formula, every argument check
before any HIP call (the only reason these calls can be made on a machine without a device), and the host-side pieces
of the Python layer."""
import re
from pathlib import Path

import pytest
import torch

from quantizedsae_amd import _lib, build, ops
from quantizedsae_amd.inference import TokenLists, analysis as A, token_lists_to_python  # noqa: F401

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("qsae_token_lists_workspace_bytes", "qsae_token_lists_count", "qsae_token_lists_count_bits",
         "qsae_token_lists_fill", "qsae_token_lists_regroup")


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "qsae.h").read_text()
    exported = build.exported_symbols(_lib.LIB_PATH)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header)
        assert name in _lib.SIGNATURES and name in exported
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "token_lists.hip" in build.SOURCES
    assert lib.qsae_abi_version() == _lib.ABI_VERSION == 4     # an additive change


def _align(n):
    return (n + 255) // 256 * 256


def test_workspace_is_the_documented_formula_and_zero_for_invalid_shapes():
    size = _lib.load().qsae_token_lists_workspace_bytes
    for H in (1, 33, 1024, 32768):
        for B in (0, 1, 63, 64, 65, 2100, 4096, 65536):
            want = _align(H * max(2, 2 * ((B + 63) // 64)) * 4) + _align(H * 4)
            assert size(B, H) == want == ops.token_lists_workspace_bytes(B, H)
    assert size(4096, 32768) < 4096 * 32768 // 4               # one bit per (row, unit), not a byte
    for B, H in ((-1, 32), (4, 0), (4, -3)):
        assert size(B, H) == 0 == ops.token_lists_workspace_bytes(B, H)


P = 0x1000          # dummy non-null pointers: a call that got as far as a launch would not return an argument error


def _count(lib, *, idx=P, val=P, B=8, k=4, H=64, offsets=P, ws=P, ws_bytes=1 << 20):
    return lib.qsae_token_lists_count(idx, val, B, k, H, offsets, ws, ws_bytes, None)


def _count_bits(lib, *, zbits=P, words_ld=2, B=8, nbits=64, index=None, H=64, offsets=P, ws=P, ws_bytes=1 << 20):
    return lib.qsae_token_lists_count_bits(zbits, words_ld, B, nbits, index, H, offsets, ws, ws_bytes, None)


def _fill(lib, *, ws=P, ws_bytes=1 << 20, offsets=P, row_tokens=P, B=8, H=64, tokens=P, n=5):
    return lib.qsae_token_lists_fill(ws, ws_bytes, offsets, row_tokens, B, H, tokens, n, None)


def _regroup(lib, *, bo=P, nb=2, H=64, segments=P, n=5, offsets=P, tokens=P):
    return lib.qsae_token_lists_regroup(bo, nb, H, segments, n, offsets, tokens, None)


@pytest.mark.parametrize("call,bad", [
    (_count, dict(B=-1)), (_count, dict(k=-1)), (_count, dict(H=0)), (_count, dict(idx=None)), (_count, dict(offsets=None)),
    (_count_bits, dict(B=-1)), (_count_bits, dict(nbits=0)), (_count_bits, dict(nbits=48)), (_count_bits, dict(nbits=-32)),
    (_count_bits, dict(words_ld=1)), (_count_bits, dict(H=0)), (_count_bits, dict(H=32)),        # index == NULL, nbits > H
    (_count_bits, dict(zbits=None)), (_count_bits, dict(offsets=None)),
    (_fill, dict(B=-1)), (_fill, dict(H=0)), (_fill, dict(n=-1)), (_fill, dict(offsets=None)), (_fill, dict(row_tokens=None)),
    (_fill, dict(tokens=None)),
    (_regroup, dict(nb=-1)), (_regroup, dict(H=0)), (_regroup, dict(n=-1)), (_regroup, dict(bo=None)),
    (_regroup, dict(segments=None)), (_regroup, dict(tokens=None)), (_regroup, dict(offsets=None)), (_regroup, dict(nb=0)),
])
def test_invalid_arguments_are_refused_before_any_hip_call(call, bad):
    lib = _lib.load()
    assert call(lib, **bad) == _lib.ERR_INVALID_ARG
    assert b"qsae_token_lists" in lib.qsae_last_error()


def test_unsupported_shapes_small_workspaces_and_empty_fills():
    lib = _lib.load()
    assert _count(lib, B=1 << 20, k=1 << 11) == _lib.ERR_UNSUPPORTED                  # B * k = 2^31
    need = lib.qsae_token_lists_workspace_bytes(8, 64)
    for call in (_count, _count_bits, _fill):
        assert call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
        assert call(lib, ws=None) == _lib.ERR_WORKSPACE
    assert _fill(lib, n=0, tokens=None) == _lib.OK                                     # nothing to write: no launch
    assert _fill(lib, B=0, row_tokens=None) == _lib.OK


def test_token_lists_to_python_on_cpu_tensors():
    offsets = torch.tensor([0, 2, 2, 5, 5], dtype=torch.int64)
    tokens = torch.tensor([7, 3, 9, 9, 1], dtype=torch.int32)
    assert token_lists_to_python(offsets, tokens) == [[7, 3], [], [9, 9, 1], []]
    assert token_lists_to_python(torch.tensor([0, 3]), torch.tensor([4, 4, 2], dtype=torch.int32)) == [[4, 4, 2]]   # H = 1
    assert token_lists_to_python(torch.tensor([0, 0]), torch.zeros(0, dtype=torch.int32)) == [[]]


@pytest.mark.parametrize("fn", [A.compute_activation_stats, A.analyze_dataset])
def test_with_tokens_values_are_checked_before_anything_runs(fn):
    ids = torch.zeros((4, 1), dtype=torch.long)
    with pytest.raises(ValueError, match="with_tokens"):
        fn(None, [], token_ids=ids, tokens_per_context=1, with_tokens="lists")
    with pytest.raises(ValueError, match="with_tokens"):
        fn(None, [], token_ids=ids, tokens_per_context=1, with_tokens=1)
    big = ids.clone()
    big[2, 0] = 2 ** 31
    with pytest.raises(ValueError, match="token ids"):
        fn(None, [], token_ids=big, tokens_per_context=1, with_tokens="csr")
    big[2, 0] = -1
    with pytest.raises(ValueError, match="token ids"):
        fn(None, [], token_ids=big, tokens_per_context=1, with_tokens="csr")
