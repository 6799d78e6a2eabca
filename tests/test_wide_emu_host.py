"""The slab selection's own source, run on the CPU: csrc/wide.hip is compiled for the host against the stand-in runtime of
tests/emu and compared with the numpy restatement of tests/wide_util.py (one lexsort by key descending, unit ascending), bit for
bit -- once plain and once as a stand-alone AddressSanitizer executable.  Guard bytes surround every buffer and the driver also
checks that read-only operands kept their bytes.  This checks what a GPU-less machine can: the rank formula across 2 to 32
lists with ties on every boundary, signed zeros, infinities and NaN rows; the erase of the dense latent (losers +0, winners
and every other element untouched); and, with host stand-ins for the per-slab selection forms, the plumbing of the two
whole-selection entry points: offset pointers, the shared scratch, the choice of form per slab and the sum of flagged rows."""
import numpy as np
import pytest

import wide_util as U
from emu_util import CSRC, compile_emu, run_emu

S_VALUES, K_VALUES = (2, 3, 5, 32), (1, 63, 64, 65, 256)


class Emu:
    def __init__(self, d, exe):
        self.d, self.exe = d, exe

    def merge(self, pidx, pval, starts, dense=None):
        S, B, k = pidx.shape
        ld = dense.shape[1] if dense is not None else 0
        with open(self.d / "in.bin", "wb") as f:
            f.write(pidx.tobytes() + pval.tobytes() + (dense.tobytes() if dense is not None else b""))
        run_emu(self.exe, ["merge", S, B, k, int(dense is not None), ld, ",".join(map(str, starts)), "in.bin", "out.bin"], self.d)
        raw = (self.d / "out.bin").read_bytes()
        n = B * k
        assert len(raw) == 8 * n + 4 * B * ld
        return (np.frombuffer(raw, np.int32, n).reshape(B, k), np.frombuffer(raw, np.float32, n, 4 * n).reshape(B, k),
                np.frombuffer(raw, np.float32, B * ld, 8 * n).reshape(B, ld) if dense is not None else None)

    def encode(self, x, W, bias, k, slab, with_dense, prefilter, ld):
        B, D = x.shape
        H = W.shape[0]
        wq = np.zeros((H, D), np.uint16)
        wq[:, 0] = W[:, 0].astype(np.uint16)
        with open(self.d / "in.bin", "wb") as f:
            f.write(x.tobytes() + W.tobytes() + bias.tobytes() + (wq.tobytes() if prefilter else b""))
        run_emu(self.exe, ["encode", B, D, H, k, slab, int(with_dense), int(prefilter), ld, "in.bin", "out.bin"], self.d)
        raw = (self.d / "out.bin").read_bytes()
        n, nd = B * k, (B * ld if with_dense else 0)
        assert len(raw) == 8 * n + 4 * nd + 16
        return (np.frombuffer(raw, np.int32, n).reshape(B, k), np.frombuffer(raw, np.float32, n, 4 * n).reshape(B, k),
                np.frombuffer(raw, np.float32, nd, 8 * n).reshape(B, ld) if with_dense else None,
                np.frombuffer(raw, np.int32, 4, 8 * n + 4 * nd))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan"])
def emu(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_emu")
    return Emu(d, compile_emu(d, "wide_emu.cpp", "emu", include=[CSRC], asan=request.param))


def _starts(S, k):
    """slabs of k, k + 1 or k + 2 units: every list nearly exhausts its slab, and no start is a multiple of anything"""
    widths = [k + s % 3 for s in range(S)]
    return [int(h) for h in np.concatenate([[0], np.cumsum(widths)])], widths


def _check_merge(emu, seed, S, B, k, kinds, with_dense=True):
    starts, widths = _starts(S, k)
    pidx, pval = U.part_lists(seed, S, B, k, kinds, widths)
    ld = starts[-1] + 3
    dense = U.dense_before(pidx, pval, starts, ld) if with_dense else None
    idx, val, after = emu.merge(pidx, pval, starts, dense)
    ridx, rval, rafter = U.merge_ref(pidx, pval, starts, dense)
    assert U.same_bits(idx, ridx), (S, B, k, kinds)
    assert U.same_bits(val, rval), (S, B, k, kinds)
    if with_dense:
        assert U.same_bits(after, rafter), (S, B, k, kinds)
        # the restatement's own shape: exactly S k - k elements per row became +0, the winners kept their bits
        changed = after.view(np.uint32) != dense.view(np.uint32)
        assert (after.view(np.uint32)[changed] == 0).all() and (changed.sum(axis=1) <= S * k - k).all()
        for r in range(B):
            assert U.same_bits(after[r, idx[r]], val[r])


@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("k", K_VALUES)
def test_merge_of_five_rows_one_of_every_kind(emu, S, k):
    """B = 5: all values equal, duplicates across the boundaries, signed zeros, infinities, a NaN row"""
    _check_merge(emu, 100 * S + k, S, 5, k, U.KINDS)


@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("k", K_VALUES)
def test_merge_of_a_single_row(emu, S, k):
    """B = 1, every kind in turn; the NaN row without a dense latent as well"""
    for i, kind in enumerate(U.KINDS):
        _check_merge(emu, 1000 * S + 10 * k + i, S, 1, k, (kind,))
    _check_merge(emu, 7, S, 1, k, ("nan",), with_dense=False)


def test_hand_made_row_across_two_slabs(emu):
    """NaN first, then +inf, ties to the lower unit, -0 == +0: the restatement's order on a row small enough to read, and the
    kernel's on the same row cut into two slabs of four"""
    vals = np.array([0.0, np.nan, -0.0, np.inf, 1.0, 1.0, -np.inf, 2.0], np.float32)
    units = np.arange(8, dtype=np.int32)
    su, sv = U.sort_lists(units[None], vals[None])
    assert su[0].tolist() == [1, 3, 7, 4, 5, 0, 2, 6]
    assert np.signbit(sv[0, 6]) and not np.signbit(sv[0, 5])
    parts = [U.sort_lists(np.arange(4, dtype=np.int32)[None], vals[None, 4 * s:4 * s + 4]) for s in range(2)]
    pidx = np.stack([p[0] for p in parts]).astype(np.int32)
    pval = np.stack([p[1] for p in parts])
    idx, val, _ = emu.merge(pidx, pval, [0, 4, 8])
    assert idx[0].tolist() == [1, 3, 7, 4] and U.same_bits(val[0], sv[0, :4])


def _encode_ref(x, W, bias, k, H, ld, with_dense):
    z = (x.astype(np.float64) @ W.astype(np.float64).T + bias).astype(np.float32)      # small integers: exact in every order
    units = np.broadcast_to(np.arange(H, dtype=np.int64), z.shape)
    su, sv = U.sort_lists(units, z)
    dense = None
    if with_dense:
        dense = np.frombuffer(b"\x5a" * (4 * x.shape[0] * ld), np.float32).reshape(x.shape[0], ld).copy()
        dense[:, :H] = 0.0
        np.put_along_axis(dense, su[:, :k], sv[:, :k], axis=1)
    return su[:, :k].astype(np.int32), sv[:, :k], dense


@pytest.mark.parametrize("B,H,k,slab,prefilter,forms", [
    (5, 2564, 7, 1024, True, (2, 1, 0)),       # slabs of 1024, 1024, 516: two through the prefilter stand-in, the tail exact
    (5, 2564, 7, 1024, False, (0, 3, 0)),
    (3, 2564, 7, 1024, True, (0, 3, 0)),       # a batch the prefilter stand-in refuses: every slab exact
    (1, 1536, 256, 512, False, (0, 3, 0)),     # k = 256 out of slabs of 512
])
def test_whole_selection_over_stand_in_slab_forms(emu, B, H, k, slab, prefilter, forms):
    """integer operands with many ties, so that the merge sees duplicates across the slab boundaries; dense stride H + 4"""
    assert U.plan(H, k, slab) is not None
    rng = np.random.default_rng(B * H + k)
    D = 4
    x = rng.integers(-2, 3, (B, D)).astype(np.float32)
    W = rng.integers(-2, 3, (H, D)).astype(np.float32)
    W[:, 0] = np.arange(H) % 3                                # >= 0: the stand-in checks the 16-bit copy's offset with it
    bias = rng.integers(-1, 2, H).astype(np.float32)
    for with_dense in (True, False):
        idx, val, dense, words = emu.encode(x, W, bias, k, slab, with_dense, prefilter, H + 4)
        ridx, rval, rdense = _encode_ref(x, W, bias, k, H, H + 4, with_dense)
        assert U.same_bits(idx, ridx) and U.same_bits(val, rval)
        if with_dense:
            assert U.same_bits(dense, rdense)                # zeros, the k survivors, and the four pad columns still 0x5A
        pre, latent, compact = forms
        exact = (latent, 0) if with_dense else (0, latent)
        assert words.tolist() == [pre if prefilter else -1, pre, *exact]
