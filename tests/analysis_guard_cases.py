"""The case table of tests/test_analysis_guards_gpu.py: one builder per C-ABI entry point of the ten kernel files that are
otherwise driven on the GPU only through quantizedsae_amd.ops -- analysis.hip, coactivation_bits.hip,
coactivation_partners.hip, token_lists.hip, token_overlap.hip, dictionary.hip, evaluation.hip, optim.hip, trainer.hip and
watch.hip (the ``*_workspace_bytes`` sizers are used, not tabled).  A builder takes a shape name and returns the valid calls
(guard_util.Call) that cover the entry point at that shape: its nullable operands and every kernel form the entry chooses
between.  Roles follow the comments in include/qsae.h.

Shapes:
* ``minimal``: the smallest valid call -- one row, one word, one unit, k = 1, V = 1, n = 1, one tensor of one element.
* ``tails``: one step past each tile, chunk or lane round the kernel uses; the figures stand with each builder and are derived
  from the constants in the sources.

Expected values come from the CPU: the restatements of tests/*_util.py and the oracle give ``Call.expect`` (bit equality) or,
where a restatement is not bitwise (the expf of the quantization error, the MFMA chain of the cosines), ``Call.verify`` with
the bound the project's own GPU test of that entry uses.  The bits of ``ops.*`` on plain tensors are compared as well
(``Call.front``).  Every builder asserts its input conditions on the CPU before anything is launched: accumulated outputs
start from a fixed non-zero state, the expected change is non-zero in the last row / word / unit / chunk / tile, pad columns of
strided outputs hold 0x5A before and after.

A strided output (ld > width) is tabled as an ``inout`` buffer of the full [rows, ld] extent whose pad columns hold 0x5A: the
expected tensor holds the same bytes there, so a store into a pad column fails the comparison.

Importing this module touches no GPU: the builders do.
"""
from __future__ import annotations

import numpy as np
import torch

import oracle
from quantizedsae_amd import ops, synthetic as S

import coactivation_partners_util as P
import dictionary_util as DU
import evaluation_util as EV
import optim_util as OU
import token_lists_util as TL
import token_overlap_util as TO
import trainer_util as TU
import watch_util as WU
from guard_util import POISON, STREAM, WS, WS_BYTES, Buf, Call, HostArray, HostPointers

DEV = "cuda:0"
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
SHAPES = ("minimal", "tails")
POISON32 = np.uint32(0x5A5A5A5A)


# ---- helpers --------------------------------------------------------------------------------------------------------------
def cpu(a) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a)


def dev(a) -> torch.Tensor:
    return cpu(a).to(DEV)


def In(name, a, **kw):
    return Buf(name, "in", data=a if isinstance(a, torch.Tensor) else dev(a), **kw)


def InOut(name, a, **kw):
    return Buf(name, "inout", data=a if isinstance(a, torch.Tensor) else dev(a), **kw)


def Out(name, shape, dtype=F32, **kw):
    return Buf(name, "out", shape=tuple(shape), dtype=dtype, **kw)


def Carried(name, source):
    return Buf(name, "in", carried=source)


def strided(a: np.ndarray, ld: int) -> np.ndarray:
    """[rows, ld] of 0x5A bytes with ``a`` [rows, width] in its first columns (width == ld: a copy of ``a``)"""
    a = np.ascontiguousarray(a)
    assert a.ndim == 2 and ld >= a.shape[1]
    full = np.full((a.shape[0], ld), POISON, np.uint8).repeat(a.dtype.itemsize, axis=1).view(a.dtype).copy()
    full[:, :a.shape[1]] = a
    return full


def pads_poisoned(full: np.ndarray, width: int) -> bool:
    return bool((np.ascontiguousarray(full[:, width:]).view(np.uint8) == POISON).all())


def rng_of(*key):
    return np.random.default_rng([20250, *key])


# ---- compact (idx, val) rows of the top-k models --------------------------------------------------------------------------
def compact_case(seed, B, k, H):
    """idx int32 [B, k] in [0, H) with repeats, val fp32 [B, k] > 0, and what must not count planted as far as the shape has
    room: val 0.0, -0.0 and NaN, indices -1 and H, a unit listed twice in one row.  The last entry of the last row is the
    last unit, active."""
    rng = rng_of(seed, B, k, H)
    idx = rng.integers(0, H, (B, k)).astype(np.int32)
    val = rng.uniform(0.1, 2.0, (B, k)).astype(np.float32)
    if k >= 4:
        val[0, 0], val[0, 1], val[0, 2] = 0.0, -0.0, np.nan
    if B >= 2 and k >= 2:
        idx[1, 0], idx[1, 1] = -1, H
    if B >= 3 and k >= 2:
        idx[2, 1] = idx[2, 0]
        val[2, 0], val[2, 1] = 0.5, 0.75
    idx[B - 1, k - 1] = H - 1
    val[B - 1, k - 1] = 1.0
    return idx, val


def compact_active(idx, val, H):
    with np.errstate(invalid="ignore"):
        on = np.ones(idx.shape, bool) if val is None else (val > 0)
    return on & (idx >= 0) & (idx < H)


def multiplicity(idx, val, H):
    """int64 [B, H]: how often a row lists a unit as active (qsae_activation_counts and qsae_coactivation_sparse count an
    entry, not a mask bit)"""
    act = compact_active(idx, val, H)
    M = np.zeros((idx.shape[0], H), np.int64)
    for b in range(idx.shape[0]):
        np.add.at(M[b], idx[b][act[b]], 1)
    return M


COMPACT = {"minimal": dict(B=1, H=1, ks=(1,)), "tails": dict(B=5, H=33, ks=(65, 256))}


def compact_variants(shape, seed):
    """(idx, val or None, B, k, H, label): every k of the shape with val, the first k with val == NULL as well"""
    d = COMPACT[shape]
    out = []
    for i, k in enumerate(d["ks"]):
        idx, val = compact_case(seed + i, d["B"], k, d["H"])
        out.append((idx, val, d["B"], k, d["H"], f"B {d['B']} k {k} H {d['H']} val"))
        if i == 0:
            out.append((idx, None, d["B"], k, d["H"], f"B {d['B']} k {k} H {d['H']} val NULL"))
    return out


# ---- analysis.hip ---------------------------------------------------------------------------------------------------------
def activation_counts(shape):
    """tails: B = 5, H = 33, k = 65 (a second 64-entry stride of the flat loop is B k > 256) and k = 256."""
    calls = []
    for idx, val, B, k, H, label in compact_variants(shape, 2101):
        inc = multiplicity(idx, val, H).sum(0)
        init = rng_of(2101, k).integers(1, 1000, H).astype(np.int64)
        assert inc[H - 1] > 0 and compact_active(idx, val, H)[B - 1].any() and (init > 0).all()

        def front(p, H=H):
            ops.activation_counts(p["idx"], p.get("val"), H, p["counts"])
            return {"counts": p["counts"]}
        calls.append(Call(label, "qsae_activation_counts",
                          [In("idx", idx), In("val", val) if val is not None else None, B, k, H, InOut("counts", init), STREAM],
                          front, expect={"counts": cpu(init + inc)}))
    return calls


def activation_counts_bits(shape):
    """tails: B = 5 (a second group of 4 rows), 33 words, words_ld = 35."""
    B, words, ld = (1, 1, 1) if shape == "minimal" else (5, 33, 35)
    bits = S.fair_bits(2102, (B, 32 * words))
    bits[B - 1, 32 * words - 1] = 1
    zb = strided(P.pack(bits), ld)
    inc = bits.astype(np.int64).sum(0)
    init = rng_of(2102).integers(1, 1000, 32 * words).astype(np.int64)
    assert inc[-1] > 0 and bits[B - 1].any() and (init > 0).all() and pads_poisoned(zb, words)

    def front(p):
        ops.activation_counts_bits(p["zbits"][:, :words], p["counts"])
        return {"counts": p["counts"]}
    return [Call(f"B {B} words {words} words_ld {ld}", "qsae_activation_counts_bits",
                 [In("zbits", zb), ld, B, 32 * words, InOut("counts", init), STREAM], front, expect={"counts": cpu(init + inc)})]


def coactivation_sparse(shape):
    """tails: H = 33 (the last unit alone in a second word of the partner form; here the last row and column), B = 5 (a second
    workgroup of one wave), k = 65 and 256, ld = 36 > H.  Expected: the int64 M^T M of the multiplicity matrix (mask^T mask
    where no unit repeats; a unit listed twice counts twice, include/qsae.h)."""
    calls = []
    for idx, val, B, k, H, label in compact_variants(shape, 2103):
        ld = H if shape == "minimal" else 36
        M = multiplicity(idx, val, H)
        inc = M.T @ M
        init = strided(rng_of(2103, k).integers(1, 1000, (H, H)).astype(np.int32), ld)
        want = init.copy()
        want[:, :H] += inc.astype(np.int32)
        assert inc[H - 1, H - 1] > 0 and inc[H - 1].sum() > 0 and M[B - 1].any() and pads_poisoned(want, H)
        assert int(inc.max()) + 1000 < 2 ** 31

        def front(p, H=H):
            ops.coactivation_sparse(p["idx"], p.get("val"), H, p["coact"])
            return {"coact": p["coact"]}
        calls.append(Call(f"{label} ld {ld}", "qsae_coactivation_sparse",
                          [In("idx", idx), In("val", val) if val is not None else None, B, k, H, InOut("coact", init), ld, STREAM],
                          front, expect={"coact": cpu(want)}))
    return calls


def quantize_bits(shape):
    """tails: B D = 257 (one element past a 256-thread workgroup) as B = 257 rows of D = 1 at ld = 3; n_bits 1 and 8, signed
    and unsigned.  Expected: the oracle."""
    B, D, ld, ns = (1, 1, 1, (1,)) if shape == "minimal" else (257, 1, 3, (1, 8))
    x = S.normal(2104, (B, D), stream=1, std=3.0).astype(np.float32)
    if B > 8:
        x[3, 0], x[4, 0], x[5, 0] = np.nan, np.inf, -np.inf
    xs = strided(x, ld)
    calls = []
    for n in ns:
        sf = 2 ** (n - 1) / (4 + 1e-5)
        for signed in (True, False):
            want = oracle.quantize_bits(x, n, sf, signed=signed)
            assert want.shape == (B, D * n) and (want.size == 1 or (want.any() and not want.all()))
            calls.append(Call(f"B {B} D {D} ld {ld} n_bits {n} signed {signed}", "qsae_quantize_bits",
                              [In("x", xs), ld, B, D, n, float(np.float32(sf)), int(signed), Out("bits", (B, D * n)), STREAM],
                              lambda p, n=n, sf=sf, signed=signed: {"bits": ops.quantize_bits(p["x"][:, :D], n, sf, signed)},
                              expect={"bits": cpu(want)}))
    return calls


# ---- coactivation_bits.hip / coactivation_partners.hip: packed bits ------------------------------------------------------------
def coact_bits_form(B, nbits) -> str:
    """coact_bits_stage (coactivation_bits.hip:116-137): chunks of 256 rows, a triangle of 256-position tiles; below 256 tiles
    the chunks are split over gridDim.y, at least 4 chunks per split, and more than one split means integer atomics."""
    nchunks, ntiles = (B + 255) // 256, (nbits + 255) // 256
    ntri = ntiles * (ntiles + 1) // 2
    splits = 1
    if ntri < 256:
        splits = max(1, min((512 + ntri - 1) // ntri, (nchunks + 3) // 4))
    per = (nchunks + splits - 1) // splits
    return "atomic" if (nchunks + per - 1) // per > 1 else "plain store"


def packed_case(seed, B, nbits, words_ld, mapped: bool):
    """Packed rows of density 2^-s (coactivation_partners_util) and, when ``mapped``, a position -> unit map with pad slots in
    both tiles whose input bits are all set.  The last row holds the first and the last live position, so the last row, the
    last word, the last tile and the mirrored tile's tail all change.
    -> (zbits int32 [B, words_ld] with 0x5A pad words, index int32 [nbits] or None, H, live bits uint8 [B, nbits])"""
    bits = P.make_bits(seed, B, nbits)
    index, H = None, nbits
    if mapped:
        if nbits == 32:
            pad = np.ones(32, bool)
            pad[7] = False                                   # one unit
        else:
            pad = np.zeros(nbits, bool)
            pad[[3, 31, 130, 255, 257, nbits - 2]] = True
        live = np.flatnonzero(~pad)
        H = live.size
        index = np.full(nbits, -1, np.int32)
        index[live] = H - 1 - np.arange(H)                   # a permutation: no two positions share a unit
        bits[:, pad] = 1
    else:
        live = np.arange(nbits)
    bits[B - 1, live[0]] = bits[B - 1, live[-1]] = 1
    zb = strided(P.pack(bits), words_ld)
    livebits = bits.copy()
    if mapped:
        livebits[:, pad] = 0
    assert pads_poisoned(zb, nbits // 32)
    return zb, index, H, livebits


PACKED = {"minimal": [dict(B=1, nbits=32, mapped=True, expect="plain store")],
          "tails": [dict(B=257, nbits=288, mapped=True, expect="plain store"),
                    dict(B=1025, nbits=288, mapped=True, expect="atomic"),
                    dict(B=257, nbits=288, mapped=False, expect="plain store")]}


def coactivation_bits(shape):
    """tails: nbits = 288 (a second 256-position tile of 32: 3 workgroup tiles, one mirrored with a tail), a map with pad slots
    and H = 282 < nbits, B = 257 (a second chunk of one row, plain stores) and B = 1025 (five chunks, two splits: atomics);
    index == NULL with H == nbits; ld > H.  Expected: int64 mask^T mask of the unit mask."""
    calls = []
    for i, c in enumerate(PACKED[shape]):
        B, nbits = c["B"], c["nbits"]
        words = nbits // 32
        words_ld = words + (0 if shape == "minimal" else 2)
        zb, index, H, _ = packed_case(2110 + i, B, nbits, words_ld, c["mapped"])
        ld = H if shape == "minimal" else H + 3
        bits = np.unpackbits(np.ascontiguousarray(zb[:, :words]).view(np.uint8), axis=1, bitorder="little")
        mask = P.unit_mask(bits, index, H).astype(np.int64)
        inc = mask.T @ mask
        init = strided(rng_of(2110, i).integers(1, 1000, (H, H)).astype(np.int32), ld)
        want = init.copy()
        want[:, :H] += inc.astype(np.int32)
        u_first, u_last = (H - 1, 0) if c["mapped"] else (0, H - 1)   # units of the first / last live position
        assert inc[u_last, u_last] > 0 and inc[u_first, u_last] > 0 and inc[u_last, u_first] > 0 and inc[H - 1].sum() > 0
        assert mask[B - 1].any() and pads_poisoned(want, H) and (shape == "minimal" or ld > H)
        if H > 1:
            P.check_density(inc > 0)

        def front(p, H=H, words=words):
            ops.coactivation_bits(p["zbits"][:, :words], H, p.get("index"), p["coact"])
            return {"coact": p["coact"]}
        calls.append(Call(f"B {B} nbits {nbits} words_ld {words_ld} index {c['mapped']} H {H} ld {ld}", "qsae_coactivation_bits",
                          [In("zbits", zb), words_ld, B, nbits, In("index", index) if index is not None else None, H,
                           InOut("coact", init), ld, WS, WS_BYTES, STREAM], front,
                          sizer=("qsae_coactivation_bits_workspace_bytes", (B, nbits)), expect={"coact": cpu(want)},
                          form=(c["expect"], coact_bits_form(B, nbits))))
    return calls


def _partners_bits_call(i, c, shape, ld_words=None):
    """-> (Call, expected state uint32 [nbits, ld_words], index, H)"""
    B, nbits = c["B"], c["nbits"]
    words = nbits // 32
    words_ld = words + (0 if shape == "minimal" else 2)
    if ld_words is None:
        ld_words = words if shape == "minimal" else 12
    zb, index, H, livebits = packed_case(2120 + i, B, nbits, words_ld, c["mapped"])
    dense = P.expected_dense(livebits.astype(bool))                            # packed-position space, pad slots masked
    inc = np.packbits(dense, axis=1, bitorder="little").view(np.uint32)
    init = strided(rng_of(2120, i).integers(0, 2 ** 32, (nbits, words), dtype=np.uint64).astype(np.uint32)
                   & rng_of(2121, i).integers(0, 2 ** 32, (nbits, words), dtype=np.uint64).astype(np.uint32), ld_words)
    live = np.flatnonzero(index >= 0) if index is not None else np.arange(nbits)
    init[live[0], words - 1] = 0                               # so that the bits of the last row's pair are new
    init[live[-1], :words] = 0
    want = init.copy()
    want[:, :words] |= inc
    new = inc & ~init[:, :words]
    assert init[:, :words].any() and new[live[-1]].any() and new[live[0], words - 1] != 0 and new[:, words - 1].any()
    assert livebits[B - 1].any() and pads_poisoned(want, words)
    if nbits > 32:
        P.check_density(dense[np.ix_(live, live)])

    def front(p, words=words):
        ops.coactivation_partners_bits(p["zbits"][:, :words], p.get("index"), p["partners"])
        return {"partners": p["partners"]}
    call = Call(f"B {B} nbits {nbits} words_ld {words_ld} index {c['mapped']} ld_words {ld_words}", "qsae_coactivation_partners_bits",
                [In("zbits", zb), words_ld, B, nbits, In("index", index) if index is not None else None, InOut("partners", init),
                 ld_words, WS, WS_BYTES, STREAM], front, sizer=("qsae_coactivation_bits_workspace_bytes", (B, nbits)),
                expect={"partners": cpu(want)}, form=(c["expect"], coact_bits_form(B, nbits)))
    return call, want, index, H


def coactivation_partners_bits(shape):
    """The shapes of coactivation_bits; partners uint32 [nbits][ld_words] with ld_words = 12 > nbits / 32 = 9, OR-ed into a
    random prior state.  Expected: coactivation_partners_util.expected_dense of the live bits, packed."""
    return [_partners_bits_call(i, c, shape)[0] for i, c in enumerate(PACKED[shape])]


def coactivation_partners_sparse(shape):
    """tails: H = 33 (P = 64: the last unit alone in a second word), k = 65 (a second 64-lane round of one entry) and 256 (the
    largest accepted), B = 5, ld_words = 3 > 2; val with zeros, -0.0 and a NaN, a repeated unit, indices -1 and H; val NULL."""
    calls = []
    for idx, val, B, k, H, label in compact_variants(shape, 2130):
        Pn = (H + 31) // 32 * 32
        words = Pn // 32
        ld_words = words if shape == "minimal" else words + 1
        mask = multiplicity(idx, val, H) > 0
        dense = np.zeros((Pn, Pn), bool)
        dense[:H, :H] = P.expected_dense(mask)
        inc = np.packbits(dense, axis=1, bitorder="little").view(np.uint32)
        init = np.zeros((Pn, words), np.uint32)
        init[:H] = rng_of(2130, k).integers(0, 2 ** 32, (H, words), dtype=np.uint64).astype(np.uint32)
        init[:H, words - 1] &= np.uint32((1 << (H - 32 * (words - 1))) - 1 if H % 32 else 0xFFFFFFFF)   # no bit at a column >= H
        init[::2] = 0                                          # every other row empty, so that new bits are certain
        init[H:] = rng_of(2131, k).integers(0, 2 ** 32, (Pn - H, words), dtype=np.uint64).astype(np.uint32)   # rows past H: never touched
        init = strided(init, ld_words)
        want = init.copy()
        want[:, :words] |= inc
        new = inc & ~init[:, :words]
        assert init.any() and new[H - 1].any() and new[:, words - 1].any() and mask[B - 1].any() and pads_poisoned(want, words)

        def front(p, H=H):
            ops.coactivation_partners_sparse(p["idx"], p.get("val"), H, p["partners"])
            return {"partners": p["partners"]}
        calls.append(Call(f"{label} ld_words {ld_words}", "qsae_coactivation_partners_sparse",
                          [In("idx", idx), In("val", val) if val is not None else None, B, k, H, InOut("partners", init), ld_words,
                           STREAM], front, expect={"partners": cpu(want)}))
    return calls


def partner_counts_form(ld_words) -> str:
    """qsae_coactivation_partner_counts (coactivation_partners.hip:195): 16-byte loads when the rows are 16-byte aligned"""
    return "16-byte loads" if ld_words % 4 == 0 else "word loads"


def coactivation_partner_counts(shape):
    """On the state that qsae_coactivation_partners_bits left in the same arena.  tails: P = 288 (9 words) at ld_words = 12 (two
    16-byte vectors and one word behind them) and at ld_words = 9 (word loads); with the map, without it, and P > H without it
    (rows p < H only).  Expected: coactivation_partners_util.expected_counts of the expected state."""
    if shape == "minimal":
        variants = [(0, PACKED[shape][0], None, True, None, "word loads")]
    else:
        variants = [(0, PACKED[shape][0], 12, True, None, "16-byte loads"), (2, PACKED[shape][2], 9, False, None, "word loads"),
                    (2, PACKED[shape][2], 12, False, 280, "16-byte loads")]
    calls = []
    for i, c, ld_words, use_index, H_over, expect in variants:
        prep, state, index, H = _partners_bits_call(i, c, shape, ld_words)
        Pn = c["nbits"]
        ld_words = state.shape[1]
        H = H if H_over is None else H_over
        if not use_index:
            index = None
        dense = np.unpackbits(np.ascontiguousarray(state[:, :Pn // 32]).view(np.uint8), axis=1, bitorder="little").astype(bool)
        per_position = P.expected_counts(dense)
        want = np.zeros(H, np.int32)
        if index is None:
            want[:min(Pn, H)] = per_position[:min(Pn, H)]
        else:
            want[index[index >= 0]] = per_position[index >= 0]
        assert shape == "minimal" or (want[H - 1] > 0 and (want > 0).sum() > H // 2)

        def front(p, H=H):
            return {"counts": ops.coactivation_partner_counts(p["partners"], H, p.get("index")).to(I32)}
        calls.append(Call(f"P {Pn} ld_words {ld_words} index {use_index} H {H}", "qsae_coactivation_partner_counts",
                          [Carried("partners", "partners"), Pn, ld_words, In("index", index) if index is not None else None, H,
                           Out("counts", (H,), I32), STREAM], front, expect={"counts": cpu(want)}, prepare=prep,
                          form=(expect, partner_counts_form(ld_words))))
    return calls


def partner_counts_dense_form(ld) -> str:
    """qsae_coactivation_partner_counts_dense (coactivation_partners.hip:209)"""
    return "16-byte loads" if ld % 4 == 0 else "word loads"


def coactivation_partner_counts_dense(shape):
    """tails: H = 33, R = 5 (a second workgroup of one wave); ld = 36 (eight vectors and a tail of one; row0 = 10 puts the
    diagonal inside the slab's columns) and ld = 33 (word loads; row0 = 30: the last two rows have row0 + i >= H).  Pad
    columns hold positive counts that must not be counted."""
    variants = [(1, 1, 1, 0, "word loads")] if shape == "minimal" else [(5, 33, 36, 10, "16-byte loads"), (5, 33, 33, 30, "word loads")]
    calls = []
    for R, H, ld, row0, expect in variants:
        rng = rng_of(2140, ld)
        slab = rng.choice(np.array([-1, 0, 0, 1, 5], np.int32), (R, ld))
        slab[:, H:] = 7
        for i in range(R):
            if row0 + i < H:
                slab[i, row0 + i] = 3 if i % 2 == 0 else 0
        slab[R - 1, H - 1] = 2
        pos = slab[:, :H] > 0
        diag = np.array([row0 + i < H and slab[i, row0 + i] > 0 for i in range(R)])
        want = (pos.sum(1) - diag).astype(np.int32)
        assert diag[0] and (H == 1 or (want[R - 1] > 0 and not diag.all()))

        def front(p, H=H, row0=row0):
            return {"counts": ops.coactivation_partner_counts_dense(p["coact"][:, :H], row0).to(I32)}
        calls.append(Call(f"R {R} H {H} ld {ld} row0 {row0}", "qsae_coactivation_partner_counts_dense",
                          [In("coact", slab), ld, R, H, row0, Out("counts", (R,), I32), STREAM], front, expect={"counts": cpu(want)},
                          form=(expect, partner_counts_dense_form(ld))))
    return calls


# ---- token_lists.hip ------------------------------------------------------------------------------------------------------
def _lists_compact(shape, with_val=True):
    B, k, H = (1, 1, 1) if shape == "minimal" else (2049, 3, 33)
    idx, val = compact_case(2150, B, k, H)
    if not with_val:
        val = None
    mask = multiplicity(idx, val, H) > 0
    tok = TL.row_tokens(B)
    offsets, tokens = TL.restate(mask, tok)
    assert mask[B - 1, H - 1] and offsets[H] > offsets[H - 1]
    return dict(B=B, k=k, H=H, idx=idx, val=val, mask=mask, tok=tok, offsets=offsets, tokens=tokens)


def _count_call(c):
    B, k, H = c["B"], c["k"], c["H"]
    return Call(f"B {B} k {k} H {H} val {c['val'] is not None}", "qsae_token_lists_count",
                [In("idx", c["idx"]), In("val", c["val"]) if c["val"] is not None else None, B, k, H, Out("offsets", (H + 1,), I64), WS,
                 WS_BYTES, STREAM], lambda p: {"offsets": ops.token_lists_count(p["idx"], p.get("val"), H)[0]},
                sizer=("qsae_token_lists_workspace_bytes", (B, H)), expect={"offsets": cpu(c["offsets"])})


def token_lists_count(shape):
    """tails: B = 2049 (W = 66 bitmap words per unit: a second round of 64 holding two), k = 3, H = 33; with val and val NULL.
    The workspace is garbage of exactly qsae_token_lists_workspace_bytes(B, H) bytes: the entry clears its own bitmap."""
    return [_count_call(_lists_compact(shape, with_val)) for with_val in (True, False)]


def count_bits_form(index, nbits, H) -> str:
    """qsae_token_lists_count_bits (token_lists.hip:224): the bitmap is cleared unless the transpose writes every word of it"""
    return "memset" if index is not None or nbits < H else "no memset"


def _lists_bits(shape, variant, B=None):
    """variant: "identity" (H == nbits, index NULL: the form without the memset), "mapped" (a permutation with pad slots whose
    bits are set), "fewer" (nbits < H, index NULL)"""
    if shape == "minimal":
        B, nbits = 1, 32
    elif B is None:
        B, nbits = 65, 2080                                   # a second 64-row block of one row, a second 64-word group of one word
    else:
        nbits = 64
    words = nbits // 32
    words_ld = words + (0 if shape == "minimal" else 2)
    bits = P.make_bits(2160 + len(variant), B, nbits)
    index, H = None, nbits
    if variant == "mapped":
        pad = np.zeros(nbits, bool)
        pad[1::2] = True
        if nbits == 64:                                       # 33 units in 64 positions
            pad[:] = True
            pad[np.r_[0:64:2, 63]] = False
        live = np.flatnonzero(~pad)
        H = live.size
        index = np.full(nbits, -1, np.int32)
        index[live] = (np.arange(H) * 7 + 3) % H if H % 7 else np.arange(H)[::-1]
        assert sorted(index[live].tolist()) == list(range(H))
        bits[:, pad] = 1
    elif variant == "fewer":
        H = nbits + 20
        live = np.arange(nbits)
    else:
        live = np.arange(nbits)
    bits[B - 1, live[-1]] = bits[0, live[0]] = 1
    mask = P.unit_mask(bits, index, H)
    if mask.shape[1] < H:                                     # fewer positions than units: the units past nbits never fire
        mask = np.concatenate([mask, np.zeros((B, H - mask.shape[1]), bool)], axis=1)
    tok = TL.row_tokens(B)
    offsets, tokens = TL.restate(mask, tok)
    zb = strided(TL.pack(bits), words_ld)
    assert mask[B - 1].any() and mask[:, (index[live[-1]] if index is not None else live[-1])].any() and pads_poisoned(zb, words)
    return dict(B=B, nbits=nbits, words=words, words_ld=words_ld, index=index, H=H, zb=zb, mask=mask, tok=tok, offsets=offsets,
                tokens=tokens)


def _count_bits_call(c, expect):
    B, nbits, H, words, index = c["B"], c["nbits"], c["H"], c["words"], c["index"]
    return Call(f"B {B} nbits {nbits} words_ld {c['words_ld']} index {index is not None} H {H}", "qsae_token_lists_count_bits",
                [In("zbits", c["zb"]), c["words_ld"], B, nbits, In("index", index) if index is not None else None, H,
                 Out("offsets", (H + 1,), I64), WS, WS_BYTES, STREAM],
                lambda p: {"offsets": ops.token_lists_count_bits(p["zbits"][:, :words], H, p.get("index"))[0]},
                sizer=("qsae_token_lists_workspace_bytes", (B, H)), expect={"offsets": cpu(c["offsets"])},
                form=(expect, count_bits_form(index, nbits, H)))


def token_lists_count_bits(shape):
    """tails: B = 65, nbits = 2080, words_ld = 67: once with H = 2080 and index NULL (no memset: the poisoned workspace shows a
    bitmap word the transpose leaves out), once mapped with pad slots whose bits are set, once with nbits < H."""
    return [_count_bits_call(_lists_bits(shape, v), e) for v, e in (("identity", "no memset"), ("mapped", "memset"), ("fewer", "memset"))]


def token_lists_fill(shape):
    """On what a count call left in a poisoned workspace of exactly qsae_token_lists_workspace_bytes(B, H) bytes (the alignment
    gaps hold 0x5A there), in the same arena, and on the offsets it wrote.  tails: B = 2049 (W = 66), H = 33, after the compact
    count and after the bits count (64 positions mapped to 33 units), and after the bits count without the memset (B = 65)."""
    preps = [(_lists_compact(shape), None)]
    if shape == "tails":
        preps += [(_lists_bits(shape, "mapped", B=2049), "memset"), (_lists_bits(shape, "identity"), "no memset")]
    else:
        preps += [(_lists_bits(shape, "identity"), "no memset")]
    calls = []
    for c, expect in preps:
        prep = _count_call(c) if expect is None else _count_bits_call(c, expect)
        B, H, n = c["B"], c["H"], int(c["offsets"][-1])
        assert n == c["tokens"].size and n > 0 and c["mask"][B - 1].any()
        calls.append(Call(f"after {prep.entry} [{prep.label}], {n} entries", "qsae_token_lists_fill",
                          [WS, WS_BYTES, Carried("offsets", "offsets"), In("row_tokens", c["tok"]), B, H, Out("tokens", (n,), I32), n,
                           STREAM], lambda p, n=n: {"tokens": ops.token_lists_fill(p[WS], p["offsets"], p["row_tokens"], n)},
                          expect={"tokens": cpu(c["tokens"])}, prepare=prep))
    return calls


def token_lists_regroup(shape):
    """tails: H = 33, nb = 3 with an empty middle batch, and nb = 1."""
    H = 1 if shape == "minimal" else 33
    layouts = [(1,)] if shape == "minimal" else [(70, 5, 40), (70,)]
    calls = []
    for rows in layouts:
        masks, toks, start = [], [], 0
        for j, B in enumerate(rows):
            m = S.uniform01(2170 + j, B * H, stream=len(rows)).reshape(B, H) < 0.2
            if len(rows) == 3 and j == 1:
                m[:] = False
            m[B - 1, H - 1] = j != 1 or len(rows) != 3
            masks.append(m)
            toks.append(TL.row_tokens(B, start))
            start += B
        per = [TL.restate(m, t) for m, t in zip(masks, toks)]
        bo = np.stack([o for o, _ in per])
        seg = np.concatenate([t for _, t in per])
        offsets, tokens = TL.restate(np.concatenate(masks), np.concatenate(toks))
        n = seg.size
        assert n == offsets[H] > offsets[H - 1] and (len(rows) != 3 or bo[1, H] == 0)

        def front(p):
            o, t = ops.token_lists_regroup(p["batch_offsets"], p["segments"])
            return {"offsets": o, "tokens": t}
        calls.append(Call(f"nb {len(rows)} rows {rows} H {H} entries {n}", "qsae_token_lists_regroup",
                          [In("batch_offsets", bo), len(rows), H, In("segments", seg), n, Out("offsets", (H + 1,), I64),
                           Out("tokens", (n,), I32), STREAM], front, expect={"offsets": cpu(offsets), "tokens": cpu(tokens)}))
    return calls


# ---- token_overlap.hip ----------------------------------------------------------------------------------------------------
def _overlap_side(seed, N, V, k, density, stream, ld):
    M, size = TO.random_sets(seed, N, V, k, density, stream)
    if N > 1:
        M[N - 1, V - 1] = 1                                   # the last token in the last feature's set: a bit of the last word
        if M[N - 1].sum() > k:
            M[N - 1, np.flatnonzero(M[N - 1])[0]] = 0
        size = M.sum(axis=1).astype(np.int32)
    else:
        M[:] = 1
        size = M.sum(axis=1).astype(np.int32)
    words = (V + 31) // 32
    packed = TO.pack(M).view(np.uint32).copy()
    if V % 32:
        packed[:, words - 1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)     # the dead bits of the last word, all set
    return M, size, strided(packed, ld)


def token_overlap_hist(shape):
    """tails: Na = 257 (a second 256-feature tile of one), Nb = 33, V = 300 (two 256-token chunks; 12 valid bits in the last
    word, its 20 dead bits set), a_ld = 12 and b_ld = 11 > ceil(V / 32) = 10 with 0x5A pad words, k = 3 and k = 128 (the full LDS
    table); asize == 0 on a feature whose bits are set, and one bsize above k (a contradicting pair, not counted)."""
    variants = [(1, 1, 1, 1, 1, 1)] if shape == "minimal" else [(257, 33, 300, 3, 12, 11), (257, 33, 300, 128, 12, 11)]
    calls = []
    for Na, Nb, V, k, a_ld, b_ld in variants:
        density = 0.02 if k == 3 else 0.6
        Ma, asize, asets = _overlap_side(2180 + k, Na, V, k, density, 10, a_ld)
        Mb, bsize, bsets = _overlap_side(2180 + k, Nb, V, k, density, 20, b_ld)
        if Na > 1:
            asize[np.flatnonzero(asize > 0)[[2, 7]]] = 0       # bits set, no set: they take part in no pair
            bsize[np.flatnonzero(bsize > 0)[1]] = k + 1        # contradicts itself: not counted
        inc = TO.hist_numpy(Ma, asize, Mb, bsize, k)
        live = int((asize > 0).sum()) * int(((bsize > 0) & (bsize <= k)).sum())     # every other size is the popcount of its bits
        init = rng_of(2180, k).integers(1, 1000, (k + 1, 2 * k + 1)).astype(np.int64)
        assert int(inc.sum()) == live > 0 and int((Ma[Na - 1] & Mb[Nb - 1]).sum()) >= 1 and inc[1:].sum() > 0
        assert Na == 1 or live < Na * Nb
        assert pads_poisoned(asets, (V + 31) // 32) and pads_poisoned(bsets, (V + 31) // 32)

        def front(p, V=V, k=k):
            ops.token_overlap_hist(p["asets"], p["asize"], p["bsets"], p["bsize"], V, k, p["hist"])
            return {"hist": p["hist"]}
        calls.append(Call(f"Na {Na} Nb {Nb} V {V} k {k} a_ld {a_ld} b_ld {b_ld}", "qsae_token_overlap_hist",
                          [In("asets", asets), a_ld, In("asize", asize), Na, In("bsets", bsets), b_ld, In("bsize", bsize), Nb, V, k,
                           InOut("hist", init), WS, WS_BYTES, STREAM], front,
                          sizer=("qsae_token_overlap_hist_workspace_bytes", (Na, Nb, V)), expect={"hist": cpu(init + inc)}))
    return calls


# ---- dictionary.hip -------------------------------------------------------------------------------------------------------
def _atoms(seed, H, D, ld, zero_row=None):
    a = S.normal(seed, (H, D), stream=3).astype(np.float32)
    if zero_row is not None:
        a[zero_row] = 0.0
    return a, strided(a, ld)


def inv_norms_restate(a):
    """atom_inv_norms_kernel (dictionary.hip:265-283): lane l of 64 adds the fp64 squares of d = l, l + 64, ... in ascending
    order, the butterfly xor 32 .. 1 joins them (the order of evaluation_util.unit_sums), then fp32(1 / max(sqrt(s), 1e-12))."""
    a64 = a.astype(np.float64)
    n = np.sqrt(EV.unit_sums(a64 * a64))
    return (1.0 / np.maximum(n, 1e-12)).astype(np.float32)


def atom_inv_norms(shape):
    """tails: H = 129 (a 33rd workgroup holding one wave), D = 36, ld = 40, and a zero atom."""
    H, D, ld, z = (1, 1, 1, None) if shape == "minimal" else (129, 36, 40, 17)
    a, full = _atoms(2190, H, D, ld, z)
    want = inv_norms_restate(a)
    assert np.isfinite(want).all() and (z is None or want[z] == np.float32(1e12)) and (H == 1 or want[H - 1] != want[0])
    return [Call(f"H {H} D {D} ld {ld}", "qsae_atom_inv_norms", [In("atoms", full), ld, H, D, Out("inv_norm", (H,)), STREAM],
                 lambda p: {"inv_norm": ops.atom_inv_norms(p["atoms"][:, :D])}, expect={"inv_norm": cpu(want)})]


def cosine_form(D) -> str:
    """qsae_cosine_compare (dictionary.hip:465-467): the asm-staged loader takes whole 32-wide K slices (and operands below
    2^30 elements, which every tabled shape is); anything else the compiler-load form, which clamps the K tail"""
    return "staged loader" if D % 32 == 0 else "compiler loads"


def _key32(c):
    return EV.mono_key32((np.asarray(c, np.float32) + np.float32(0.0)).astype(np.float32))


def _best_keys(c, ok, axis):
    """u64 keys (mono(c) << 32 | ~index) of the best allowed entry along ``axis`` of c; 0 where none is allowed"""
    n = c.shape[axis]
    idx = np.arange(n, dtype=np.uint64)
    idx = idx[None, :] if axis == 1 else idx[:, None]
    keys = (_key32(c) << np.uint64(32)) | (~idx & np.uint64(0xFFFFFFFF))
    return np.where(ok, keys, np.uint64(0)).max(axis=axis)


def cosine_compare(shape):
    """tails: Ha = 129, Hb = 130 (a second 128-row and 128-column tile of one and two), lda = ldb = D + 4; D = 36 (compiler
    loads, a K tail of 4) and D = 64 (staged loader); pair and self mode; three thresholds, bins = 7, out at out_ld = 132 > Hb;
    and every nullable operand NULL.  Every reduction is recomputed exactly from the call's own ``out``; ``out`` itself against
    the fp64 cosines at atol 1e-5 (test_dictionary_gpu.py), the moments within evaluation_util.fp64_sum_bound."""
    thr = (0.0, 0.2, -0.1)
    if shape == "minimal":
        variants = [(1, 1, 4, False, True), (2, 2, 4, True, True)]       # D a multiple of 4; self mode needs a pair i < j
    else:
        variants = [(129, 130, 36, False, True), (129, 130, 64, False, True), (129, 130, 36, True, True), (129, 130, 64, True, True),
                    (129, 130, 36, False, False), (129, 130, 36, True, False)]
    calls = []
    for Ha, Hb, D, self_mode, full in variants:
        lda = D if shape == "minimal" else D + 4
        a, afull = _atoms(2200 + D, Ha, D, lda, 5 if Ha > 5 else None)
        b, bfull = _atoms(2300 + D, Hb, D, lda)
        if self_mode:
            b, Hb_eff = a, Ha
        else:
            Hb_eff = Hb
        out_ld = Hb_eff if shape == "minimal" else 132
        bins = 7 if full else 0
        n_thr = len(thr) if full else 0
        ref = DU.cosine_f64(a, b)
        ii, jj = np.indices((Ha, Hb_eff))
        ok = (ii < jj) if self_mode else np.ones((Ha, Hb_eff), bool)
        tile_written = (ii // 128 <= jj // 128) if self_mode else ok           # self mode: the tiles on and above the diagonal
        assert ok[:, Hb_eff - 1].any() and ok[Ha - 1 - int(self_mode)].any() and np.abs(ref[ok]).max() > (0.05 if Ha > 2 else 0.0)

        def verify(got, Ha=Ha, Hb_eff=Hb_eff, self_mode=self_mode, full=full, ref=ref, ok=ok, tile_written=tile_written,
                   out_ld=out_ld, bins=bins, n_thr=n_thr):
            u64 = lambda t: t.numpy().view(np.uint64)                                   # noqa: E731
            if full:
                o = got["out"].numpy()
                assert pads_poisoned(o, Hb_eff), "out: a pad column changed"
                c = o[:, :Hb_eff]
                assert (c.view(np.uint32)[~tile_written] == POISON32).all(), "out: a tile below the diagonal was written"
                err = np.abs(c[tile_written].astype(np.float64) - ref[tile_written]).max()
                assert err <= 1e-5, f"out: max |c - fp64 cosine| = {err:.3g} > 1e-5"
            else:
                # no matrix to recompute from: the fp32 chain of the kernel differs from the fp64 cosines by at most 1e-5 per
                # entry (the bound above); keys and counts are then checked on the entries that the bound cannot flip
                c = ref.astype(np.float32)
            cs = np.where(ok, c, np.float32(0))
            if full:
                assert np.array_equal(u64(got["row_best"]), _self_row_best(c, ok) if self_mode else _best_keys(c, ok, 1)), "row_best"
                if not self_mode:
                    assert np.array_equal(u64(got["col_best"]), _best_keys(c, ok, 0)), "col_best"
                k = _key32(c[ok])
                assert np.array_equal(u64(got["extrema"]), np.array([k.max(), ~k.min() & np.uint64(0xFFFFFFFF)], np.uint64)), "extrema"
                assert np.array_equal(u64(got["counts"]), np.array([(c[ok] > np.float32(t)).sum() for t in thr], np.uint64)), "counts"
                hs = np.float32(0.5) * np.float32(bins)
                bn = np.clip(np.floor(((c[ok] + np.float32(1.0)).astype(np.float32) * hs).astype(np.float32)), 0, bins - 1).astype(np.int64)
                assert np.array_equal(u64(got["hist"]), np.bincount(bn, minlength=bins).astype(np.uint64)), "hist"
                terms = cs.astype(np.float64)
                bound = [EV.fp64_sum_bound(terms), EV.fp64_sum_bound(terms * terms)]
            else:
                terms = np.where(ok, ref, 0.0)
                n = int(ok.sum())
                bound = [n * 1e-5, n * 2e-5 + n * 1e-10]                                # |c| <= 1: |c^2 - ref^2| <= 2e-5 + 1e-10
                idx = np.array([(~int(v)) & 0xFFFFFFFF for v in u64(got["row_best"])])
                oks = (ok | ok.T) if self_mode else ok
                rows = np.flatnonzero(oks.any(axis=1))
                best = np.where(oks, ref, -np.inf).max(axis=1)
                assert all(oks[r, idx[r]] and ref[r, idx[r]] >= best[r] - 2e-5 for r in rows), "row_best"
            m = got["moments"].numpy()
            want = [terms.sum(), (terms * terms).sum()]
            for j in range(2):
                assert abs(m[j] - want[j]) <= bound[j], f"moments[{j}] = {m[j]!r}, the fp64 sum is {want[j]!r} (bound {bound[j]:.3g})"

        def front(p, self_mode=self_mode, full=full, Hb_eff=Hb_eff, D=D, tile_written=tile_written):
            rb, cb, mom, ext, cnt, hist, mat = ops.cosine_compare(p["A"][:, :D], None if self_mode else p["B"][:, :D],
                                                                  thr if full else (), 7 if full else 0, want_matrix=full)
            out = {"row_best": rb, "moments": mom, "extrema": ext}
            if not self_mode:
                out["col_best"] = cb
            if full:
                out["counts"], out["hist"] = cnt, hist
                o = p["out"]
                # the front end mirrors the upper triangle in self mode; the raw call leaves the tiles below the diagonal alone
                keep = dev(tile_written)
                o[:, :Hb_eff] = torch.where(keep, mat, o[:, :Hb_eff])
                out["out"] = o
            return out
        args = [In("A", afull), lda, Ha, In("B", bfull) if not self_mode else None, lda, Hb, D, int(self_mode),
                HostArray(thr if full else (), "float32"), n_thr, bins, Out("row_best", (Ha,), I64),
                Out("col_best", (Hb,), I64) if not self_mode else None, Out("moments", (2,), F64), Out("extrema", (2,), I64),
                Out("counts", (n_thr,), I64) if full else None, Out("hist", (bins,), I64) if full else None,
                InOut("out", strided(np.zeros((Ha, 0), np.float32), out_ld)) if full else None, out_ld, WS, WS_BYTES, STREAM]
        calls.append(Call(f"Ha {Ha} Hb {Hb} D {D} lda {lda} self {self_mode} thresholds {n_thr} bins {bins} out {full} out_ld {out_ld}",
                          "qsae_cosine_compare", args, front, sizer=("qsae_cosine_compare_workspace_bytes", (Ha, Hb, int(self_mode))),
                          verify=verify, form=("staged loader" if D % 32 == 0 else "compiler loads", cosine_form(D))))
    return calls


def _self_row_best(c, ok):
    """self mode: a pair i < j updates row_best[i] with (c, j) and row_best[j] with (c, i)"""
    sym = np.where(ok, c, np.float32(0)) + np.where(ok, c, np.float32(0)).T
    return _best_keys(sym.astype(np.float32), ok | ok.T, 1)


# ---- evaluation.hip -------------------------------------------------------------------------------------------------------
def quant_error_form(n_bits, offset_bytes) -> str:
    """qsae_quantization_error (evaluation.hip:407): n_bits 4 and 8 read 16-byte vectors when logits is 16-byte aligned"""
    return "16-byte loads" if n_bits in (4, 8) and offset_bytes % 16 == 0 else "scalar loads"


def quantization_error(shape):
    """tails: H = 257 (a second round of the 256 join threads holding one unit), D = 65 (a second 64-lane round of one entry);
    n_bits 4 and 8 (16-byte loads), 3 (scalar), and n_bits 4 with logits 4 bytes off its 16-byte boundary (scalar).  The soft
    side runs through expf, so the CPU restatement is not bitwise: evaluation_util.check_quant holds the hard side, the counts
    and the index to equality and the soft side to the bounds derived in that module, as test_evaluation_gpu.py does."""
    variants = [(1, 1, 1, 0, "scalar loads")] if shape == "minimal" else \
        [(257, 65, 4, 0, "16-byte loads"), (257, 65, 8, 0, "16-byte loads"), (257, 65, 3, 0, "scalar loads"), (257, 65, 4, 4, "scalar loads")]
    calls = []
    for H, D, n, off, expect in variants:
        logits = EV.quant_logits(H, D, n) if H > 1 else np.array([[0.7]], np.float32)
        step = EV.step_of(n)
        assert np.abs(logits[H - 1, -n:]).max() > 0

        def verify(got, logits=logits, D=D, n=n, step=step):
            EV.check_quant(EV.parse_block(got["result"].numpy()), got["unit_err_sq"].numpy(), logits, D, n, step)

        def front(p, D=D, n=n, step=step):
            r, u = ops.quantization_error(p["logits"], D, n, step, EV.MARGIN)
            return {"result": r, "unit_err_sq": u}
        calls.append(Call(f"H {H} D {D} n_bits {n} logits offset {off}", "qsae_quantization_error",
                          [In("logits", logits, offset_bytes=off), H, D, n, float(step), float(np.float32(EV.MARGIN)),
                           Out("result", (48,), F64), Out("unit_err_sq", (H,), F64), WS, WS_BYTES, STREAM], front,
                          sizer=("qsae_quantization_error_workspace_bytes", (H, D, n)), verify=verify,
                          form=(expect, quant_error_form(n, off))))
    return calls


MOMENT_DTYPES = {0: "float32", 1: "float16", 2: "bfloat16"}


def moments_form(D, dtype, x_offset) -> str:
    """qsae_dataset_moments_add (evaluation.hip:458): four columns per thread when D % 4 == 0 and x starts on a boundary of
    four elements (recon is tabled aligned or NULL)"""
    esize = 4 if dtype == 0 else 2
    return "four columns" if D % 4 == 0 and x_offset % (4 * esize) == 0 else "one column"


def dataset_moments_add(shape):
    """tails: B = 33 at group_rows = 16 (two full groups and a last group of one row), D = 68 (aligned), D = 67, and x 4 bytes off
    its boundary; dtype 0, 1 and 2; with and without recon; the middle group holds a NaN.  The state starts non-zero."""
    if shape == "minimal":
        variants = [(1, 1, 1, 0, True, 0, "one column")]
    else:
        variants = [(33, 68, 16, 0, True, 0, "four columns"), (33, 67, 16, 0, True, 0, "one column"), (33, 68, 16, 0, True, 4, "one column"),
                    (33, 68, 16, 1, False, 0, "four columns"), (33, 68, 16, 2, True, 0, "four columns"), (33, 68, 16, 1, True, 4, "one column")]
    calls = []
    for B, D, group_rows, dtype, with_recon, off, expect in variants:
        raw = EV.moment_rows(B, D, MOMENT_DTYPES[dtype], seed=dtype)
        x32 = EV.moments_as_f32(raw).copy()
        if B > 20:
            if dtype == 0:
                raw[20, 3] = np.nan
            elif dtype == 1:
                raw[20, 3] = np.float16(np.nan)
            else:
                raw[20, 3] = 0x7FC0
            x32 = EV.moments_as_f32(raw).copy()
            assert np.isnan(x32[20, 3]) and np.isnan(x32).sum() == 1
        recon = (x32 * np.float32(0.9) + S.normal(2210, (B, D), stream=4, std=0.1)).astype(np.float32) if with_recon else None
        if recon is not None:
            recon = np.nan_to_num(recon)
        rng = rng_of(2210, D, dtype)
        sums0 = rng.standard_normal((3, D))
        counts0 = np.array([7, 3], np.int64)
        sums, kept, skipped = EV.moments_restate(x32, recon, group_rows, state=(sums0, 7, 3))
        G = -(-B // group_rows)
        assert (sums[0] != sums0[0]).all() and kept - 7 == (B if B <= 20 else B - group_rows) and skipped - 3 == (0 if B <= 20 else group_rows)
        assert with_recon == bool((sums[2] != sums0[2]).any()) and (G == 1 or B % group_rows == 1)
        if dtype == 0:
            xt = cpu(raw)
        elif dtype == 1:
            xt = cpu(raw)
        else:
            xt = cpu(raw.view(np.int16)).view(torch.bfloat16)

        def front(p, group_rows=group_rows):
            ops.dataset_moments_add(p["x"], p.get("recon"), group_rows, p["sums"], p["counts"])
            return {"sums": p["sums"], "counts": p["counts"]}
        calls.append(Call(f"B {B} D {D} group_rows {group_rows} dtype {dtype} recon {with_recon} x offset {off}", "qsae_dataset_moments_add",
                          [In("x", xt.to(DEV), offset_bytes=off), dtype, In("recon", recon) if with_recon else None, B, D, group_rows,
                           InOut("sums", sums0), InOut("counts", counts0), WS, WS_BYTES, STREAM], front,
                          sizer=("qsae_dataset_moments_workspace_bytes", (B, D, group_rows, int(with_recon))),
                          expect={"sums": cpu(sums), "counts": cpu(np.array([kept, skipped], np.int64))},
                          form=(expect, moments_form(D, dtype, off))))
    return calls


# ---- optim.hip ------------------------------------------------------------------------------------------------------------
def adam_form(offsets) -> str:
    """qsae_adam_step (optim.hip:157): 16-byte loads when all four pointers are 16-byte aligned"""
    return "16-byte loads" if all(o % 16 == 0 for o in offsets) else "element loads"


def adam_step(shape):
    """tails: n = 4097 (one element past 1024 vectors of four, and past sixteen 256-thread workgroups), aligned and with m 4
    bytes off its boundary.  Expected: optim_util.adam_f32 (no NaN plant: a NaN's payload is not part of the contract)."""
    n = 1 if shape == "minimal" else 4097
    sc = OU.scalars()
    sc32 = [float(np.float32(s)) for s in sc]
    p, g, m, v = OU.adam_case(n, seed=3, plants=OU.PLANTS[:4] if n > 4 else ())
    p2, m2, v2 = OU.adam_f32(p, g, m, v, sc)
    assert p2[n - 1] != p[n - 1] and m2[n - 1] != m[n - 1] and v2[n - 1] != v[n - 1]
    calls = []
    for m_off, expect in ((0, "16-byte loads"),) if shape == "minimal" else ((0, "16-byte loads"), (4, "element loads")):
        def front(t):
            ops.adam_step(t["p"], t["g"], t["m"], t["v"], *sc)
            return {"p": t["p"], "m": t["m"], "v": t["v"]}
        calls.append(Call(f"n {n} m offset {m_off}", "qsae_adam_step",
                          [InOut("p", p), In("g", g), InOut("m", m, offset_bytes=m_off), InOut("v", v), n, *sc32, STREAM], front,
                          expect={"p": cpu(p2), "m": cpu(m2), "v": cpu(v2)}, form=(expect, adam_form((0, 0, m_off, 0)))))
    return calls


def adam_step_prefilter(shape):
    """tails: H = 129 (a 33rd workgroup of one wave), D = 132 (a third 64-lane round of four), with and without the bias
    quadruple.  Expected: optim_util.pref_expected (the Adam restatement followed by the pack_w restatement)."""
    H, D = (1, 1) if shape == "minimal" else (129, 132)
    sc = OU.scalars()
    sc32 = [float(np.float32(s)) for s in sc]
    calls = []
    for variant in ("plain", "nobias"):
        w, b = OU.pref_case(H, D, variant, seed=5)
        if H * D == 1:                                         # no room for the plants: the first one is a zero gradient on zero moments
            w = tuple(a.reshape(1, 1) for a in OU.adam_case(1, seed=6, plants=()))
        (W2, mW2, vW2), b2, Wq, meta = OU.pref_expected(w, b, sc)
        assert (W2[H - 1] != w[0][H - 1]).any() and Wq[H - 1].any() and meta.view(np.uint32).all() == (b is not None)

        def front(t):
            quad = [t.get(nm) for nm in ("bias", "gb", "mb", "vb")]
            Wq_, meta_ = ops.adam_step_prefilter(t["W"], t["gW"], t["mW"], t["vW"], *quad, *sc)
            out = {"W": t["W"], "mW": t["mW"], "vW": t["vW"], "Wq": Wq_, "meta": meta_}
            if quad[0] is not None:
                out.update(bias=t["bias"], mb=t["mb"], vb=t["vb"])
            return out
        expect = {"W": cpu(W2), "mW": cpu(mW2), "vW": cpu(vW2), "Wq": cpu(Wq), "meta": cpu(meta)}
        quad = [None] * 4
        if b is not None:
            quad = [InOut("bias", b[0]), In("gb", b[1]), InOut("mb", b[2]), InOut("vb", b[3])]
            expect.update(bias=cpu(b2[0]), mb=cpu(b2[1]), vb=cpu(b2[2]))
        calls.append(Call(f"H {H} D {D} {variant}", "qsae_adam_step_prefilter",
                          [InOut("W", w[0]), In("gW", w[1]), InOut("mW", w[2]), InOut("vW", w[3]), *quad, H, D, *sc32,
                           Out("Wq", (H, D), torch.float16), Out("meta", (4,)), STREAM], front, expect=expect))
    return calls


# ---- trainer.hip ----------------------------------------------------------------------------------------------------------
def rows_form(D, dtype) -> str:
    """qsae_rows_nan_bitmap / qsae_gather_rows (trainer.hip:271, 301): 16-byte pieces when a row is a whole number of them (the
    tabled pointers are aligned)"""
    return "16-byte pieces" if (D * (4 if dtype == "fp32" else 2)) % 16 == 0 else "elements"


def _chunk(n_rows, D, dtype):
    src = TU.special_chunk(n_rows, D, dtype)
    if n_rows > 1:
        src[n_rows - 1, D - 1] = float("nan")                  # the last element of the last row: bit 0 of the second word
    return src


def _row_variants(shape):
    """(D, dtype): D = 36 and 35 at every dtype as the issue sets them; 36 fp16 / bf16 elements are 72 bytes, not a whole number
    of 16-byte pieces, so D = 40 is added for the 16-bit types to reach their 16-byte form"""
    if shape == "minimal":
        return [(1, "fp32")]
    return [(D, dt) for dt in ("fp32", "fp16", "bf16") for D in (36, 35)] + [(40, "fp16"), (40, "bf16")]


def rows_nan_bitmap(shape):
    """tails: n_rows = 33 (a second word holding one row), D = 36 and 35 (and 40 for the 16-bit types), all three dtypes."""
    n_rows = 1 if shape == "minimal" else 33
    calls = []
    for D, dt in _row_variants(shape):
        src = _chunk(n_rows, D, dt) if n_rows > 1 else torch.full((1, 1), float("nan"))
        want = TU.nan_bitmap_ref(src)
        assert want[-1] == 1 and (n_rows == 1 or 0 < bin(int(want[0])).count("1") < 32)
        calls.append(Call(f"n_rows {n_rows} D {D} {dt}", "qsae_rows_nan_bitmap",
                          [In("src", src.to(DEV)), TU.DTYPE_CODES[dt], n_rows, D, Out("bits", (want.size,), I32), STREAM],
                          lambda p: {"bits": ops.rows_nan_bitmap(p["src"])}, expect={"bits": cpu(want)},
                          form=(rows_form(D, dt), rows_form(D, dt)) if n_rows > 1 else None))
    return calls


def gather_rows(shape):
    """tails: B = 5 (a second workgroup of one wave) out of n_rows = 33, D = 36 and 35 (and 40 for the 16-bit types), all three
    dtypes; the flag word stays 0; and once with one index out of range: a row of zeros and the flag word 1."""
    n_rows, B = (1, 1) if shape == "minimal" else (33, 5)
    variants = [(D, dt, False) for D, dt in _row_variants(shape)]
    if shape == "tails":
        variants += [(36, "fp32", True), (35, "bf16", True)]
    calls = []
    for D, dt, bad in variants:
        src = _chunk(n_rows, D, dt) if n_rows > 1 else torch.tensor([[1.5]])
        idx = np.array([0] if B == 1 else [0, 32, 7, 7, n_rows - 1], np.int64)
        if bad:
            idx[3] = n_rows
        want = TU.gather_ref(src, idx)
        assert want[B - 1].any() and (not bad or not want[3].any()) and want[0].any()

        def front(p):
            out = ops.gather_rows(p["src"], p["idx"], p["flag"])
            return {"out": out, "flag": p["flag"]}
        calls.append(Call(f"n_rows {n_rows} D {D} {dt} B {B} bad index {bad}", "qsae_gather_rows",
                          [In("src", src.to(DEV)), TU.DTYPE_CODES[dt], n_rows, D, In("idx", idx), B, Out("out", (B, D)),
                           InOut("flag", np.zeros(1, np.int32)), STREAM], front,
                          expect={"out": cpu(want), "flag": cpu(np.array([int(bad)], np.int32))},
                          form=(rows_form(D, dt), rows_form(D, dt)) if n_rows > 1 else None))
    return calls


def loss_form(offsets) -> str:
    """qsae_trainer_loss (trainer.hip:343-351): 16-byte loads and stores when all 2 n + 1 pointers are 16-byte aligned"""
    return "16-byte" if all(o % 16 == 0 for o in offsets) else "scalar"


def trainer_loss(shape):
    """tails: B D = 17 * 241 = 4097, one element past the 4096-element block; n = 1 and n = 8, mode 0 and mode 1; aligned, and
    with one reconstruction / one gradient 4 bytes off its boundary."""
    if shape == "minimal":
        variants = [(1, 1, 1, 0, None)]
    else:
        variants = [(17, 241, 8, 0, None), (17, 241, 8, 1, None), (17, 241, 1, 0, "r0"), (17, 241, 1, 1, None), (17, 241, 8, 1, "g3")]
    coef = 2.5
    calls = []
    for B, D, n, mode, off in variants:
        x, recons = TU.loss_case(B, D, n)
        losses, grads = TU.loss_ref(x, recons, mode, coef)
        assert all(g.reshape(-1)[-1] != 0 for g in grads) and (losses > 0).all()
        r_off = [4 if off == f"r{i}" else 0 for i in range(n)]
        g_off = [4 if off == f"g{i}" else 0 for i in range(n)]

        def front(p, n=n, mode=mode):
            ls, gs = ops.trainer_loss(p["x"], [p[f"r{i}"] for i in range(n)], mode, coef)
            return {"losses": ls, **{f"g{i}": gs[i] for i in range(n)}}
        expect = {"losses": cpu(losses), **{f"g{i}": cpu(g) for i, g in enumerate(grads)}}
        calls.append(Call(f"B {B} D {D} n {n} mode {mode} off {off}", "qsae_trainer_loss",
                          [In("x", x), HostPointers([In(f"r{i}", r, offset_bytes=r_off[i]) for i, r in enumerate(recons)]), n, B, D, mode,
                           coef, HostPointers([Out(f"g{i}", (B, D), offset_bytes=g_off[i]) for i in range(n)]), Out("losses", (n,)), WS,
                           WS_BYTES, STREAM], front, sizer=("qsae_trainer_loss_workspace_bytes", (n, B, D)), expect=expect,
                          form=("scalar" if off else "16-byte", loss_form([0] + r_off + g_off))))
    return calls


# ---- watch.hip ------------------------------------------------------------------------------------------------------------
def tensor_stats(shape):
    """tails: T = 33 (a second launch of the 32-tensor table holding one tensor); sizes 0, 1, 8191, 8192 and 8193 (around the
    8192-element chunk); the 8193-element tensor 4 bytes off its boundary; one tensor of equal values, one with non-finite
    entries; bins 1, 64 and 256.  The sizer takes the host array of counts."""
    rng = rng_of(2230)
    if shape == "minimal":
        tensors, offs, all_bins = [np.array([1.5], np.float32)], [0], (1,)
    else:
        sizes = [0, 1, 8191, 8192, 8193] + [3 + 11 * i for i in range(27)] + [257]
        tensors = [(rng.standard_normal(s) * (1 + i % 5) + (i % 3)).astype(np.float32) for i, s in enumerate(sizes)]
        tensors[5] = np.full(300, 0.375, np.float32)
        tensors[6][::7] = np.nan
        tensors[6][3] = np.inf
        tensors[7][:] = 0.0
        tensors[7][::2] = -0.0
        offs = [4 if s == 8193 else 0 for s in sizes]
        all_bins = (1, 64, 256)
    T = len(tensors)
    counts = [int(t.size) for t in tensors]
    calls = []
    for bins in all_bins:
        want = WU.restate_block(tensors, bins)
        last = WU.block_counts(want)[T - 1]
        assert last.sum() == np.isfinite(tensors[T - 1]).sum() > 0 and (bins == 1 or last[-1] > 0)

        def front(p, bins=bins):
            ts = [p[f"t{i}"] if counts[i] else torch.zeros(0, device=DEV) for i in range(T)]
            return {"result": ops.tensor_stats(ts, bins)}
        ptrs = HostPointers([In(f"t{i}", t, offset_bytes=offs[i]) if t.size else None for i, t in enumerate(tensors)])
        calls.append(Call(f"T {T} bins {bins}", "qsae_tensor_stats",
                          [ptrs, HostArray(counts, "int64"), T, 0, bins, Out("result", (T, WU.HEAD + bins), I64), WS, WS_BYTES, STREAM],
                          front, sizer=("qsae_tensor_stats_workspace_bytes", (HostArray(counts, "int64"), T)),
                          expect={"result": cpu(want)}))
    return calls


#: C symbol -> builder(shape name) -> [Call]
CASES = {
    "qsae_activation_counts": activation_counts,
    "qsae_activation_counts_bits": activation_counts_bits,
    "qsae_coactivation_sparse": coactivation_sparse,
    "qsae_quantize_bits": quantize_bits,
    "qsae_coactivation_bits": coactivation_bits,
    "qsae_coactivation_partners_bits": coactivation_partners_bits,
    "qsae_coactivation_partners_sparse": coactivation_partners_sparse,
    "qsae_coactivation_partner_counts": coactivation_partner_counts,
    "qsae_coactivation_partner_counts_dense": coactivation_partner_counts_dense,
    "qsae_token_lists_count": token_lists_count,
    "qsae_token_lists_count_bits": token_lists_count_bits,
    "qsae_token_lists_fill": token_lists_fill,
    "qsae_token_lists_regroup": token_lists_regroup,
    "qsae_token_overlap_hist": token_overlap_hist,
    "qsae_atom_inv_norms": atom_inv_norms,
    "qsae_cosine_compare": cosine_compare,
    "qsae_quantization_error": quantization_error,
    "qsae_dataset_moments_add": dataset_moments_add,
    "qsae_adam_step": adam_step,
    "qsae_adam_step_prefilter": adam_step_prefilter,
    "qsae_rows_nan_bitmap": rows_nan_bitmap,
    "qsae_gather_rows": gather_rows,
    "qsae_trainer_loss": trainer_loss,
    "qsae_tensor_stats": tensor_stats,
}

#: entry -> the forms it chooses between, each of which some tabled call must reach (test_every_kernel_form_is_reached)
FORMS = {
    "qsae_coactivation_bits": {"plain store", "atomic"},
    "qsae_coactivation_partners_bits": {"plain store", "atomic"},
    "qsae_coactivation_partner_counts": {"16-byte loads", "word loads"},
    "qsae_coactivation_partner_counts_dense": {"16-byte loads", "word loads"},
    "qsae_token_lists_count_bits": {"memset", "no memset"},
    "qsae_cosine_compare": {"staged loader", "compiler loads"},
    "qsae_quantization_error": {"16-byte loads", "scalar loads"},
    "qsae_dataset_moments_add": {"four columns", "one column"},
    "qsae_adam_step": {"16-byte loads", "element loads"},
    "qsae_rows_nan_bitmap": {"16-byte pieces", "elements"},
    "qsae_gather_rows": {"16-byte pieces", "elements"},
    "qsae_trainer_loss": {"16-byte", "scalar"},
}

#: the widest row stride in bytes of any tabled buffer: the logits of qsae_quantization_error at D = 65, n_bits = 8 (coact at
#: ld = 291 is 1164 bytes, a trainer row of D = 241 is 964, `out` of the cosines at out_ld = 132 is 528)
WIDEST_ROW_STRIDE_BYTES = 65 * 8 * 4
