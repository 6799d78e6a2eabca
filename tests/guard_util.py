"""Guard words around device buffers, and the harness that drives a C-ABI entry point inside them.

A parity test sees what a kernel writes into its outputs.  It does not see a store one element past an output, a kernel that
uses more workspace than its ``*_workspace_bytes`` declares, a kernel that needs its workspace zeroed, or a backward that
alters a tensor autograd saved: those land in the caching allocator's slack or in a neighbouring tensor.  Here every device
buffer of a call lies between two guards of 0x5A bytes and is itself poisoned with 0x5A unless it carries data, so

* a stray store shows in ``GuardedArena.intact()``,
* an output that is not fully written cannot pass for a result (0x5A5A5A5A is 1.5e16 as fp32, 1515870810 as int32),
* a workspace arrives as garbage, sized to the byte,
* ``snapshot`` / ``unchanged`` compare the read-only operands bit for bit.

``run_call`` is the table-driven form: a ``Call`` names an entry point, its arguments in C order, the role of every pointer
(``in`` / ``out`` / ``inout``; the workspace comes from the entry's sizer) and the front-end call that gives the expected
bits.  tests/train_guard_cases.py tables the training entry points this way, tests/analysis_guard_cases.py the analysis and
training-loop entry points.  The second table uses what the first does not need: expected bits from a CPU restatement
(``Call.expect`` / ``Call.verify``) next to the front end's, host arrays of device pointers (``HostPointers``), typed host
arrays, a payload 4 bytes off its 16-byte boundary (``Buf.offset_bytes``; the guards still touch both of its ends), and staged
calls (``Call.prepare``): a first call leaves a buffer -- its workspace included -- that the main call reads in the same arena.

Importing this module touches no GPU (test_train_guards_host.py imports the case table, which imports this).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

POISON = 0x5A
# Larger than the worst stray store of a 128-row tile at the shapes tabled: a row predicate that fails open writes up to 127
# rows past the last one, 127 rows x ld 1060 x 4 B = 538 480 B (0.54 MB).  A multiple of 4096, so that a payload keeps the
# allocator's alignment (the entry points take 16-byte aligned operands).
GUARD_BYTES = 1 << 20
assert GUARD_BYTES > 127 * 1060 * 4 and GUARD_BYTES % 4096 == 0


class GuardedArena:
    """Device tensors that each lie inside a larger uint8 buffer of 0x5A: GUARD_BYTES before and after the payload."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._buffers: List[Tuple[torch.Tensor, int, int]] = []      # (whole buffer, payload start, payload bytes)

    def _place(self, shape, dtype, offset_bytes: int = 0) -> torch.Tensor:
        """``offset_bytes``: the payload starts that many bytes past the (256-byte aligned) end of a full guard; the guard
        before it grows by as much, so guard bytes run right up to both ends of the payload."""
        shape = tuple(int(s) for s in shape)
        esize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * esize
        assert 0 <= offset_bytes < 4096 and offset_bytes % esize == 0, (offset_bytes, dtype)
        start = GUARD_BYTES + offset_bytes
        buf = torch.full((start + nbytes + GUARD_BYTES,), POISON, dtype=torch.uint8, device=self.device)
        assert buf.data_ptr() % 256 == 0
        self._buffers.append((buf, start, nbytes))
        return buf[start:start + nbytes].view(dtype).view(shape)

    def tensor(self, shape, dtype, fill=None, offset_bytes: int = 0) -> torch.Tensor:
        """A contiguous [shape] view between two guards; poisoned with 0x5A unless ``fill`` is given."""
        t = self._place(shape, dtype, offset_bytes)
        if fill is not None:
            t.fill_(fill)
        return t

    def from_tensor(self, src: torch.Tensor, offset_bytes: int = 0) -> torch.Tensor:
        t = self._place(src.shape, src.dtype, offset_bytes)
        t.copy_(src.detach().contiguous())
        return t

    def from_numpy(self, a: np.ndarray) -> torch.Tensor:
        return self.from_tensor(torch.from_numpy(np.ascontiguousarray(a)))

    def intact(self) -> bool:
        """Every guard byte of every buffer still reads 0x5A (compared on the device, one host read)."""
        if not self._buffers:
            return True
        bad = [((b[:s] != POISON).any() | (b[s + n:] != POISON).any()) for b, s, n in self._buffers]
        return not bool(torch.stack(bad).any())

    def guard_bytes(self, index: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
        """(guard before, guard after) of the index-th buffer placed, as uint8 views: for the test that shows the arena bites."""
        b, s, n = self._buffers[index]
        return b[:s], b[s + n:]


def poison_(t: torch.Tensor) -> torch.Tensor:
    t.reshape(-1).view(torch.uint8).fill_(POISON)                  # (a 0-d tensor has no byte view of its own)
    return t


def _bits(t: torch.Tensor) -> torch.Tensor:
    """Integer view of a contiguous tensor: equal bits compare equal, NaNs included."""
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    return t.reshape(-1).view(torch.uint8)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and bool(torch.equal(_bits(a), _bits(b)))


def snapshot(tensors: Sequence[torch.Tensor]):
    """The bits of read-only operands before a call."""
    return [(t, _bits(t).clone()) for t in tensors]


def unchanged(snap) -> bool:
    """... and whether they are the same bits after it."""
    return all(bool(torch.equal(_bits(t), before)) for t, before in snap)


# ---- the table-driven harness -------------------------------------------------------------------------------------------
WS, WS_BYTES, STREAM = "<workspace>", "<workspace bytes>", "<stream>"      # argument tokens


@dataclass
class Buf:
    """A device pointer argument.  role ``in`` / ``inout``: ``data`` (a device tensor) is copied into the arena; ``out``:
    ``shape`` / ``dtype``, poisoned.  ``offset_bytes``: the payload starts that far past a 16-byte boundary (a multiple of the
    element size).  ``carried``: an ``in`` operand that is not copied in but left by the call's ``prepare`` -- the name of one
    of its buffers, or WS for its workspace (then ``data`` stays None)."""
    name: str
    role: str
    data: Optional[torch.Tensor] = None
    shape: Optional[tuple] = None
    dtype: Optional[torch.dtype] = None
    offset_bytes: int = 0
    carried: Optional[str] = None


_CTYPES = {"int32": C.c_int32, "int64": C.c_int64, "float32": C.c_float}


@dataclass
class HostArray:
    """A host pointer argument (level sizes, element counts, thresholds): a ctypes array of ``ctype`` (int32, int64 or
    float32) that the entry point reads before it returns."""
    values: Sequence
    ctype: str = "int32"

    def carg(self):
        conv = float if self.ctype == "float32" else int
        self.keep = (_CTYPES[self.ctype] * max(1, len(self.values)))(*[conv(v) for v in self.values])
        return C.cast(self.keep, C.c_void_p)


@dataclass
class HostPointers:
    """A host array of device pointers to tabled buffers (None: a NULL entry).  The Bufs are placed in the arena like every
    other buffer of the call."""
    bufs: Sequence[Optional[Buf]]

    def carg(self, placed):
        self.keep = (C.c_void_p * max(1, len(self.bufs)))(*[placed[b.name].data_ptr() if b is not None else None
                                                            for b in self.bufs])
        return C.cast(self.keep, C.c_void_p)


@dataclass
class Call:
    """One valid call of ``entry``.  ``args``: the C arguments in order -- Python scalars, None (a NULL pointer), a Buf, a
    HostArray, a HostPointers, or the tokens WS / WS_BYTES / STREAM.  ``sizer``: (symbol, arguments) of the entry's
    ``*_workspace_bytes`` (an argument may be a HostArray).  ``front(t)``: runs the ordinary front end on ``t`` (name -> plain
    device tensor, fresh copies of the ``in`` / ``inout`` data) and returns name -> expected tensor for every ``out`` /
    ``inout`` Buf.  ``form``: (expected, reached) names of the kernel form, where the entry chooses between forms.
    ``expect``: name -> CPU tensor from a restatement, compared bit for bit with the ``out`` / ``inout`` payload of that name.
    ``verify(got)``: further assertions on the payloads (name -> CPU tensor), for what is not bitwise fixed by a restatement.
    ``prepare``: a call that runs first, once, in the same arena; buffers of this call marked ``carried`` are what it left.  A
    call with ``prepare`` and no sizer of its own takes the prepared workspace for WS / WS_BYTES and must leave it unchanged."""
    label: str
    entry: str
    args: list
    front: Callable[[Dict[str, torch.Tensor]], Dict[str, torch.Tensor]]
    sizer: Optional[tuple] = None
    form: Optional[tuple] = None
    expect: Optional[Dict[str, torch.Tensor]] = None
    verify: Optional[Callable[[Dict[str, torch.Tensor]], None]] = None
    prepare: Optional["Call"] = None
    bufs: List[Buf] = field(init=False)

    def __post_init__(self):
        self.bufs = []
        for a in self.args:
            if isinstance(a, Buf):
                self.bufs.append(a)
            elif isinstance(a, HostPointers):
                self.bufs += [b for b in a.bufs if b is not None]
        names = [b.name for b in self.bufs]
        assert len(set(names)) == len(names), names
        assert all(b.role in ("in", "out", "inout") for b in self.bufs)
        assert all(b.carried is None or (b.role == "in" and self.prepare is not None) for b in self.bufs)


def _first_difference(got: torch.Tensor, exp: torch.Tensor) -> str:
    g, e = got.detach().cpu().reshape(-1), exp.detach().cpu().reshape(-1)
    bad = (_bits(g).view(-1, g.element_size()) != _bits(e).view(-1, e.element_size())).any(dim=1).nonzero().reshape(-1)
    i = int(bad[0])
    return f"{bad.numel()} of {g.numel()} elements differ, the first at flat index {i}: {g[i].item()!r} instead of {e[i].item()!r}"


def _execute(call: Call, lib, device, arena: GuardedArena, prepared, shrink_workspace: int, runs):
    """Places the call's buffers in ``arena`` and runs it ``runs`` times; -> (placed, workspace, workspace bytes)."""
    what = f"{call.entry} [{call.label}]"
    if call.form is not None:
        assert call.form[0] == call.form[1], f"{what}: expected the {call.form[0]} form, the shape reaches {call.form[1]}"
    placed: Dict[str, torch.Tensor] = {}
    for b in call.bufs:
        if b.carried is not None:
            placed[b.name] = prepared[0][b.carried] if b.carried is not WS else prepared[1]
        elif b.role == "out":
            placed[b.name] = arena.tensor(b.shape, b.dtype, offset_bytes=b.offset_bytes)
        else:
            placed[b.name] = arena.from_tensor(b.data, offset_bytes=b.offset_bytes)
        assert placed[b.name].data_ptr() % 16 == b.offset_bytes % 16 or b.carried is not None
    ws, need = None, 0
    read_only_ws = False
    if call.sizer is not None:
        sizer_args = [a.carg() if isinstance(a, HostArray) else a for a in call.sizer[1]]
        need = int(getattr(lib, call.sizer[0])(*sizer_args))
        assert need > 0, f"{what}: {call.sizer[0]}{tuple(call.sizer[1])} refuses a supported shape"
        ws = arena.tensor((need - shrink_workspace,), torch.uint8)
    elif prepared is not None and any(a is WS for a in call.args):
        ws, need = prepared[1], prepared[2]
        read_only_ws = True

    plain = {b.name: (placed[b.name] if b.carried is not None else b.data).detach().clone() for b in call.bufs if b.role != "out"}
    if read_only_ws:
        plain[WS] = ws.detach().clone()
    want = call.front(plain)
    written = [b for b in call.bufs if b.role != "in"]
    assert sorted(want) == sorted(b.name for b in written), f"{what}: the front end gives {sorted(want)}"
    if call.expect is not None:
        assert set(call.expect) <= {b.name for b in written}, f"{what}: expect names {sorted(call.expect)}"

    keep, cargs = [], []
    for a in call.args:
        if isinstance(a, Buf):
            cargs.append(C.c_void_p(placed[a.name].data_ptr()))
        elif isinstance(a, HostArray):
            keep.append(a)
            cargs.append(a.carg())
        elif isinstance(a, HostPointers):
            keep.append(a)
            cargs.append(a.carg(placed))
        elif a is WS:
            cargs.append(C.c_void_p(ws.data_ptr()))
        elif a is WS_BYTES:
            cargs.append(need)
        elif a is STREAM:
            cargs.append(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        else:
            cargs.append(a)
    read_only = snapshot([placed[b.name] for b in call.bufs if b.role == "in"] + ([ws] if read_only_ws else []))

    fn = getattr(lib, call.entry)
    for run in runs:
        if run != "first call":
            for b in written:
                if b.role == "inout":
                    placed[b.name].copy_(b.data)
                else:
                    poison_(placed[b.name])
        with torch.cuda.device(torch.device(device)):
            rc = fn(*cargs)
            torch.cuda.synchronize()
        assert rc == 0, f"{what}, {run}: returned {rc}: {lib.qsae_last_error().decode(errors='replace')}"
        assert arena.intact(), f"{what}, {run}: wrote outside its buffers (a guard word changed)"
        assert unchanged(read_only), f"{what}, {run}: altered a read-only operand"
        for b in written:
            got = placed[b.name]
            if call.expect is not None and b.name in call.expect:
                exp = call.expect[b.name]
                assert got.dtype == exp.dtype and tuple(got.shape) == tuple(exp.shape), \
                    f"{what}: {b.name} is {got.dtype} {tuple(got.shape)}, the restatement gives {exp.dtype} {tuple(exp.shape)}"
                if not same_bits(got.cpu(), exp):
                    raise AssertionError(f"{what}, {run}: {b.name} differs from the CPU restatement: {_first_difference(got, exp)}")
            exp = want[b.name]
            assert got.dtype == exp.dtype and tuple(got.shape) == tuple(exp.shape), \
                f"{what}: {b.name} is {got.dtype} {tuple(got.shape)}, the front end gives {exp.dtype} {tuple(exp.shape)}"
            if not same_bits(got, exp):
                diff = int((_bits(got) != _bits(exp)).sum())
                raise AssertionError(f"{what}, {run}: {b.name} differs from the front end's result in {diff} bytes "
                                     f"of {got.numel() * got.element_size()}")
        if call.verify is not None:
            call.verify({b.name: placed[b.name].detach().cpu().clone() for b in written})
    return placed, ws, need


def run_call(call: Call, lib, device, shrink_workspace: int = 0) -> None:
    """Every device buffer of the call in one arena, the workspace sized to the byte and left poisoned; two calls on the same
    workspace; after each: return code 0, guards intact, ``in`` operands unchanged, ``out`` / ``inout`` payloads equal to the
    front end's bits (and to ``call.expect``, and passing ``call.verify``).  A ``prepare`` call runs first, once, under the same
    checks.  ``shrink_workspace``: bytes withheld from the workspace (only to show that the harness bites)."""
    arena = GuardedArena(device)
    prepared = None
    if call.prepare is not None:
        assert call.prepare.prepare is None
        prepared = _execute(call.prepare, lib, device, arena, None, 0, ("first call",))
    _execute(call, lib, device, arena, prepared, shrink_workspace, ("first call", "second call on the same workspace"))
