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
bits.  tests/train_guard_cases.py tables the training entry points this way; other entry points can be tabled the same way.

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
        self._buffers: List[Tuple[torch.Tensor, int]] = []           # (whole buffer, payload bytes)

    def _place(self, shape, dtype) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((2 * GUARD_BYTES + nbytes,), POISON, dtype=torch.uint8, device=self.device)
        assert buf.data_ptr() % 256 == 0
        self._buffers.append((buf, nbytes))
        return buf[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype).view(shape)

    def tensor(self, shape, dtype, fill=None) -> torch.Tensor:
        """A contiguous [shape] view between two guards; poisoned with 0x5A unless ``fill`` is given."""
        t = self._place(shape, dtype)
        if fill is not None:
            t.fill_(fill)
        return t

    def from_tensor(self, src: torch.Tensor) -> torch.Tensor:
        t = self._place(src.shape, src.dtype)
        t.copy_(src.detach().contiguous())
        return t

    def from_numpy(self, a: np.ndarray) -> torch.Tensor:
        return self.from_tensor(torch.from_numpy(np.ascontiguousarray(a)))

    def intact(self) -> bool:
        """Every guard byte of every buffer still reads 0x5A (compared on the device, one host read)."""
        if not self._buffers:
            return True
        bad = [((b[:GUARD_BYTES] != POISON).any() | (b[GUARD_BYTES + n:] != POISON).any()) for b, n in self._buffers]
        return not bool(torch.stack(bad).any())


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
    ``shape`` / ``dtype``, poisoned."""
    name: str
    role: str
    data: Optional[torch.Tensor] = None
    shape: Optional[tuple] = None
    dtype: Optional[torch.dtype] = None


@dataclass
class HostArray:
    """A host pointer argument (level sizes): a ctypes array the entry point reads before it returns."""
    values: Sequence[int]

    def carg(self):
        self.keep = (C.c_int32 * len(self.values))(*[int(v) for v in self.values])
        return C.cast(self.keep, C.c_void_p)


@dataclass
class Call:
    """One valid call of ``entry``.  ``args``: the C arguments in order -- Python scalars, None (a NULL pointer), a Buf, a
    HostArray, or the tokens WS / WS_BYTES / STREAM.  ``sizer``: (symbol, arguments) of the entry's ``*_workspace_bytes``.
    ``front(t)``: runs the ordinary front end on ``t`` (name -> plain device tensor, fresh copies of the ``in`` / ``inout``
    data) and returns name -> expected tensor for every ``out`` / ``inout`` Buf.  ``form``: (expected, reached) names of the
    kernel form, where the entry chooses between forms."""
    label: str
    entry: str
    args: list
    front: Callable[[Dict[str, torch.Tensor]], Dict[str, torch.Tensor]]
    sizer: Optional[tuple] = None
    form: Optional[tuple] = None
    bufs: List[Buf] = field(init=False)

    def __post_init__(self):
        self.bufs = [a for a in self.args if isinstance(a, Buf)]
        names = [b.name for b in self.bufs]
        assert len(set(names)) == len(names), names
        assert all(b.role in ("in", "out", "inout") for b in self.bufs)


def run_call(call: Call, lib, device, shrink_workspace: int = 0) -> None:
    """Every device buffer of the call in one arena, the workspace sized to the byte and left poisoned; two calls on the same
    workspace; after each: return code 0, guards intact, ``in`` operands unchanged, ``out`` / ``inout`` payloads equal to the
    front end's bits.  ``shrink_workspace``: bytes withheld from the workspace (only to show that the harness bites)."""
    what = f"{call.entry} [{call.label}]"
    if call.form is not None:
        assert call.form[0] == call.form[1], f"{what}: expected the {call.form[0]} form, the shape reaches {call.form[1]}"
    arena = GuardedArena(device)
    placed: Dict[str, torch.Tensor] = {}
    for b in call.bufs:
        placed[b.name] = arena.tensor(b.shape, b.dtype) if b.role == "out" else arena.from_tensor(b.data)
    ws, need = None, 0
    if call.sizer is not None:
        need = int(getattr(lib, call.sizer[0])(*call.sizer[1]))
        assert need > 0, f"{what}: {call.sizer[0]}{tuple(call.sizer[1])} refuses a supported shape"
        ws = arena.tensor((need - shrink_workspace,), torch.uint8)

    plain = {b.name: b.data.detach().clone() for b in call.bufs if b.role != "out"}
    want = call.front(plain)
    written = [b for b in call.bufs if b.role != "in"]
    assert sorted(want) == sorted(b.name for b in written), f"{what}: the front end gives {sorted(want)}"

    keep, cargs = [], []
    for a in call.args:
        if isinstance(a, Buf):
            cargs.append(C.c_void_p(placed[a.name].data_ptr()))
        elif isinstance(a, HostArray):
            keep.append(a)
            cargs.append(a.carg())
        elif a is WS:
            cargs.append(C.c_void_p(ws.data_ptr()))
        elif a is WS_BYTES:
            cargs.append(need)
        elif a is STREAM:
            cargs.append(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        else:
            cargs.append(a)
    read_only = snapshot([placed[b.name] for b in call.bufs if b.role == "in"])

    fn = getattr(lib, call.entry)
    for run in ("first call", "second call on the same workspace"):
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
            got, exp = placed[b.name], want[b.name]
            assert got.dtype == exp.dtype and tuple(got.shape) == tuple(exp.shape), \
                f"{what}: {b.name} is {got.dtype} {tuple(got.shape)}, the front end gives {exp.dtype} {tuple(exp.shape)}"
            if not same_bits(got, exp):
                diff = int((_bits(got) != _bits(exp)).sum())
                raise AssertionError(f"{what}, {run}: {b.name} differs from the front end's result in {diff} bytes "
                                     f"of {got.numel() * got.element_size()}")
