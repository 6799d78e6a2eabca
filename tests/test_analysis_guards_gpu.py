"""What the analysis and training-loop kernels write OUTSIDE their outputs, and whether they depend on what their workspace held
before: every C-ABI entry point of analysis.hip, coactivation_bits.hip, coactivation_partners.hip, token_lists.hip,
token_overlap.hip, dictionary.hip, evaluation.hip, optim.hip, trainer.hip and watch.hip called straight through ctypes with
all of its device buffers -- inputs, outputs, workspace -- between 1 MiB guards of 0x5A (guard_util.GuardedArena), at the two
shapes of analysis_guard_cases.py.  The workspace is exactly what the entry's ``*_workspace_bytes`` returns and arrives as
garbage; the outputs arrive poisoned, accumulated outputs in a fixed non-zero state.  After each of two calls on the same
workspace: return code 0, every guard byte intact, every read-only operand bitwise unchanged, every output equal to the CPU
restatement of the operation (bit for bit, or within the bound the entry's own GPU test uses where the restatement is not
bitwise) and bit for bit what the ordinary front end (quantizedsae_amd.ops on plain tensors) returns.
test_analysis_guards_host.py proves the table complete without a GPU."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import analysis_guard_cases as A  # noqa: E402
import guard_util as GU  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", A.SHAPES)
@pytest.mark.parametrize("entry", sorted(A.CASES))
def test_entry_point_between_guards(entry, shape):
    from quantizedsae_amd import _lib
    lib = _lib.load()
    calls = A.CASES[entry](shape)
    assert calls and all(c.entry == entry for c in calls)
    for call in calls:
        GU.run_call(call, lib, A.DEV)
    print(f"{entry} {shape}: " + "; ".join(c.label + (f" ({c.form[1]})" if c.form else "") for c in calls))


def test_every_kernel_form_is_reached():
    """The forms an entry point chooses between are each reached by some tabled call (the call asserts the choice from the
    entry's own shape arithmetic; this asserts that the table as a whole leaves none out -- and that the tails shape alone
    does, since the minimal shape has no room for most of them)."""
    for entry, forms in A.FORMS.items():
        reached = {c.form[1] for c in A.CASES[entry]("tails") if c.form is not None}
        assert reached == forms, (entry, reached)
        assert all(c.form is None or c.form[1] in forms for c in A.CASES[entry]("minimal")), entry
    # an entry that is not listed chooses between no forms
    for entry in set(A.CASES) - set(A.FORMS):
        assert all(c.form is None for shape in A.SHAPES for c in A.CASES[entry](shape)), entry


def test_the_arena_bites_without_any_kernel():
    """One byte written through torch indexing just outside a payload turns ``intact()`` false: at the last byte of the guard
    before it, at the first byte of the guard behind it, and at the very last guard byte of the buffer; a write inside the
    payload does not.  The same for a payload 4 bytes off its 16-byte boundary."""
    for offset in (0, 4):
        for where in ("before", "after", "end", "inside"):
            arena = GU.GuardedArena(A.DEV)
            arena.tensor((3,), torch.float32)
            t = arena.tensor((5, 7), torch.float32, offset_bytes=offset)
            assert t.data_ptr() % 16 == offset and arena.intact()
            before, after = arena.guard_bytes()
            assert before.numel() == GU.GUARD_BYTES + offset and after.numel() == GU.GUARD_BYTES
            assert before.data_ptr() + before.numel() == t.data_ptr() and after.data_ptr() == t.data_ptr() + t.numel() * 4
            if where == "before":
                before[-1] = 0
            elif where == "after":
                after[0] = 0
            elif where == "end":
                after[-1] = 0x5B
            else:
                t.view(-1)[-1] = 1.0
            assert arena.intact() == (where == "inside"), (offset, where)
