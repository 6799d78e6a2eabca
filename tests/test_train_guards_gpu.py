"""What the training kernels write OUTSIDE their outputs (csrc/train.hip, csrc/train_gemm.hip, csrc/train_mask.hip): every C-ABI
entry point called straight through ctypes with all of its device buffers -- inputs, outputs, workspace -- between 1 MiB guards
of 0x5A (guard_util.GuardedArena), at the two shapes of train_guard_cases.py.  The workspace is exactly what the entry's
``*_workspace_bytes`` returns and arrives as garbage; the outputs arrive poisoned.  After each of two calls on the same
workspace: return code 0, every guard byte intact, every read-only operand bitwise unchanged, and every output bit for bit
what the ordinary front end (quantizedsae_amd.ops on plain tensors) returns -- the kernels are documented as bitwise
reproducible, so bit equality is the criterion.  test_train_guards_host.py proves the table complete without a GPU."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard_util as GU  # noqa: E402
import train_guard_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("entry", sorted(T.CASES))
def test_entry_point_between_guards(entry, shape):
    from quantizedsae_amd import _lib
    lib = _lib.load()
    calls = T.CASES[entry](shape)
    assert calls and all(c.entry == entry for c in calls)
    for call in calls:
        GU.run_call(call, lib, T.DEV)
    print(f"{entry} {shape}: " + "; ".join(c.label + (f" ({c.form[1]})" if c.form else "") for c in calls))


def test_every_kernel_form_is_reached():
    """The forms an entry point chooses between are each reached by some tabled call (the call asserts the choice from the
    entry's own shape arithmetic; this asserts that the table as a whole leaves none out)."""
    want = {
        "qsae_train_matryoshka_dpre": {"matrix pipe", "constant kernel"},
        "qsae_train_ternary_dpre": {"matrix pipe", "constant kernel"},
        "qsae_train_matryoshka_dsum_dense": {"one launch", "per level"},
        "qsae_train_blatent_dpre": {"whole K slices", "clamped K tail"},
        "qsae_train_table_unit_grad": {"16-byte store", "element store"},
    }
    for entry, forms in want.items():
        reached = {c.form[1] for shape in T.SHAPES for c in T.CASES[entry](shape) if c.form is not None}
        assert reached == forms, (entry, reached)
    # the tails shape alone reaches both forms of the level-wise contraction: the 1000-unit layout sits on 128-unit tiles
    tails = {c.form[1] for c in T.CASES["qsae_train_matryoshka_dsum_dense"]("tails")}
    assert tails == {"one launch", "per level"}
