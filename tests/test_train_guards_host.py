"""Completeness of the guard table (tests/train_guard_cases.py) against the C ABI, without a GPU: every entry point that
csrc/train.hip, csrc/train_gemm.hip and csrc/train_mask.hip define has a case, and a training entry point added later cannot
go without one."""
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

TRAIN_SOURCES = ("train.hip", "train_gemm.hip", "train_mask.hip")
ENTRY_POINTS = [
    # train.hip
    "qsae_binary_soft_table_polarize", "qsae_train_csr", "qsae_train_row_grad", "qsae_train_unit_grad", "qsae_train_col_sum",
    "qsae_train_table_unit_grad", "qsae_normalize_columns_table", "qsae_train_ternary_rows", "qsae_transpose_rows",
    "qsae_train_pre_bits", "qsae_train_bits_csr", "qsae_train_matryoshka_dsum_lists", "qsae_train_matryoshka_sign_rows",
    "qsae_train_matryoshka_finish", "qsae_train_matryoshka_secant",
    # train_gemm.hip
    "qsae_train_matryoshka_dpre", "qsae_train_gemm_tn", "qsae_train_matryoshka_dsum_dense", "qsae_train_ternary_dpre",
    "qsae_train_ternary_dweight", "qsae_blatent_binarize", "qsae_train_blatent_dpre", "qsae_train_blatent_dweight",
    # train_mask.hip
    "qsae_train_mask_init", "qsae_train_mask_update",
]


def _is_sizer(name: str) -> bool:
    return name.endswith("_workspace_bytes")


def _defined_in_train_sources():
    names = set()
    for src in TRAIN_SOURCES:
        text = (ROOT / "quantizedsae_amd" / "csrc" / src).read_text()
        names |= set(re.findall(r'^extern "C"\s+[A-Za-z_0-9]+\s+(qsae_[a-z0-9_]+)\s*\(', text, flags=re.M))
    return names


def test_guard_util_imports_without_a_gpu():
    import guard_util as GU
    assert GU.GUARD_BYTES % 4096 == 0 and GU.GUARD_BYTES > 127 * 1060 * 4
    assert callable(GU.GuardedArena) and callable(GU.snapshot) and callable(GU.unchanged)


def test_every_training_entry_point_has_a_guard_case():
    from quantizedsae_amd._lib import SIGNATURES
    import train_guard_cases as T
    assert len(ENTRY_POINTS) == 25 and len(set(ENTRY_POINTS)) == 25
    defined = _defined_in_train_sources()
    assert defined <= set(SIGNATURES), sorted(defined - set(SIGNATURES))
    in_table = {name for name in SIGNATURES if name in defined and not _is_sizer(name)}
    assert in_table == set(ENTRY_POINTS), sorted(in_table ^ set(ENTRY_POINTS))
    assert set(T.CASES) == in_table, sorted(set(T.CASES) ^ in_table)
    assert tuple(T.SHAPES) == ("minimal", "tails")
    # a training entry point added to the signature table is either listed above (and so tabled) or a sizer
    for name in SIGNATURES:
        if name.startswith(("qsae_train_", "qsae_blatent_")):
            assert name in ENTRY_POINTS or _is_sizer(name), f"{name} has no guard case in tests/train_guard_cases.py"
    # every sizer of these files is used by the case of its entry point (or is the one the two mask entry points share)
    for name in defined:
        if _is_sizer(name):
            entry = name[: -len("_workspace_bytes")]
            assert entry in ENTRY_POINTS or name == "qsae_train_mask_workspace_bytes", name
