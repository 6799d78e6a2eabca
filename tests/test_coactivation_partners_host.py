"""Co-activation partner sets without a GPU: the ABI surface, the argument checks that answer before any HIP call, and
the summary functions on CPU tensors against the reference's own results (tests/golden/coactivation_summary_*.npz,
written by tools/gen_golden_coactivation_summary.py)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import coactivation_partners_util as U
from quantizedsae_amd import _lib, build
from quantizedsae_amd.inference import summary as SM

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NEW = ["qsae_coactivation_partners_bits", "qsae_coactivation_partners_sparse", "qsae_coactivation_partner_counts",
       "qsae_coactivation_partner_counts_dense"]
P16 = ctypes.c_void_p(16)                                       # non-null, never dereferenced: the checks come first


def goldens():
    return {p.stem[len(U.GOLDEN_PREFIX):]: np.load(p) for p in sorted(GOLDEN.glob(f"{U.GOLDEN_PREFIX}*.npz"))}


def test_goldens_cover_the_recipes():
    assert set(goldens()) == set(U.RECIPES)


def test_symbols_are_declared_bound_and_exported():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    declared = ge.declared_symbols()
    exported = set(build.exported_symbols(build.LIB))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert "coactivation_partners.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 4 and _lib.load().qsae_abi_version() == 4


def test_argument_checks_answer_before_any_hip_call():
    lib = _lib.load()
    bad, ws = _lib.ERR_INVALID_ARG, _lib.ERR_WORKSPACE
    big = 1 << 20
    bits = lib.qsae_coactivation_partners_bits
    assert bits(None, 2, 4, 64, None, P16, 2, P16, big, None) == bad            # null zbits, B > 0
    assert bits(P16, 2, 4, 64, None, None, 2, P16, big, None) == bad            # null partners
    assert bits(P16, 2, 4, 48, None, P16, 2, P16, big, None) == bad             # nbits % 32 != 0
    assert bits(P16, 2, 4, 0, None, P16, 2, P16, big, None) == bad
    assert bits(P16, 1, 4, 64, None, P16, 2, P16, big, None) == bad             # words_ld < nbits / 32
    assert bits(P16, 2, 4, 64, None, P16, 1, P16, big, None) == bad             # ld_words < P / 32
    assert bits(P16, 2, -1, 64, None, P16, 2, P16, big, None) == bad
    assert b"invalid argument" in lib.qsae_last_error()
    need = lib.qsae_coactivation_bits_workspace_bytes(4, 64)
    assert need == 64 * 32
    assert bits(P16, 2, 4, 64, None, P16, 2, P16, need - 1, None) == ws
    assert bits(P16, 2, 4, 64, None, P16, 2, None, 0, None) == ws
    assert b"workspace too small" in lib.qsae_last_error()
    assert bits(P16, 2, 4, 64, None, P16, 2, ctypes.c_void_p(8), need, None) == bad  # misaligned workspace
    assert bits(None, 2, 0, 64, None, None, 2, None, 0, None) == 0              # B == 0 does nothing

    sparse = lib.qsae_coactivation_partners_sparse
    assert sparse(None, None, 4, 8, 64, P16, 2, None) == bad
    assert sparse(P16, None, 4, 8, 64, None, 2, None) == bad
    assert sparse(P16, None, 4, 0, 64, P16, 2, None) == bad                     # k outside 1..256
    assert sparse(P16, None, 4, 257, 64, P16, 2, None) == bad
    assert sparse(P16, None, 4, 8, 0, P16, 2, None) == bad                      # H <= 0
    assert sparse(P16, None, 4, 8, 65, P16, 2, None) == bad                     # ld_words < ceil(H / 32)
    assert sparse(None, None, 0, 8, 64, None, 2, None) == 0

    counts = lib.qsae_coactivation_partner_counts
    assert counts(None, 64, 2, None, 64, P16, None) == bad
    assert counts(P16, 64, 2, None, 64, None, None) == bad
    assert counts(P16, 48, 2, None, 64, P16, None) == bad                       # P % 32 != 0
    assert counts(P16, 64, 1, None, 64, P16, None) == bad                       # ld_words < P / 32
    assert counts(P16, 64, 2, None, 0, P16, None) == bad                        # H <= 0

    dense = lib.qsae_coactivation_partner_counts_dense
    assert dense(None, 64, 4, 64, 0, P16, None) == bad
    assert dense(P16, 64, 4, 64, 0, None, None) == bad
    assert dense(P16, 63, 4, 64, 0, P16, None) == bad                           # ld < H
    assert dense(P16, 64, 4, 0, 0, P16, None) == bad                            # H <= 0
    assert dense(P16, 64, 4, 64, -1, P16, None) == bad
    assert dense(None, 64, 0, 64, 0, None, None) == 0


@pytest.mark.parametrize("name", list(U.RECIPES))
def test_summary_on_partner_counts_equals_the_reference(name):
    g = goldens()[name]
    act = torch.from_numpy(g["activation_counts"])
    counts = torch.from_numpy(g["partner_counts"])
    sizes, threshold = g["level_sizes"].tolist(), int(g["threshold"])
    H = act.numel()

    def close(ours, ref):                                       # the division's rounding: at most two fp32 roundings
        assert abs(float(np.float32(ours)) - ref) <= 2.0 ** -23 * abs(ref), (ours, ref)

    assert SM.summarize_activation_counts(act) == g["mean_activation_count"][0]
    assert SM.count_below_threshold(act, threshold) == g["below_threshold"][0]
    close(SM.average_coactivating_features(counts, act), g["avg_coactivating_features"][0])
    close(SM.average_coactivating_features(counts, act, row_mask=torch.from_numpy(g["row_mask"])),
          float(g["avg_coactivating_selected"]))
    for f in range(0, H, 7):                                    # a one-hot selection is the count itself
        one = torch.zeros(H, dtype=torch.bool)
        one[f] = True
        assert SM.average_coactivating_features(counts, act, row_mask=one) == float(counts[f] if act[f] > 0 else 0)
    for lv, sl in enumerate(U.level_slices(sizes), start=1):
        row_mask = torch.zeros(H, dtype=torch.bool)
        row_mask[sl] = True
        assert SM.summarize_activation_counts(act[sl]) == g["mean_activation_count"][lv]
        assert SM.count_below_threshold(act[sl], threshold) == g["below_threshold"][lv]
        close(SM.average_coactivating_features(counts, act, row_mask=row_mask), g["avg_coactivating_features"][lv])

    out = SM.summarize_sae({"activation_counts": act, "coactivation": None, "coactivation_partner_counts": counts},
                           sizes, threshold)
    assert len(out["levels"]) == len(sizes)
    for lv, block in enumerate([out] + out["levels"]):
        assert block["mean_activation_count"] == g["mean_activation_count"][lv]
        assert block["below_threshold"] == g["below_threshold"][lv]
        close(block["avg_coactivating_features"], g["avg_coactivating_features"][lv])
        assert block["avg_unique_tokens"] is None
    flat = SM.summarize_sae({"activation_counts": act, "coactivation_partner_counts": counts})
    assert flat["levels"] == [] and flat["below_threshold"] == int((act < 1).sum())


def test_summary_counts_tokens_from_lists_and_csr():
    act = torch.tensor([2, 0, 3, 1])
    lists = [[5, 5], [], [1, 2, 1], [9]]
    csr = (torch.tensor([0, 2, 2, 5, 6]), torch.tensor([5, 5, 1, 2, 1, 9], dtype=torch.int32))
    for tokens in (lists, csr):
        out = SM.summarize_sae({"activation_counts": act, "coactivation_partner_counts": torch.tensor([1, 0, 2, 1]),
                                "tokens_per_feature": tokens}, [2, 2])
        assert out["avg_unique_tokens"] == (1 + 2 + 1) / 3
        assert [lv["avg_unique_tokens"] for lv in out["levels"]] == [1.0, 1.5]
        assert out["avg_coactivating_features"] == 4 / 3


def test_empty_inputs_give_zero():
    e = torch.zeros(0, dtype=torch.int64)
    assert SM.average_coactivating_features(e, e) == 0.0
    assert SM.average_coactivating_features(torch.zeros((0, 0), dtype=torch.int32), e) == 0.0
    assert SM.average_coactivating_features(torch.tensor([3, 4]), torch.tensor([0, 0])) == 0.0
    assert SM.count_below_threshold(e, 1) == 0


def test_level_sizes_by_model_type():
    from quantizedsae_amd import BinarySAE, QuantizedMatryoshkaSAE, ResidualQuantizedSAE
    q = QuantizedMatryoshkaSAE(16, 128, top_k=4, abs_range=2, n_bits=3)
    assert SM.level_sizes(q) == list(q.decoder.nested_dictionary_size) and sum(SM.level_sizes(q)) == 128
    r = ResidualQuantizedSAE(16, 64, top_k=4, abs_range=1.5, n_bits=3)
    assert SM.level_sizes(r) == list(r.sae_hidden_dims)
    assert SM.level_sizes(BinarySAE(16, 64, gamma=4.0, n_bits=4)) is None


def test_matrix_on_the_cpu_has_no_fallback_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    co = torch.ones((4, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SM.average_coactivating_features(co, torch.ones(4, dtype=torch.int64))
