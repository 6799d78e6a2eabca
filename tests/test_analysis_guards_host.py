"""Completeness of the second guard table (tests/analysis_guard_cases.py) against the C ABI, without a GPU: every entry point
that the ten kernel files define has a case and every sizer of these files is used by its entry's case; and a ledger over the
whole signature table -- every function of the ABI is guarded by exactly one table or named test, has no device buffers, or is
listed by name as not yet guarded.  A function added to the ABI later fails here until someone places it."""
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
TESTS = Path(__file__).resolve().parent
sys.path.insert(0, str(TESTS))

#: kernel file -> the entry points it defines (sizers apart)
ENTRY_POINTS = {
    "analysis.hip": ["qsae_activation_counts", "qsae_activation_counts_bits", "qsae_coactivation_sparse", "qsae_quantize_bits"],
    "coactivation_bits.hip": ["qsae_coactivation_bits"],
    "coactivation_partners.hip": ["qsae_coactivation_partners_bits", "qsae_coactivation_partners_sparse",
                                  "qsae_coactivation_partner_counts", "qsae_coactivation_partner_counts_dense"],
    "token_lists.hip": ["qsae_token_lists_count", "qsae_token_lists_count_bits", "qsae_token_lists_fill", "qsae_token_lists_regroup"],
    "token_overlap.hip": ["qsae_token_overlap_hist"],
    "dictionary.hip": ["qsae_atom_inv_norms", "qsae_cosine_compare"],
    "evaluation.hip": ["qsae_quantization_error", "qsae_dataset_moments_add"],
    "optim.hip": ["qsae_adam_step", "qsae_adam_step_prefilter"],
    "trainer.hip": ["qsae_rows_nan_bitmap", "qsae_gather_rows", "qsae_trainer_loss"],
    "watch.hip": ["qsae_tensor_stats"],
}
#: sizer -> the entry points whose cases must size their workspace with it
SIZERS = {
    "qsae_coactivation_bits_workspace_bytes": ["qsae_coactivation_bits", "qsae_coactivation_partners_bits"],
    "qsae_token_lists_workspace_bytes": ["qsae_token_lists_count", "qsae_token_lists_count_bits"],
    "qsae_token_overlap_hist_workspace_bytes": ["qsae_token_overlap_hist"],
    "qsae_cosine_compare_workspace_bytes": ["qsae_cosine_compare"],
    "qsae_quantization_error_workspace_bytes": ["qsae_quantization_error"],
    "qsae_dataset_moments_workspace_bytes": ["qsae_dataset_moments_add"],
    "qsae_trainer_loss_workspace_bytes": ["qsae_trainer_loss"],
    "qsae_tensor_stats_workspace_bytes": ["qsae_tensor_stats"],
}

# ---- the ledger ------------------------------------------------------------------------------------------------------------
#: guarded by ad-hoc guard words or a guard table inside the named GPU test
GUARDED_ELSEWHERE = {
    "test_kmeans_gpu.py": ["qsae_kmeans_assign_f32", "qsae_kmeans_update_f32"],
    "test_top_examples_gpu.py": ["qsae_top_examples_compact", "qsae_top_examples_dense", "qsae_top_examples_decode"],
    "test_dictionary_neighbors_gpu.py": ["qsae_nearest_atoms_i8"],
    "test_neighbors_f32_gpu.py": ["qsae_nearest_atoms_f32"],
    "test_activity_gpu.py": ["qsae_activity_add_compact", "qsae_activity_add_bits", "qsae_activity_add_dense", "qsae_activity_summary"],
    "test_resample_gpu.py": ["qsae_resample_row_weights", "qsae_resample_draw", "qsae_resample_alive_stats",
                             "qsae_resample_write_table", "qsae_resample_write_binary"],
}
#: no device buffer among the arguments: version, error text, device info, profile events, host-side answers (and every
#: ``*_bytes`` sizer, by suffix)
NO_DEVICE_BUFFERS = ["qsae_abi_version", "qsae_last_error", "qsae_device_info", "qsae_profile_sweep_events",
                     "qsae_profile_event_create", "qsae_profile_event_destroy", "qsae_profile_event_elapsed_ms",
                     "qsae_profile_sweep_flop_fraction", "qsae_matryoshka_sizes", "qsae_split_dec_supported"]
#: the inference path, not yet guarded: the visible remainder for a later table
NOT_YET_GUARDED = [
    "qsae_kperm_rows", "qsae_encode_dense", "qsae_encode_dense_kperm", "qsae_emu_pack_w", "qsae_encode_dense_emu", "qsae_encode_bits",
    "qsae_topk_rows", "qsae_encode_topk", "qsae_encode_topk_kperm", "qsae_encode_topk_latent", "qsae_prefilter_pack_w",
    "qsae_encode_topk_prefilter", "qsae_binary_forward_prefilter", "qsae_prefilter_submit", "qsae_prefilter_finish",
    "qsae_table_forward_prefilter", "qsae_prefilter_submit_table", "qsae_prefilter_finish_table", "qsae_densify", "qsae_pack_binary",
    "qsae_unpack_binary", "qsae_decode_binary_sparse", "qsae_decode_table_sparse", "qsae_binary_soft_table", "qsae_pack_ternary",
    "qsae_decode_ternary_dense", "qsae_pack_matryoshka", "qsae_decode_matryoshka", "qsae_encode_bits_prefilter",
    "qsae_encode_bits_prefilter_submit", "qsae_encode_bits_prefilter_finish", "qsae_encode_bits_band", "qsae_encode_bits_band_submit",
    "qsae_encode_bits_band_finish", "qsae_pack_matryoshka_rows", "qsae_decode_matryoshka_sparse", "qsae_expand_codes_bf16",
    "qsae_decode_ternary_dense_split", "qsae_split_scale_bf16", "qsae_decode_matryoshka_split", "qsae_pack_bits_gt",
    "qsae_residual_update", "qsae_threshold_ge", "qsae_scale_bias_rows", "qsae_sq_err_sum",
]


def _is_sizer(name: str) -> bool:
    return name.endswith("_bytes")


def _defined_in(src: str):
    text = (ROOT / "quantizedsae_amd" / "csrc" / src).read_text()
    return set(re.findall(r'^extern "C"\s+[A-Za-z_0-9]+\s+(qsae_[a-z0-9_]+)\s*\(', text, flags=re.M))


def _all_entries():
    return [name for names in ENTRY_POINTS.values() for name in names]


def test_guard_bytes_cover_the_worst_fail_open_store():
    """A row predicate that fails open writes up to 255 rows past the last one (the widest tile of these kernels is 256 rows):
    the guard is wider than that at the widest row stride tabled, and than the training table's own worst case."""
    import analysis_guard_cases as A
    import guard_util as GU
    assert GU.GUARD_BYTES == 1 << 20 and GU.GUARD_BYTES % 4096 == 0
    assert GU.GUARD_BYTES > 255 * A.WIDEST_ROW_STRIDE_BYTES and GU.GUARD_BYTES > 127 * 1060 * 4
    assert A.WIDEST_ROW_STRIDE_BYTES >= max(291 * 4, 241 * 4, 132 * 4, 65 * 8 * 4)


def test_the_harness_extensions_without_a_gpu():
    import ctypes as C
    import guard_util as GU
    assert C.cast(GU.HostArray([3, 4]).carg(), C.POINTER(C.c_int32))[1] == 4                       # the training table's use
    assert C.cast(GU.HostArray([3, 1 << 40], "int64").carg(), C.POINTER(C.c_int64))[1] == 1 << 40
    assert C.cast(GU.HostArray([0.5, 0.25], "float32").carg(), C.POINTER(C.c_float))[1] == 0.25
    assert GU.HostArray((), "float32").carg()                                                      # never a NULL array
    a, b = GU.Buf("a", "in"), GU.Buf("b", "out", shape=(1,), offset_bytes=4)
    call = GU.Call("x", "qsae_x", [GU.HostPointers([a, None]), GU.HostPointers([b]), 3], lambda t: {})
    assert [x.name for x in call.bufs] == ["a", "b"]


def test_every_entry_point_of_the_ten_files_has_a_guard_case():
    from quantizedsae_amd._lib import SIGNATURES
    import analysis_guard_cases as A
    entries = _all_entries()
    assert len(ENTRY_POINTS) == 10 and len(entries) == 24 and len(set(entries)) == 24
    sizers = set()
    for src, names in ENTRY_POINTS.items():
        defined = _defined_in(src)
        assert defined <= set(SIGNATURES), sorted(defined - set(SIGNATURES))
        assert {n for n in defined if not _is_sizer(n)} == set(names), (src, sorted(defined))
        sizers |= {n for n in defined if _is_sizer(n)}
    assert set(A.CASES) == set(entries), sorted(set(A.CASES) ^ set(entries))
    assert tuple(A.SHAPES) == ("minimal", "tails")
    assert set(A.FORMS) <= set(entries)
    # every sizer of these files is used by the case of its entry point: the builder's source names it in its Call
    assert sizers == set(SIZERS), sorted(sizers ^ set(SIZERS))
    text = (TESTS / "analysis_guard_cases.py").read_text()
    for sizer, users in SIZERS.items():
        assert text.count(f'sizer=("{sizer}"') >= 1, sizer
        assert all(u in entries for u in users)
    # the entries that take a workspace are exactly those whose signature ends (..., void*, size_t, stream)
    import ctypes as C
    with_ws = {n for n in entries if SIGNATURES[n][1][-2:] == [C.c_size_t, C.c_void_p]}
    staged = {"qsae_token_lists_fill"}                           # reads the workspace its count call left: sized by that call
    assert with_ws - staged == {u for users in SIZERS.values() for u in users}, sorted(with_ws)


def test_ledger_places_every_function_of_the_abi_exactly_once():
    from quantizedsae_amd._lib import SIGNATURES
    import test_train_guards_host as TH
    groups = {
        "training table": list(TH.ENTRY_POINTS),
        "analysis table": _all_entries(),
        "no device buffers": NO_DEVICE_BUFFERS + [n for n in SIGNATURES if _is_sizer(n)],
        "not yet guarded": NOT_YET_GUARDED,
    }
    for test_file, names in GUARDED_ELSEWHERE.items():
        text = (TESTS / test_file).read_text()
        assert "0x5A" in text or "guard_util" in text, f"{test_file} holds no guards"
        for name in names:
            assert re.search(rf"\b{name}\b", text), f"{test_file} does not call {name}"
        groups[test_file] = names
    placed = {}
    for group, names in groups.items():
        assert len(set(names)) == len(names), group
        for name in names:
            assert name in SIGNATURES, f"{name} ({group}) is not in the ABI"
            assert name not in placed, f"{name} is in two groups: {placed[name]} and {group}"
            placed[name] = group
    missing = [n for n in SIGNATURES if n not in placed]
    assert not missing, f"not placed in the guard ledger (tests/test_analysis_guards_host.py): {missing}"
    # nothing that is guarded may sit in the remainder, and no sizer is tabled
    assert not any(_is_sizer(n) for g in groups if g != "no device buffers" for n in groups[g])
