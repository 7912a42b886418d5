"""The table of the guarded-buffer tests (tests/test_gpu_guarded_buffers.py): which case runs which entry points of
the library under guarded, pre-filled allocations (tests/guarded_alloc.py).  Importing it needs no GPU:
tests/test_guarded_alloc_cpu.py checks the table against torchpq_amd/_lib.py's signature table and against the symbols
the wrappers in torchpq_amd/kernels/ reach.

CASE_SYMBOLS  case id -> the entry points the case calls (through a wrapper, or directly where no wrapper reaches one)
CASES         entry-point symbol -> case ids (the inverse)
NOT_BIT_EXACT case id -> why its results are not compared bit for bit, and with what instead
"""

_SCAN_AUX = ("tpq_ivfpq_pack_codes",)

CASE_SYMBOLS = {
    # ---- IVFPQTopkHip, plain -----------------------------------------------------------------------------------------
    "scan_reference_layout_m8": ("tpq_ivfpq_scan_topk", "tpq_ivfpq_search_fused_tickets"),
    "scan_one_launch_m16_split7_tickets": ("tpq_ivfpq_scan_topk_packed_tickets", "tpq_ivfpq_search_fused_tickets") + _SCAN_AUX,
    "scan_three_launch_direct_no_tickets": ("tpq_ivfpq_scan_topk_packed", "tpq_ivfpq_search_fused") + _SCAN_AUX,
    "scan_pools_m64_k600": ("tpq_ivfpq_scan_topk_packed_tickets",) + _SCAN_AUX,
    "scan_pools_split_clamp_m120_k1000": ("tpq_ivfpq_scan_topk_packed_tickets",) + _SCAN_AUX,
    "scan_dump_f32_m16_k40": ("tpq_ivfpq_search_fused_tickets", "tpq_ivfpq_scan_topk_packed_tickets") + _SCAN_AUX,
    "scan_dump_sel16_split_tail_ordered": ("tpq_ivfpq_search_fused_tickets",) + _SCAN_AUX,
    "scan_dump_sel16_lists_in_use_only": ("tpq_ivfpq_search_fused_tickets",) + _SCAN_AUX,
    "scan_dump_sel16_w8_k300": ("tpq_ivfpq_search_fused_tickets",) + _SCAN_AUX,
    "scan_cell_major_slot_norms": ("tpq_ivfpq_search_fused_cells",) + _SCAN_AUX,
    "scan_cell_major_own_norms": ("tpq_ivfpq_search_fused_cells",) + _SCAN_AUX,
    "scan_exact_redo_in_a_dump_batch": ("tpq_ivfpq_search_fused_tickets",) + _SCAN_AUX,
    "scan_exact_redo_in_one_launch": ("tpq_ivfpq_scan_topk_packed_tickets",) + _SCAN_AUX,
    "scan_lds_fallback_m128": ("tpq_ivfpq_scan_topk_packed_tickets",) + _SCAN_AUX,
    # ---- IVFPQTopkHip, residual --------------------------------------------------------------------------------------
    "scan_residual_sorted_lists_m8": ("tpq_ivfpq_scan_topk_residual_packed", "tpq_ivfpq_residual_slot_terms",
                                      "tpq_residual_part1") + _SCAN_AUX,
    "scan_residual_sorted_lists_m64": ("tpq_ivfpq_scan_topk_residual_packed", "tpq_ivfpq_residual_slot_terms",
                                       "tpq_residual_part1") + _SCAN_AUX,
    "scan_residual_full_table_and_precomputed": ("tpq_ivfpq_scan_topk_residual",),
    # ---- the other scan-side entry points ----------------------------------------------------------------------------
    "adc_lut": ("tpq_adc_lut",),
    "residual_part1": ("tpq_residual_part1",),
    "residual_slot_terms": ("tpq_ivfpq_residual_slot_terms",),
    "scan_order": ("tpq_ivfpq_scan_order",),
    "cell_candidates_slot_norms": ("tpq_ivfpq_cell_candidates",),
    "cell_candidates_own_norms": ("tpq_ivfpq_cell_candidates",),
    "slot_filter_build_77": ("tpq_slot_filter_build",),
    # ---- filtered search -----------------------------------------------------------------------------------------------
    "filtered_plain_m8": ("tpq_ivfpq_scan_filtered_topk",),
    "filtered_plain_m148": ("tpq_ivfpq_scan_filtered_topk",),
    "filtered_residual_m8": ("tpq_ivfpq_scan_filtered_residual_topk",),
    "filtered_residual_m148": ("tpq_ivfpq_scan_filtered_residual_topk",),
    # ---- range search and the other list scans -----------------------------------------------------------------------
    "ivfpq_range_plain": ("tpq_ivfpq_range_count", "tpq_ivfpq_range_fill"),
    "ivfpq_range_residual": ("tpq_ivfpq_range_residual_count", "tpq_ivfpq_range_residual_fill"),
    "ivfflat_topk": ("tpq_ivfflat_scan_topk",),
    "ivfflat_range": ("tpq_ivfflat_range_count", "tpq_ivfflat_range_fill"),
    "ivfpq4_topk": ("tpq_ivfpq4_scan_topk",),
    "ivfpq4_residual_topk": ("tpq_ivfpq4_scan_residual_topk",),
    "ivfpqr_rerank": ("tpq_ivfpqr_rerank",),
    "flat_topk": ("tpq_flat_topk",),
    "flat_range": ("tpq_flat_range_count", "tpq_flat_range_fill"),
    # ---- the coarse step -----------------------------------------------------------------------------------------------
    "coarse_probe_d32_nq5_all_cells": ("tpq_ivfpq_coarse_probe_route",),
    "coarse_probe_d7_one_query_one_probe": ("tpq_ivfpq_coarse_probe_route",),
    "coarse_probe_fp16_last_group_half_full": ("tpq_ivfpq_coarse_probe_route", "tpq_ivfpq_coarse_probe_prepare"),
    "coarse_probe_group_filter": ("tpq_ivfpq_coarse_probe_route",),
    "coarse_probe_600_probes": ("tpq_ivfpq_coarse_probe_route", "tpq_ivfpq_coarse_probe_prepare"),
    "coarse_probe_direct_auto": ("tpq_ivfpq_coarse_probe",),
    "topk_select": ("tpq_topk_select",),
    "coarse_select": ("tpq_coarse_select",),
    "smart_probing": ("tpq_smart_probing",),
    # ---- k-means and assign ---------------------------------------------------------------------------------------------
    "max_sim_fp32": ("tpq_max_sim",),
    "max_sim_bf16x3": ("tpq_max_sim_split",),
    "max_sim_bf16x3_unsupported_shape": ("tpq_max_sim",),
    "coarse_assign_auto": ("tpq_coarse_assign_route",),
    "coarse_assign_cascade_narrow": ("tpq_coarse_assign_route",),
    "coarse_assign_cascade_wide": ("tpq_coarse_assign_route",),
    "coarse_assign_cascade_wide_one_centroid": ("tpq_coarse_assign_route",),
    "coarse_assign_candidate_overflow": ("tpq_coarse_assign_route",),
    "coarse_assign_direct": ("tpq_coarse_assign",),
    "max_sim_select_cached_workspace": ("tpq_max_sim_select",),
    "lloyd_prepare_and_two_steps": ("tpq_lloyd_prepare", "tpq_lloyd_step"),
    "compute_centroids_mfma": ("tpq_compute_centroids",),
    "compute_centroids_lds": ("tpq_compute_centroids",),
    "compute_centroids_lds_k2409": ("tpq_compute_centroids",),
    "compute_centroids_global_k2410": ("tpq_compute_centroids",),
    # ---- containers -------------------------------------------------------------------------------------------------------
    "get_ioa": ("tpq_get_ioa",),
    "get_write_address": ("tpq_get_write_address",),
    "get_cell_by_address": ("tpq_get_cell_by_address",),
    "get_id_by_address": ("tpq_get_id_by_address",),
    "get_address_by_id": ("tpq_get_address_by_id",),
    "grow_cells": ("tpq_grow_cells",),
    "scatter_codes": ("tpq_scatter_codes",) + _SCAN_AUX,
    "pack_codes_m24": _SCAN_AUX,
    "pack_codes_m120": _SCAN_AUX,
    "pq_decode": ("tpq_pq_decode",),
    # ---- the index end to end ----------------------------------------------------------------------------------------
    "index_plain_end_to_end": ("tpq_ivfpq_coarse_probe_route", "tpq_ivfpq_search_fused_tickets", "tpq_ivfpq_range_count",
                               "tpq_ivfpq_range_fill", "tpq_ivfpq_scan_filtered_topk", "tpq_slot_filter_build",
                               "tpq_grow_cells", "tpq_scatter_codes"),
    "index_residual_end_to_end": ("tpq_ivfpq_coarse_probe_route", "tpq_ivfpq_scan_topk_residual_packed",
                                  "tpq_ivfpq_range_residual_count", "tpq_ivfpq_range_residual_fill",
                                  "tpq_ivfpq_scan_filtered_residual_topk", "tpq_slot_filter_build", "tpq_grow_cells",
                                  "tpq_scatter_codes"),
}

CASE_IDS = list(CASE_SYMBOLS)

CASES = {}
for _cid, _symbols in CASE_SYMBOLS.items():
    for _s in _symbols:
        CASES.setdefault(_s, []).append(_cid)

# The only comparisons that are not bit for bit: results that depend on the order in which workgroups arrive.  `source`:
# the lines that make them so; `comparison`: the existing test's own comparison, imported by the GPU module.
_CENTROID_ATOMICS = ("csrc/centroid_update.hip:70, :75 (LDS route: a block's partial sums), :92, :94 (global route) and "
                     ":323, :330 (matrix route): unsafeAtomicAdd of fp32 sums and counts")
NOT_BIT_EXACT = {
    "compute_centroids_mfma": dict(source=_CENTROID_ATOMICS, comparison="test_gpu_centroid_update._check_general"),
    "compute_centroids_lds": dict(source=_CENTROID_ATOMICS, comparison="test_gpu_centroid_update._check_general"),
    "compute_centroids_lds_k2409": dict(source=_CENTROID_ATOMICS, comparison="test_gpu_centroid_update._check_general"),
    "compute_centroids_global_k2410": dict(source=_CENTROID_ATOMICS,
                                           comparison="test_gpu_centroid_update._check_general"),
    "lloyd_prepare_and_two_steps": dict(
        source="csrc/lloyd.hip:233, :240 (update_kernel) and :258, :260 (flagged_accum_kernel): unsafeAtomicAdd of fp32 "
               "sums and counts -- the new centroids only; maxima and labels are compared bit for bit",
        comparison="test_gpu_lloyd_update.lloyd_bound"),
    "cell_candidates_slot_norms": dict(
        source="csrc/scan_cells.hip:566: a wave appends its admitted rows at atomicAdd(&cnt[q], fill) -- the candidates "
               "of a query arrive in any order; their set, values, count and band are compared bit for bit",
        comparison="test_gpu_scan_cell_norms._pairs"),
    "cell_candidates_own_norms": dict(
        source="csrc/scan_cells.hip:566: as cell_candidates_slot_norms",
        comparison="test_gpu_scan_cell_norms._pairs"),
}
