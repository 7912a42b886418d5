// What scan_flat.hip and scan_flat_cells.hip share: the query-major IVFFlat scan with a probe cap, which the cell-major
// route runs as its threshold pass.
#pragma once
#include "common.h"

namespace tpq {

// tpq_ivfflat_scan_topk over each query's first min(n_probe_list[q], probe_cap) probes; probe_cap == 0: no cap
// (defined in scan_flat.hip: the entry point itself is this function with probe_cap = 0)
int ivfflat_scan_topk_capped(const float* vectors, const float* query, const uint8_t* is_empty,
                             const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                             float* out_vals, int64_t* out_addr, int64_t n_slots, int d, int nq, int max_nprobe, int k,
                             int metric, int n_split, int probe_cap, void* workspace, size_t workspace_bytes,
                             tpq_stream_t stream);

}  // namespace tpq
