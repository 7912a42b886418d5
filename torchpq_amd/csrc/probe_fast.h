// What tpq_ivfpq_coarse_probe (coarse_probe.hip) needs of the coarse step's fp16 route (probe_sims.hip): whether a shape
// has one, its sizes, the once-per-codebook preparation, and the route itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "row_select.h"

namespace tpq {
int lloyd_probe_supported(int d, int nq, int n_cells);
// groups of cells whose maxima the fast pass keeps (32 cells up to 8 192, 64 up to 16 384, 128 beyond)
int lloyd_probe_groups(int n_cells);
size_t lloyd_probe_workspace_bytes(int d, int nq, int n_cells);
// the part that depends on the centroids alone (mean, scale, fp16 fragments, row copies, |C|^2): once per codebook
size_t lloyd_probe_prepared_bytes(int d, int n_cells);
int lloyd_probe_prepare(const float* centroids, int d, int n_cells, char* prepared, hipStream_t st);
// the fast similarities of every (query, cell) pair, then the n_probe best cells of every query with their fp32 values
// and the epilogue `pe`; n_probe + 16 <= 1024.  prepared == nullptr: prepared into the workspace for this call
int lloyd_probe_select(const float* query, const float* centroids, const void* prepared, int d, int nq, int n_cells,
                       int n_probe, float* topk_sims, int64_t* cells, const ProbeEpilogue& pe, char* ws, hipStream_t st);
}  // namespace tpq
