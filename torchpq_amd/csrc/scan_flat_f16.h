// What scan_flat_f16.hip and scan_flat_f16_cells.hip share: the value of a slot of the fp16 lists -- one definition, so
// the cell-major route's finish kernel returns the query-major scan's bits -- and the query-major scan with a probe
// cap, which the cell-major route runs as its threshold pass.
#pragma once
#include "scan_list.h"

namespace tpq {

// tpq_ivf_flat16_scan_topk over each query's first min(n_probe_list[q], probe_cap) probes; probe_cap == 0: no cap
// (defined in scan_flat_f16.hip: the entry point itself is this function with probe_cap = 0)
int ivf_flat16_scan_topk_capped(const uint32_t* vectors, const float* query, const uint8_t* is_empty,
                                const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                float* out_vals, int64_t* out_addr, int64_t n_slots, int d, int nq, int max_nprobe,
                                int k, int metric, int n_split, int probe_cap, void* workspace, size_t workspace_bytes,
                                tpq_stream_t stream);

namespace flat16 {

constexpr int kRowsInFlight = 8;  // dword loads in flight per lane: 16 dimensions, 8 x 256 B per wave

__device__ __forceinline__ float low_half(uint32_t w) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
}
__device__ __forceinline__ float high_half(uint32_t w) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}

// the two components of one dword against the query's components y0, y1
template <int METRIC>
__device__ __forceinline__ float pair_step(float v, float y0, float y1, uint32_t w) {
  v = metric_step<METRIC>(v, y0, low_half(w));
  return metric_step<METRIC>(v, y1, high_half(w));
}
// ... at xq[0] and xq[1] of the query
template <int METRIC>
__device__ __forceinline__ float pair_step(float v, const float* xq, uint32_t w) {
  return pair_step<METRIC>(v, xq[0], xq[1], w);
}

// The value of a slot: `col` is its dword of row 0, rows are `stride` dwords apart; component i of the query is
// xq[i * QS] (the query-major scan keeps the query in LDS, qstride = 1; the cell-major finish reads it from global
// memory, qstride = nq, the same address in every lane).  GROUPS groups of kRowsInFlight rows per trip (the order of
// the sum does not depend on it); rows left over one by one; the low half alone of the last row when d is odd.
template <int METRIC, int GROUPS>
__device__ __forceinline__ float slot_value(const uint32_t* __restrict__ col, const float* xq, int d, int64_t stride,
                                            int64_t qstride = 1) {
  float v = 0.f;
  const int pairs = d >> 1;
  int r = 0;
#pragma unroll GROUPS
  for (; r + kRowsInFlight <= pairs; r += kRowsInFlight) {
    uint32_t w[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) w[u] = col[(int64_t)u * stride];
    col += (int64_t)kRowsInFlight * stride;
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u)
      v = pair_step<METRIC>(v, xq[(int64_t)(2 * (r + u)) * qstride], xq[(int64_t)(2 * (r + u) + 1) * qstride], w[u]);
  }
  for (; r < pairs; ++r) {
    v = pair_step<METRIC>(v, xq[(int64_t)(2 * r) * qstride], xq[(int64_t)(2 * r + 1) * qstride], *col);
    col += stride;
  }
  if (d & 1) v = metric_step<METRIC>(v, xq[(int64_t)(d - 1) * qstride], low_half(*col));
  return v;
}

}  // namespace flat16
}  // namespace tpq
