// IVF list scan: the k-th largest of a wave's key images, by a bit-wise binary search over chunks of 64 keys that never
// leave their registers -- what scan_finish_exact_kernel (scan_finish.h) cuts a query's lists at, and what cell_kth_kernel
// (scan_cells.hip) takes a query's threshold from.
#pragma once
#include "common.h"

namespace tpq {

// F_k over the first N chunks: the largest key image t with at least k entries >= t (0 while fewer than k entries exist)
template <int N, int NCH>
__device__ __forceinline__ unsigned finish_fk(const unsigned (&hi)[NCH], int k) {
  unsigned fk = 0u;
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned t = fk | (1u << bit);
    int n = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) n += __popcll(__ballot(hi[c] >= t));
    fk = n >= k ? t : fk;
  }
  return fk;
}
// ... over the T chunks in use (wave-uniform; the chunks behind them hold 0 and count for nothing)
template <int N, int NCH>
__device__ __forceinline__ unsigned finish_fk_upto(const unsigned (&hi)[NCH], int T, int k) {
  if constexpr (N >= NCH) {
    return finish_fk<NCH, NCH>(hi, k);
  } else {
    if (T <= N) return finish_fk<N, NCH>(hi, k);
    return finish_fk_upto<(N < 8 ? N + 2 : N + 4), NCH>(hi, T, k);
  }
}

}  // namespace tpq
