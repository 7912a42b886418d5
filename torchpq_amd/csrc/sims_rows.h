// The fp32-MFMA similarity chunk of sims_chunk.h on rows the caller names: thread i of the block stages row `row` of C,
// whatever it is -- a gathered address (flat_filtered.hip) or a slot of a probed cell (scan_flat_cells.hip).  A row's dot
// product and norm do not depend on where in a chunk the row sits.
#pragma once
#include "sims_chunk.h"

namespace tpq {

// sims_chunk_mfma (sims_chunk.h) on gathered rows: this thread stages row `row` of C (row < 0: none; such a row's
// |row|^2 is +inf), everything else -- the slab pipeline, the chains, what staged(cv) may do -- is that function's.
template <class Staged>
__device__ __forceinline__ void sims_rows_mfma(const float* __restrict__ xq, bool qvalid, const float* __restrict__ C,
                                               int row, int d, int nq, int n_cells, float* cs, float* c2s,
                                               f32x16 (&acc)[8], Staged&& staged) {
  const int lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int n_slabs = (d + kCsKC - 1) / kCsKC;
  const bool cv = row >= 0;
  const float* __restrict__ Cc = C + (cv ? row : 0);
  float rs[kCsKC], yc[kCsKC / 2], yn[kCsKC / 2];
  float csq = 0.f;
  auto load_slab = [&](int kb) {
    const float* __restrict__ p = Cc + (int64_t)kb * n_cells;
#pragma unroll
    for (int u = 0; u < kCsKC; ++u) {
      rs[u] = (cv && kb + u < d) ? *p : 0.f;
      p += n_cells;
    }
  };
  auto square_slab = [&]() {
#pragma unroll
    for (int u = 0; u < kCsKC; ++u) csq = fmaf(rs[u], rs[u], csq);
  };
  auto store_slab = [&](float* dst) {
#pragma unroll
    for (int u = 0; u < kCsKC; ++u) dst[u * kCsRows + threadIdx.x] = rs[u];
  };
  auto load_y = [&](int kb, float (&y)[kCsKC / 2]) {
    const float* __restrict__ p = xq + (int64_t)(kb + half) * nq;
#pragma unroll
    for (int j = 0; j < kCsKC / 2; ++j) {
      y[j] = (qvalid && kb + 2 * j + half < d) ? *p : 0.f;
      p += 2 * (int64_t)nq;
    }
  };
  load_slab(0);
  load_y(0, yc);
  __syncthreads();  // every wave finished the previous chunk (reads of cs, c2s and what staged() wrote)
  staged(cv);
  square_slab();
  if (n_slabs == 1) c2s[threadIdx.x] = cv ? csq : INFINITY;
  store_slab(cs);
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  __syncthreads();
  for (int sb = 0; sb < n_slabs; ++sb) {
    const float* cur = cs + (sb & 1) * kCsSlab;
    const bool more = sb + 1 < n_slabs;
    if (more) {
      load_slab((sb + 1) * kCsKC);
      load_y((sb + 1) * kCsKC, yn);
    }
#pragma unroll
    for (int j = 0; j < kCsKC / 2; ++j) {
      const float* crow = cur + (2 * j + half) * kCsRows + l31;  // A operand [row][k]
#pragma unroll
      for (int t = 0; t < 8; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(crow[t * 32], yc[j], acc[t], 0, 0, 0);
    }
    if (more) {
      square_slab();
      if (sb + 2 == n_slabs) c2s[threadIdx.x] = cv ? csq : INFINITY;
      store_slab(cs + ((sb + 1) & 1) * kCsSlab);
#pragma unroll
      for (int j = 0; j < kCsKC / 2; ++j) yc[j] = yn[j];
    }
    __syncthreads();
  }
}

}  // namespace tpq
