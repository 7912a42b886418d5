// The fp32-MFMA similarity tile that coarse_sims_kernel (coarse_probe.hip) and flat_tile_kernel (flat_topk.hip) share:
// a 256-thread block owns 128 QUERIES (4 waves x 32 MFMA columns, operand in registers, prefetched one k-slab ahead)
// and walks chunks of 256 MFMA rows whose 16-row k-slabs are double-buffered in LDS (global -> registers while the
// previous slab's 8 x 8 MFMAs run -> the other buffer, one barrier per slab).  |row|^2 is accumulated from the values
// each thread stages (its row, every slab, ascending k), |x|^2 by each lane for its own query: dot and both norms are
// ascending-k fmaf chains from 0.f, the arithmetic of oracle_coarse_sims.  The kernels differ in their epilogues only.
#pragma once
#include "mfma_util.h"

namespace tpq {

constexpr int kCsRows = 256;  // rows per chunk (8 MFMA row tiles = 2 groups of 128)
constexpr int kCsKC = 16;     // k rows per LDS slab
constexpr int kCsSlab = kCsKC * kCsRows;

// |x_q|^2 of the query at xq (stride nq): one ascending-k chain, 16 loads in flight per step
__device__ __forceinline__ float sims_query_sq_norm(const float* __restrict__ xq, int d, int nq) {
  float q2 = 0.f;
  const float* __restrict__ p = xq;
  int k = 0;
  for (; k + 16 <= d; k += 16) {
    load_then_use<16>([&](int u) { return p[(int64_t)u * nq]; }, [&](int, float y) { q2 = fmaf(y, y, q2); });
    p += 16 * (int64_t)nq;
  }
  for (; k < d; ++k) {
    q2 = fmaf(*p, *p, q2);
    p += nq;
  }
  return q2;
}

// row inside a 32-row MFMA tile of accumulator register r in the lanes of half-wave `half`
__device__ __forceinline__ int sims_tile_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// One chunk: acc[t][r] = dot(row c0 + 32 t + sims_tile_row(r, half), query of lane l31), c2s[row] = |row|^2 (+inf for
// the rows past n_cells).  cs [2 * kCsSlab] and c2s [kCsRows] are LDS; every thread of the block calls it.  staged(cv) runs
// after the barrier that ends the previous chunk's LDS reads (cv: this thread's row of the chunk exists); what it
// writes to LDS is visible to the block when the call returns.
template <class Staged>
__device__ __forceinline__ void sims_chunk_mfma(const float* __restrict__ xq, bool qvalid, const float* __restrict__ C,
                                                int c0, int d, int nq, int n_cells, float* cs, float* c2s,
                                                f32x16 (&acc)[8], Staged&& staged) {
  const int lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int n_slabs = (d + kCsKC - 1) / kCsKC;
  const int nc = (n_cells - c0) < kCsRows ? (n_cells - c0) : kCsRows;
  const bool cv = (int)threadIdx.x < nc;  // this thread's row of the chunk exists
  const float* __restrict__ Cc = C + c0 + (cv ? (int)threadIdx.x : 0);
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
  __syncthreads();  // every wave finished the previous chunk (reads of cs and c2s)
  staged(cv);
  square_slab();
  // (rows past the last one get |row|^2 = +inf: their sims come out as -inf and drop out of
  // the group maxima without a per-element predicate)
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
