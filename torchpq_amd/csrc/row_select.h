// One wave selects the top-k of a row: what topk_select_kernel (select.hip), probe_small_kernel (coarse_probe.hip) and
// probe_select_fast_kernel (probe_sims.hip) share -- the similarity and coarse-probe epilogues, the row writer and the
// row scan -- and the host launch of topk_select_kernel for the units that select rows they computed.
#pragma once
#include "common.h"
#include "wave_topk.h"

namespace tpq {

constexpr int kSelWaves = 4;

// a2 / b2 non-null: the coarse-probe epilogue of metric.negative_squared_l2_distance
// (torchpq/metric.py:89-96) is applied on the fly -- v = (2*x - a2[row]) - b2[col], the reference's
// order of roundings -- so the three element-wise passes over the [nq, n_cells] GEMM output vanish.
// Optional coarse-probe epilogue (tpq_ivfpq_coarse_probe): the selected columns are cells, so the
// same wave also gathers their list extents (IVFPQIndex.search_cells, index/IVFPQIndex.py:425-426)
// and derives the per-query probe count (smart probing :499-512, or all of them).
// Optional two-level select: gmax[row][g] = max of the row over columns [128 g, 128 g + 128) (written
// by coarse_sims_kernel).  The k-th largest group maximum is a lower bound of the k-th largest
// element (the k largest group maxima are k distinct elements), so only groups whose maximum
// reaches it can hold a member of the top-k: with n_probe = 8 of 16 384 cells the row select reads
// ~8 % of the row.  The result is the same total order (value desc, column asc) as the full scan.
struct GroupFilter {
  const float* gmax;  // [rows][n_groups]; nullptr = scan every column
  int n_groups;
};

struct ProbeEpilogue {
  const int64_t* cell_start_tbl;  // [cols]; nullptr = no epilogue
  const int64_t* cell_size_tbl;
  int64_t* out_cell_start;        // [rows][k]
  int64_t* out_cell_size;
  int64_t* n_probe_list;          // [rows]
  float inv_t;                    // 1 / temperature; <= 0: n_probe_list = k
};

// The similarity of a (query, centroid) pair from their dot product and squared norms, in the reference's order of
// roundings (metric.negative_squared_l2_distance, torchpq/metric.py:89-96): every kernel that produces a coarse
// similarity goes through here, which is what makes them agree bit for bit.
__device__ __forceinline__ float neg_sq_l2(float dot, float q2, float c2) {
  float v = 2.f * dot;
  v = v - q2;
  v = v - c2;
  return v;
}

// the selected row: values, columns and -- coarse probe -- the cells' extents and the probe count
template <int R>
__device__ __forceinline__ void write_row(const WaveTopK<R>& top, float* __restrict__ vals, int64_t* __restrict__ idx,
                                          int row, int k, const ProbeEpilogue& pe) {
  const int lane = lane_id();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = r * 64 + lane;
    if (e < k) {
      const int ci = key_index(top.k[r]);
      const bool pad = ci == kPadIdx;
      vals[(int64_t)row * k + e] = pad ? -INFINITY : key_value(top.k[r]);
      idx[(int64_t)row * k + e] = pad ? -1 : (int64_t)ci;
      if (pe.cell_start_tbl) {
        pe.out_cell_start[(int64_t)row * k + e] = pad ? 0 : pe.cell_start_tbl[ci];
        pe.out_cell_size[(int64_t)row * k + e] = pad ? 0 : pe.cell_size_tbl[ci];
      }
    }
  }
  if (!pe.cell_start_tbl) return;
  if (!(pe.inv_t > 0.f) || k < 2) {
    if (lane == 0) pe.n_probe_list[row] = k;
    return;
  }
  // smart probing on the register-resident sims: element e = r*64 + lane, the assignment (and so
  // the summation order) of smart_probing_kernel (select.hip)
  float zmax = -INFINITY;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r * 64 + lane < k) zmax = fmaxf(zmax, -sqrtf(fabsf(key_value(top.k[r]))) * pe.inv_t);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) zmax = fmaxf(zmax, __shfl_xor(zmax, d, 64));
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r * 64 + lane < k) sum += expf(-sqrtf(fabsf(key_value(top.k[r]))) * pe.inv_t - zmax);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
  const float inv_log = 1.0f / log2f((float)k);
  float h = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r * 64 + lane < k) {
      const float p = expf(-sqrtf(fabsf(key_value(top.k[r]))) * pe.inv_t - zmax) / sum;
      if (p > 0.f) h -= p * log2f(p) * inv_log;
    }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) h += __shfl_xor(h, d, 64);
  if (lane == 0) {
    long long n = (long long)ceilf(h * (float)k);
    n = n < 1 ? 1 : (n > k ? k : n);
    pe.n_probe_list[row] = n;
  }
}

// one wave selects row `row` (its values at xr[0 .. cols), global memory or LDS) -- the body of
// topk_select_kernel and of probe_small_kernel
template <int R>
__device__ __forceinline__ void select_row(float* qvw, int* qiw, const float* xr, const float* __restrict__ a2,
                                           const float* __restrict__ b2, float* __restrict__ vals,
                                           int64_t* __restrict__ idx, int row, int cols, int k,
                                           const ProbeEpilogue& pe, const GroupFilter& gf) {
  const int lane = lane_id();
  WaveSelector<R> sel;
  sel.init(qvw, qiw, k);
  const float ra2 = a2 ? a2[row] : 0.f;
  if (gf.gmax) {
    // phase 1: the k-th largest group maximum
    const float* __restrict__ gm = gf.gmax + (int64_t)row * gf.n_groups;
    for (int base = 0; base < gf.n_groups; base += 64) {
      const int g = base + lane;
      const float v = g < gf.n_groups ? gm[g] + 0.0f : -INFINITY;
      sel.push(g < gf.n_groups && (v >= sel.tau), v, g);
    }
    sel.flush();
    const float tau0 = sel.top.kth_value(k);  // -inf while there are fewer than k groups
    sel.init(qvw, qiw, k);
    // phase 2: only the groups that can hold a member of the top-k, four (eight loads) at a time
    for (int base = 0; base < gf.n_groups; base += 64) {
      const int g = base + lane;
      const bool hot = g < gf.n_groups && (gm[g] >= tau0);
      unsigned long long mask = __ballot(hot);
      while (mask != 0ull) {
        int gs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          gs[u] = -1;
          if (mask != 0ull) {
            gs[u] = base + (int)__builtin_ctzll(mask);
            mask &= mask - 1ull;
          }
        }
        float va[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int c = gs[u >> 1] * 128 + 64 * (u & 1) + lane;
          va[u] = (gs[u >> 1] >= 0 && c < cols) ? xr[c] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (gs[u >> 1] >= 0) {  // wave-uniform
            const int c = gs[u >> 1] * 128 + 64 * (u & 1) + lane;
            const bool valid = c < cols;
            const float v = va[u] + 0.0f;
            sel.push(valid && (v >= sel.tau), v, c);
          }
        }
      }
    }
  } else {
    // kSelAhead 64-column groups are loaded before any of them is pushed: with one load per
    // iteration a wave waits out a full memory latency per 256 bytes (1.9 TB/s on a
    // [10 000 x 16 384] matrix); 16 waves x 4 KiB in flight per CU cover the latency
    constexpr int kSelAhead = 16;
    for (int base = 0; base < cols; base += 64 * kSelAhead) {
      float va[kSelAhead];
  #pragma unroll
      for (int u = 0; u < kSelAhead; ++u) {
        const int c = base + 64 * u + lane;
        va[u] = c < cols ? xr[c] : -INFINITY;
      }
  #pragma unroll
      for (int u = 0; u < kSelAhead; ++u) {
        const int c = base + 64 * u + lane;
        if (base + 64 * u < cols) {  // wave-uniform
          const bool valid = c < cols;
          float v = va[u];
          if (valid) {
            if (a2) v = neg_sq_l2(v, ra2, b2[c]);
            v = v + 0.0f;  // -0.0 -> +0.0 (key order)
          }
          sel.push(valid && (v >= sel.tau), v, c);
        }
      }
    }
  }
  sel.flush();
  write_row<R>(sel.top, vals, idx, row, k, pe);
}

// Launches topk_select_kernel (select.hip) on x [rows][cols]: the k best of every row, with the epilogues above.
int launch_row_select(const float* x, const float* a2, const float* b2, float* vals, int64_t* idx, int rows, int cols,
                      int k, tpq_stream_t stream, const ProbeEpilogue& pe, const GroupFilter& gf);

}  // namespace tpq
