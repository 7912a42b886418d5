// The coarse step of search() (tpq_ivfpq_coarse_probe*): similarities of every (query, cell) pair and the n_probe best
// cells of every query, in fp32 -- the one-block small-batch kernel, or the MFMA similarity kernels + the row select
// (row_select.h) -- or selected on the fp16 matrix cores (probe_fast.h, probe_sims.hip).  Results are the same bits on
// every route.
#include "mfma_util.h"
#include "probe_fast.h"
#include "row_select.h"
#include "sims_chunk.h"

namespace tpq {

// Small batches (tpq_ivfpq_coarse_probe, nq <= kProbeSmallMaxQ): the whole coarse step of a query in ONE
// block -- its sims row computed into LDS, selected by wave 0 -- instead of the sims kernel + the select
// kernel (at one query the launch gaps and the second kernel's start-up are most of the 28 us).
// One thread per cell: dot, |C|^2 and (every thread) |x|^2 as ascending-k fmaf chains, v = (2 dot - |x|^2)
// - |C|^2: the arithmetic of coarse_sims_kernel and oracle_coarse_sims, bit for bit.  The chains are
// sequential in k, the loads are not: 16 in flight per thread.
constexpr int kProbeSmallThreads = 1024;
constexpr int kProbeSmallMaxQ = 256;
constexpr int kProbeSmallMaxCells = 8192;   // sims row in LDS (32 KiB)
constexpr int kProbeSmallMaxD = 1024;       // query in LDS

template <int R>
__global__ __launch_bounds__(kProbeSmallThreads) void probe_small_kernel(const float* __restrict__ x,
                                                                        const float* __restrict__ C,
                                                                        float* __restrict__ vals,
                                                                        int64_t* __restrict__ idx, int d, int nq,
                                                                        int n_cells, int k, ProbeEpilogue pe) {
  __shared__ float row_s[kProbeSmallMaxCells];
  __shared__ float xq[kProbeSmallMaxD];
  __shared__ float qv[64];
  __shared__ int qi[64];
  const int q = blockIdx.x;
  for (int t = threadIdx.x; t < d; t += kProbeSmallThreads) xq[t] = x[(int64_t)t * nq + q];
  __syncthreads();
  float q2 = 0.f;
  for (int t = 0; t < d; ++t) q2 = fmaf(xq[t], xq[t], q2);
  for (int c = threadIdx.x; c < n_cells; c += kProbeSmallThreads) {
    const float* __restrict__ p = C + c;
    float acc = 0.f, c2 = 0.f;
    int t = 0;
    // 64 loads in flight per thread (the chains are sequential in k, the loads are not): at one query
    // the block is alone on the chip and the 512 KiB of centroids come from L2 / the Infinity Cache --
    // with 16 in flight the eight round trips were most of the kernel's 30 us
    for (; t + 64 <= d; t += 64) {
      float y[64];
#pragma unroll
      for (int u = 0; u < 64; ++u) y[u] = p[(int64_t)(t + u) * n_cells];
#pragma unroll
      for (int u = 0; u < 64; ++u) {
        acc = fmaf(y[u], xq[t + u], acc);
        c2 = fmaf(y[u], y[u], c2);
      }
    }
    for (; t + 16 <= d; t += 16) {
      float y[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) y[u] = p[(int64_t)(t + u) * n_cells];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        acc = fmaf(y[u], xq[t + u], acc);
        c2 = fmaf(y[u], y[u], c2);
      }
    }
    for (; t < d; ++t) {
      const float y = p[(int64_t)t * n_cells];
      acc = fmaf(y, xq[t], acc);
      c2 = fmaf(y, y, c2);
    }
    row_s[c] = neg_sq_l2(acc, q2, c2);
  }
  __syncthreads();
  if (threadIdx.x < 64) select_row<R>(qv, qi, row_s, nullptr, nullptr, vals, idx, q, n_cells, k, pe, GroupFilter{nullptr, 0});
}

// Coarse similarities sims[q][c] = 2 x_q.C_c - |x_q|^2 - |C_c|^2 (metric.negative_squared_l2_distance,
// torchpq/metric.py:31-98: library GEMM + three element-wise passes) as one fp32-MFMA kernel, built
// like max_sim_kernel (max_sim.hip): a block owns 128 QUERIES (4 waves x 32 MFMA columns, operand
// in registers, prefetched one k-slab ahead) and walks centroid chunks of 256 MFMA rows whose
// 16-row k-slabs are double-buffered in LDS (global -> registers while the previous slab's 8 x 8
// MFMAs run -> the other buffer, one barrier per slab).  |C|^2 is accumulated from the values each
// thread stages (its centroid, every slab, ascending k), |x|^2 by each lane for its own query.
// With the queries on the lanes
//   * the maximum of a query's sims over a 128-centroid group is an in-lane reduction over
//     accumulator registers -> gmax[q][group], which lets the row select skip every group that
//     cannot hold a member of the top-n_probe (GroupFilter, row_select.h);
//   * a tile's sims leave through a 32 x 33 LDS transpose per wave, so that a half-wave still
//     stores 128 contiguous bytes of a sims row.
// In the reference's own benchmark grid (IVF4096 / IVF16384, n_probe 1..128) this step is 40-85 %
// of a search, not the scan.
// x [d][nq], C [d][n_cells] -> sims [nq][n_cells], gmax [nq][ceil(n_cells/128)]
// grid (ceil(nq/128), centroid-chunk groups)
__global__ __launch_bounds__(256, 2) void coarse_sims_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ C,
                                                            float* __restrict__ sims, int d, int nq,
                                                            int n_cells, int chunks_per_block,
                                                            float* __restrict__ gmax, int n_groups) {
  __shared__ float cs[2 * kCsSlab];   // [2][kCsKC][kCsRows]
  __shared__ float c2s[kCsRows];
  __shared__ float tr[4 * 32 * 33];   // per wave: 32 queries x (32 + 1) centroids
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int qw = blockIdx.x * 128 + wave * 32;   // first query of this wave
  const int q = qw + l31;                        // this lane's query
  const bool qvalid = q < nq;
  const float* __restrict__ xq = x + (qvalid ? q : 0);
  float* trw = tr + wave * 32 * 33;

  const float q2 = sims_query_sq_norm(xq, d, nq);

  const int chunk0 = blockIdx.y * chunks_per_block;
  for (int ch = chunk0; ch < chunk0 + chunks_per_block; ++ch) {
    const int c0 = ch * kCsRows;
    if (c0 >= n_cells) break;
    f32x16 acc[8];
    sims_chunk_mfma(xq, qvalid, C, c0, d, nq, n_cells, cs, c2s, acc, [](bool) {});
    // epilogue: acc[t][r] = (centroid row cl(t, r, half), query column l31)
    float gm[2] = {-INFINITY, -INFINITY};
    const int nq_w = nq - qw;  // queries of this wave that exist (may be <= 0)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cl = sims_tile_row(r, half);
        const float v = neg_sq_l2(acc[t][r], q2, c2s[t * 32 + cl]);
        gm[t >> 2] = fmaxf(gm[t >> 2], v);
        trw[l31 * 33 + cl] = v;                              // [query][centroid]
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      // read back transposed: lane (l31, half) takes centroid l31 of queries 16 half + i
      const int c = c0 + t * 32 + l31;
      if (c < n_cells) {
        float* __restrict__ out = sims + (int64_t)(qw + 16 * half) * n_cells + c;
        const int n_here = nq_w - 16 * half;  // rows of this half-wave that exist
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = trw[(16 * half + i) * 33 + l31];
          if (i < n_here) out[(int64_t)i * n_cells] = v;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_sched_barrier(0);  // one tile at a time: keeps the live predicate masks few
    }
    // the two half-waves of a query hold disjoint centroid rows
    gm[0] = fmaxf(gm[0], __shfl_xor(gm[0], 32, 64));
    gm[1] = fmaxf(gm[1], __shfl_xor(gm[1], 32, 64));
    if (half == 0 && qvalid) {
      const int g0 = 2 * ch;
      gmax[(int64_t)q * n_groups + g0] = gm[0];
      if (g0 + 1 < n_groups) gmax[(int64_t)q * n_groups + g0 + 1] = gm[1];
    }
  }
}

// Small problems (few centroid groups x query chunks): 64-query x (64 CT)-centroid tiles, both
// operands through LDS in double-buffered k-batches of 16.  CT = 4 (256 centroids per block): twice
// the blocks of the kernel above; CT = 1 (64 centroids): eight times -- a 1000-query GIST batch
// (d = 960, 1024 cells) is 64 blocks at CT = 4, a quarter of the chip each walking 960 dimensions,
// and 256 at CT = 1.
constexpr int kCsKB = 16;

template <int CT>
__global__ __launch_bounds__(256) void coarse_sims_small_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ C,
                                                         float* __restrict__ sims, int d, int nq,
                                                         int n_cells) {
  constexpr int W = 64 * CT;  // centroids per block: 2 wave columns x CT tiles x 32
  __shared__ float As[2][kCsKB][64];
  __shared__ float Bs[2][kCsKB][W];
  __shared__ float q2s[64];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int qb = blockIdx.x * 64, cb = blockIdx.y * W;
  const int wq = 32 * (wave & 1), wc = 32 * CT * (wave >> 1);

  // staging: A batch = 16 rows x 64 queries (4 elements per thread), B batch = 16 rows x W
  // centroids (4 CT per thread); a thread's elements of one row are contiguous across the wave
  const int a_col = tid & 63, a_row0 = tid >> 6;  // rows a_row0 + 4u
  const bool a_ok = qb + a_col < nq;
  constexpr int BR = 256 / W;                     // B rows covered by one pass of the block (1 or 4)
  const int b_col = tid % W, b_row0 = tid / W;    // rows b_row0 + BR u
  const bool b_ok = cb + b_col < n_cells;
  const float* __restrict__ xa = x + (a_ok ? qb + a_col : 0);
  const float* __restrict__ cbp = C + (b_ok ? cb + b_col : 0);
  float ra[4], rb[kCsKB / BR];
  auto load_batch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + a_row0 + 4 * u;
      ra[u] = (a_ok && k < d) ? xa[(int64_t)k * nq] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kCsKB / BR; ++u) {
      const int k = k0 + b_row0 + BR * u;
      rb[u] = (b_ok && k < d) ? cbp[(int64_t)k * n_cells] : 0.f;
    }
  };
  auto store_batch = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) As[buf][a_row0 + 4 * u][a_col] = ra[u];
#pragma unroll
    for (int u = 0; u < kCsKB / BR; ++u) Bs[buf][b_row0 + BR * u][b_col] = rb[u];
  };

  f32x16 acc[CT];
  float b2[CT], a2 = 0.f;
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    b2[t] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  }
  const int n_batches = (d + kCsKB - 1) / kCsKB;
  load_batch(0);
  store_batch(0);
  __syncthreads();
  for (int bt = 0; bt < n_batches; ++bt) {
    const int buf = bt & 1;
    if (bt + 1 < n_batches) load_batch((bt + 1) * kCsKB);
#pragma unroll
    for (int kk = 0; kk < kCsKB / 2; ++kk) {
      // both k rows of the step in every lane: the norms are ONE ascending-k fmaf chain, the same
      // arithmetic as coarse_sims_kernel (and oracle_coarse_sims) -- a sim does not depend on
      // which of the kernels the batch size selects.  (Even / odd partial chains added at the end
      // differed from it in the last bit.)
      const float a0 = As[buf][2 * kk][wq + l31], a1 = As[buf][2 * kk + 1][wq + l31];
      a2 = fmaf(a0, a0, a2);
      a2 = fmaf(a1, a1, a2);
      const float a = half ? a1 : a0;
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const float b0 = Bs[buf][2 * kk][wc + 32 * t + l31], b1 = Bs[buf][2 * kk + 1][wc + 32 * t + l31];
        b2[t] = fmaf(b0, b0, b2[t]);
        b2[t] = fmaf(b1, b1, b2[t]);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, half ? b1 : b0, acc[t], 0, 0, 0);
      }
    }
    if (bt + 1 < n_batches) store_batch(buf ^ 1);
    __syncthreads();
  }
  if (wave < 2 && half == 0) q2s[32 * wave + l31] = a2;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int c = cb + wc + 32 * t + l31;
    if (c >= n_cells) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int qq = qb + wq + row;
      if (qq < nq) {
        float v = 2.f * acc[t][r];  // neg_sq_l2 (row_select.h), written out: the call changes this kernel's registers
        v = v - q2s[wq + row];
        v = v - b2[t];
        sims[(int64_t)qq * n_cells + c] = v;
      }
    }
  }
}

// Which arithmetic selects (results are the same either way, bit for bit):
//   TPQ_PROBE_ROUTE_AUTO   the fp16 selection pass + exact candidates where the fp32 similarity GEMM dominates the coarse
//                          step -- from kProbeFastMinCells = 2 048 cells on for batches beyond kProbeSmallMaxQ = 256
//                          queries (up to 112 probes, or 2 n_probe <= groups of cells), and from 1 024 cells on for
//                          batches of 4 096 queries or more with up to 32 probes --; the fp32 kernels above elsewhere
//   TPQ_PROBE_ROUTE_FP32   the fp32-MFMA similarity kernels always
//   TPQ_PROBE_ROUTE_FP16   the fp16 selection pass whenever the shape supports it (use_tensor_core=True)
constexpr int kProbeFastMinCells = 2048;
static bool probe_fast_route(int d, int nq, int n_cells, int n_probe, int route) {
  if (route == TPQ_PROBE_ROUTE_FP32 || !lloyd_probe_supported(d, nq, n_cells)) return false;
  if (n_probe + 16 > 1024) return false;  // (the candidate list: 64 R >= n_probe + 16 entries, R <= 16)
  if (route == TPQ_PROBE_ROUTE_FP16) return true;
  // (beyond 112 probes the candidate list takes four registers per lane and the fast select's folds cost more than
  // the fp32 GEMM saves: 16 384 cells, 128 probes: 1.15 ms against 0.83; 64 probes: 0.38 against 0.67)
  // ... unless the direct candidate list applies (2 n_probe <= groups of cells: 16 384 cells in 256 groups, 128 probes:
  // 0.41 ms against 0.77)
  if (n_cells >= kProbeFastMinCells)
    return nq > kProbeSmallMaxQ && (n_probe <= 112 || 2 * n_probe <= lloyd_probe_groups(n_cells));
  // (1 024 cells, 10 000 queries: 0.054-0.079 ms against 0.082-0.090 up to 32 probes; 1 000 queries: 0.035 against 0.025)
  return n_cells >= 1024 && nq >= 4096 && n_probe <= 32;
}

static size_t probe_fp32_workspace_bytes(int nq, int n_cells) {
  // sims [nq][n_cells] + group maxima [nq][ceil(n_cells / 128)]
  return ((size_t)nq * (size_t)n_cells + (size_t)nq * (size_t)((n_cells + 127) / 128)) * sizeof(float);
}

}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq_coarse_probe_route_workspace_bytes(int d, int nq, int n_cells, int route) {
  if (nq <= 0 || n_cells <= 0) return 0;
  const size_t plain = probe_fp32_workspace_bytes(nq, n_cells);
  if (route == TPQ_PROBE_ROUTE_FP32 || !lloyd_probe_supported(d, nq, n_cells)) return plain;
  const size_t fast = lloyd_probe_workspace_bytes(d, nq, n_cells);
  return fast > plain ? fast : plain;
}
extern "C" size_t tpq_ivfpq_coarse_probe_workspace_bytes(int nq, int n_cells) {
  if (nq <= 0 || n_cells <= 0) return 0;
  return tpq_ivfpq_coarse_probe_route_workspace_bytes(128, nq, n_cells, TPQ_PROBE_ROUTE_AUTO);  // (covers every d <= 128)
}

extern "C" size_t tpq_ivfpq_coarse_probe_prepared_bytes(int d, int n_cells) {
  return lloyd_probe_prepared_bytes(d, n_cells);
}
extern "C" int tpq_ivfpq_coarse_probe_prepare(const float* centroids, int d, int n_cells, void* prepared,
                                              size_t prepared_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(centroids && prepared, "ivfpq_coarse_probe_prepare: null pointer");
  const size_t need = lloyd_probe_prepared_bytes(d, n_cells);
  if (need == 0) {
    set_error("ivfpq_coarse_probe_prepare: shape d=%d n_cells=%d has no fp16 selection pass (d <= 128, n_cells %% 32 == 0)",
              d, n_cells);
    return TPQ_ERR_UNSUPPORTED;
  }
  TPQ_REQUIRE(prepared_bytes >= need, "ivfpq_coarse_probe_prepare: prepared block of %zu bytes needed", need);
  return lloyd_probe_prepare(centroids, d, n_cells, reinterpret_cast<char*>(prepared), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int tpq_ivfpq_coarse_probe(const float* query, const float* centroids,
                                      const int64_t* cell_start_tbl, const int64_t* cell_size_tbl,
                                      float* topk_sims, int64_t* cells, int64_t* cell_start,
                                      int64_t* cell_size, int64_t* n_probe_list, int d, int nq,
                                      int n_cells, int n_probe, float smart_temperature,
                                      void* workspace, size_t workspace_bytes,
                                      tpq_stream_t stream) {
  return tpq_ivfpq_coarse_probe_route(query, centroids, cell_start_tbl, cell_size_tbl, topk_sims, cells, cell_start,
                                      cell_size, n_probe_list, d, nq, n_cells, n_probe, smart_temperature,
                                      TPQ_PROBE_ROUTE_AUTO, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int tpq_ivfpq_coarse_probe_route(const float* query, const float* centroids,
                                            const int64_t* cell_start_tbl, const int64_t* cell_size_tbl,
                                            float* topk_sims, int64_t* cells, int64_t* cell_start,
                                            int64_t* cell_size, int64_t* n_probe_list, int d, int nq,
                                            int n_cells, int n_probe, float smart_temperature, int route,
                                            const void* prepared, void* workspace, size_t workspace_bytes,
                                            tpq_stream_t stream) {
  TPQ_REQUIRE(route == TPQ_PROBE_ROUTE_AUTO || route == TPQ_PROBE_ROUTE_FP32 || route == TPQ_PROBE_ROUTE_FP16,
              "ivfpq_coarse_probe: bad route %d", route);
  TPQ_REQUIRE(query && centroids && cell_start_tbl && cell_size_tbl && topk_sims && cells &&
                  cell_start && cell_size && n_probe_list,
              "ivfpq_coarse_probe: null pointer argument");
  TPQ_REQUIRE(d >= 1 && nq >= 0 && n_cells >= 1, "ivfpq_coarse_probe: bad shape d=%d nq=%d n_cells=%d",
              d, nq, n_cells);
  TPQ_REQUIRE(n_probe >= 1 && n_probe <= n_cells && n_probe <= 1024,
              "ivfpq_coarse_probe: n_probe=%d out of range (n_cells=%d, max 1024)", n_probe, n_cells);
  if (nq == 0) return TPQ_OK;
  const size_t need = tpq_ivfpq_coarse_probe_route_workspace_bytes(d, nq, n_cells, route);
  if (!workspace || workspace_bytes < need) {
    set_error("ivfpq_coarse_probe: workspace too small (%zu < %zu)", workspace_bytes, need);
    return TPQ_ERR_WORKSPACE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const ProbeEpilogue pe{cell_start_tbl, cell_size_tbl, cell_start, cell_size, n_probe_list,
                         smart_temperature > 0.f ? 1.0f / smart_temperature : 0.f};
  if (probe_fast_route(d, nq, n_cells, n_probe, route))
    return lloyd_probe_select(query, centroids, prepared, d, nq, n_cells, n_probe, topk_sims, cells, pe,
                              reinterpret_cast<char*>(workspace), st);
  if (nq <= kProbeSmallMaxQ && n_cells <= kProbeSmallMaxCells && d <= kProbeSmallMaxD &&
      (long long)n_cells * d <= (1 << 20)) {  // one launch: sims row in LDS + select, one block per query
    with_list_regs(list_regs(n_probe), [&](auto r_c) {
      hipLaunchKernelGGL(probe_small_kernel<decltype(r_c)::value>, dim3(nq), dim3(kProbeSmallThreads), 0, st, query,
                         centroids, topk_sims, cells, d, nq, n_cells, n_probe, pe);
    });
    TPQ_LAUNCH_CHECK("probe_small_kernel");
    return TPQ_OK;
  }
  // large problems: blocks = 128-query groups x centroid-chunk groups (a block walks several
  // 256-centroid chunks once there are enough blocks to fill the chip a few times over) and the
  // row select is restricted by the group maxima; small ones: 64 x 256 tiles, full row select
  const int qgroups = (nq + 127) / 128, chunks = (n_cells + kCsRows - 1) / kCsRows;
  const int n_groups = (n_cells + 127) / 128;
  float* sims = reinterpret_cast<float*>(workspace);
  float* gmax = sims + (size_t)nq * n_cells;
  GroupFilter gf{nullptr, 0};
  if ((long long)qgroups * chunks < 512) {
    const long long blocks4 = (long long)((nq + 63) / 64) * ((n_cells + 255) / 256);
    if (blocks4 < 192)  // under three quarters of the CUs: 64-centroid tiles, 4x the blocks
      hipLaunchKernelGGL(coarse_sims_small_kernel<1>, dim3((nq + 63) / 64, (n_cells + 63) / 64),
                         dim3(256), 0, st, query, centroids, sims, d, nq, n_cells);
    else
      hipLaunchKernelGGL(coarse_sims_small_kernel<4>, dim3((nq + 63) / 64, (n_cells + 255) / 256),
                         dim3(256), 0, st, query, centroids, sims, d, nq, n_cells);
  } else {
    int per_block = (int)(((long long)qgroups * chunks) / 1024);
    per_block = per_block < 1 ? 1 : (per_block > 8 ? 8 : per_block);
    hipLaunchKernelGGL(coarse_sims_kernel, dim3(qgroups, (chunks + per_block - 1) / per_block),
                       dim3(256), 0, st, query, centroids, sims, d, nq, n_cells, per_block, gmax, n_groups);
    gf = GroupFilter{gmax, n_groups};
  }
  TPQ_LAUNCH_CHECK("coarse_sims_kernel");
  return launch_row_select(sims, nullptr, nullptr, topk_sims, cells, nq, n_cells, n_probe, stream, pe, gf);
}
