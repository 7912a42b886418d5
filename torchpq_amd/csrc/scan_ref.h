// IVF list scan: the reference-layout kernels (exact; plain and residual PQ) and their split merge.  scan.hip, and
// scan_flat.hip and scan_pq4.hip (the merge) only.
#pragma once
#include "scan_list.h"

namespace tpq {

// ---- reference-layout kernel ---------------------------------------------------------------

template <int R>
__global__ __launch_bounds__(kScanThreads) void scan_ref_kernel(ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ListLds lds(smem, list_region0(a.m * 1024, R), a.max_nprobe);
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(lds.tail);  // fused LUT: query [m*ds], then |q_j|^2 [m]

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  if (a.only_flagged && a.only_flagged[q] != a.epoch) return;  // exact redo of flagged queries only
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int n_probe = clamped_n_probe(a, q);

  lds.init(a, q, n_probe, wave, lane);
  if (!a.lut) stage_query(a, q, xq, kScanThreads);
  stage_lut_linear(a, q, lut, xq);
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);

  const TileRange t = part_tiles(lds.tab.tile_begin[n_probe], part, a.n_split);
  const int G = a.m >> 2;
  const uint32_t* __restrict__ codes32 = reinterpret_cast<const uint32_t*>(a.codes);

  int p = 0;
  for (int T = t.begin + wave; T < t.end; T += kScanWaves) {
    p = probe_of(lds.tab, p, T);
    // This kernel keeps two spots written out, because it compiles to other code through the shared forms: the tile's
    // three reads (tile_at reads the cell's start before its size) and the look-ups of a code word (lut_word).
    const int off = ((T - lds.tab.tile_begin[p]) << 6) + lane;
    const bool valid = off < lds.tab.size[p];  // (a cell that leaves the storage is NOT cut here)
    const int s = lds.tab.start[p] + off;
    float v = 0.f;
    bool live = valid;
    if (valid) {
      if (a.is_empty) live = (a.is_empty[s] == 0);  // ivfpq_topk.cu:878,883-884
      int g = 0;
      for (; g + 4 <= G; g += 4) {
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = codes32[(int64_t)(g + u) * a.n_slots + s];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* row = lut + (g + u) * 1024;
          v += row[w[u] & 255u];
          v += row[256 + ((w[u] >> 8) & 255u)];
          v += row[512 + ((w[u] >> 16) & 255u)];
          v += row[768 + (w[u] >> 24)];
        }
      }
      for (; g < G; ++g) {
        const uint32_t w = codes32[(int64_t)g * a.n_slots + s];
        const float* row = lut + g * 1024;
        v += row[w & 255u];
        v += row[256 + ((w >> 8) & 255u)];
        v += row[512 + ((w >> 16) & 255u)];
        v += row[768 + (w >> 24)];
      }
    }
    admit(sel, lds.tau_key, live, v, s);
  }
  {  // (this kernel alone publishes the threshold once more after the flush)
    const float tau_before = sel.tau;
    sel.flush();
    if (sel.tau > tau_before && lane == 0) atomicMax(lds.tau_key, f2key(sel.tau));
  }
  finish_list_scan<R>(a, q, part, sel.top, smem);
  // exact redo (one workgroup per query): the flag is consumed -- every thread read it before the first barrier.
  // (a captured graph replays with the same epoch: a flag left raised would redo the query on every replay)
  // Diagnostics: ws_delta[q] = kRedoneMark says "this query was redone exactly" -- on the routes whose
  // ws_delta holds a selection band the finisher's 1.f / 0.f never appears, so IVFPQTopkHip.last_redone reads this mark
  // (a band is >= 0; nobody reads ws_delta after this kernel, the call's last).
  if (a.only_flagged && threadIdx.x == 0) {
    const_cast<int*>(a.only_flagged)[q] = 0;
    if (a.ws_delta) a.ws_delta[q] = kRedoneMark;
  }
}

// ---- residual PQ (reference layout, exact) --------------------------------------------------
// Replaces ivfpq_topk_residual_precomputed (ivfpq_topk.cu:1039-1208) and ivfpq_topk_residual
// (:973-1037).  The LUT depends on the probed cell (build_residual_lut); value(slot) starts at
// base_sims[q][p] (:1113) and adds LUT_p[j][code_j] in ascending j.  One workgroup per query
// walks its probes in order: barrier, rebuild the 64-KiB LUT in LDS, barrier, the 8 waves scan
// the cell's tiles; the per-wave register top-k and shared threshold carry across cells.

template <int R>
__global__ __launch_bounds__(kScanThreads) void scan_residual_kernel(ScanArgs a, ResidualArgs ra) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ListLds lds(smem, list_region0(a.m * 1024, R), a.max_nprobe);
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(lds.tail);  // part1 built here: query [m*ds], |q_j|^2 [m]

  const int q = blockIdx.x;
  if (a.only_flagged && a.only_flagged[q] != a.epoch) return;  // exact redo of flagged queries only
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int n_probe = clamped_n_probe(a, q);
  lds.init(a, q, n_probe, wave, lane);
  const bool build_part1 = !ra.full && !ra.part1;
  if (build_part1) stage_query(a, q, xq, kScanThreads);
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);
  const int G = a.m >> 2;
  const uint32_t* __restrict__ codes32 = reinterpret_cast<const uint32_t*>(a.codes);

  for (int p = 0; p < n_probe; ++p) {
    const int sz = lds.tab.size[p];
    if (sz == 0) continue;  // empty, or same start as the previous probe (ivfpq_topk.cu:1092-1107)
    __syncthreads();        // every wave is done with the previous cell's LUT
    build_residual_lut(a, ra, q, p, lut, xq, build_part1);
    __syncthreads();
    const float base = ra.base_sims[(int64_t)q * a.max_nprobe + p];
    const int start = lds.tab.start[p];
    const int tiles = (sz + 63) >> 6;
    for (int t = wave; t < tiles; t += kScanWaves) {
      const int off = (t << 6) + lane;
      const bool valid = off < sz;
      const int s = start + off;
      float v = base;
      bool live = valid;
      if (valid) {
        if (a.is_empty) live = (a.is_empty[s] == 0);
        for (int g = 0; g < G; ++g) {
          const uint32_t w = codes32[(int64_t)g * a.n_slots + s];
          v = lut_word(v, lut + g * 1024, w);
        }
      }
      // the test is on the raw v, as ever (-0.f and +0.f compare alike); what enters is canonical: -0.f as +0.f
      admit(sel, lds.tau_key, live, v, s, v + 0.0f);
    }
  }
  sel.flush();
  finish_list_scan<R>(a, q, 0, sel.top, smem);
  if (a.only_flagged && threadIdx.x == 0) {  // consumed, and marked as redone (see scan_ref_kernel)
    const_cast<int*>(a.only_flagged)[q] = 0;
    if (a.ws_delta) a.ws_delta[q] = kRedoneMark;
  }
}

// ---- split merge ---------------------------------------------------------------------------

template <int R>
__global__ __launch_bounds__(64) void scan_merge_kernel(ScanArgs a) {
  const int q = blockIdx.x;
  if (a.only_flagged && a.only_flagged[q] != a.epoch) return;
  WaveTopK<R> top;
  top.init();
  for (int part = 0; part < a.n_split; ++part) {
    const int64_t o = ((int64_t)q * a.n_split + part) * (R * 64);
    merge_list<R>(top, a.ws_vals + o, a.ws_idx + o);
  }
  write_final<R>(a, q, top);
}

}  // namespace tpq
