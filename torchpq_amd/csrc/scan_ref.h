// IVF list scan: the reference-layout kernels (exact; plain and residual PQ) and their split merge.  scan.hip and scan_flat.hip (the merge) only.
#pragma once
#include "scan_shared.h"

namespace tpq {

// ---- reference-layout kernel ---------------------------------------------------------------

template <int R>
__global__ __launch_bounds__(kScanThreads) void scan_ref_kernel(ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lut_bytes = a.m * 1024;
  const int list_bytes = kScanWaves * R * 64 * 8;
  const int region0 = lut_bytes > list_bytes ? lut_bytes : list_bytes;
  float* lut = reinterpret_cast<float*>(smem);
  float* qv_all = reinterpret_cast<float*>(smem + region0);
  int* qi_all = reinterpret_cast<int*>(smem + region0 + kScanWaves * 256);
  int* ptab = reinterpret_cast<int*>(smem + region0 + kScanWaves * 512);
  ProbeTable tab{ptab, ptab + a.max_nprobe, ptab + 2 * a.max_nprobe};
  unsigned* tau_key = reinterpret_cast<unsigned*>(ptab + 3 * a.max_nprobe + 1);
  float* xq = reinterpret_cast<float*>(tau_key + 1);  // fused LUT: query [m*ds], then |q_j|^2 [m]

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  if (a.only_flagged && a.only_flagged[q] != a.epoch) return;  // exact redo of flagged queries only
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  int n_probe = (int)a.n_probe_list[q];
  n_probe = n_probe < 0 ? 0 : (n_probe > a.max_nprobe ? a.max_nprobe : n_probe);

  if (wave == 0) {
    build_probe_table(a, q, n_probe, tab);
    if (lane == 0) *tau_key = f2key(-INFINITY);
  }
  if (!a.lut) stage_query(a, q, xq, kScanThreads);
  stage_lut_linear(a, q, lut, xq);
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(qv_all + wave * 64, qi_all + wave * 64, a.k);

  const int total_tiles = tab.tile_begin[n_probe];
  const int t_begin = (int)(((int64_t)total_tiles * part) / a.n_split);
  const int t_end = (int)(((int64_t)total_tiles * (part + 1)) / a.n_split);
  const int G = a.m >> 2;
  const uint32_t* __restrict__ codes32 = reinterpret_cast<const uint32_t*>(a.codes);

  int p = 0;
  for (int T = t_begin + wave; T < t_end; T += kScanWaves) {
    while (T >= tab.tile_begin[p + 1]) ++p;
    const int off = ((T - tab.tile_begin[p]) << 6) + lane;
    const bool valid = off < tab.size[p];
    const int s = tab.start[p] + off;
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
    // workgroup-shared admission threshold: any wave's k-th best bounds the final k-th best
    const float tau_s = key2f(lds_poll_u32(tau_key));
    sel.tau = fmaxf(sel.tau, tau_s);
    const float tau_before = sel.tau;
    sel.push(live && (v >= sel.tau), v, s);
    if (sel.tau > tau_before && lane == 0) atomicMax(tau_key, f2key(sel.tau));
  }
  {
    const float tau_before = sel.tau;
    sel.flush();
    if (sel.tau > tau_before && lane == 0) atomicMax(tau_key, f2key(sel.tau));
  }
  finish_query<R>(a, q, part, sel.top, reinterpret_cast<float*>(smem),
                  reinterpret_cast<int*>(smem + kScanWaves * R * 64 * 4));
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
// (:973-1037).  The LUT depends on the probed cell: LUT_p = part1[q] + part2[cell] (one fp32 add
// per entry, load_precomputed_v3 :522-560) or LUT_p = full[q][p]; value(slot) starts at
// base_sims[q][p] (:1113) and adds LUT_p[j][code_j] in ascending j.  One workgroup per query
// walks its probes in order: barrier, rebuild the 64-KiB LUT in LDS, barrier, the 8 waves scan
// the cell's tiles; the per-wave register top-k and shared threshold carry across cells.

template <int R>
__global__ __launch_bounds__(kScanThreads) void scan_residual_kernel(ScanArgs a, ResidualArgs ra) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lut_bytes = a.m * 1024;
  const int list_bytes = kScanWaves * R * 64 * 8;
  const int region0 = lut_bytes > list_bytes ? lut_bytes : list_bytes;
  float* lut = reinterpret_cast<float*>(smem);
  float* qv_all = reinterpret_cast<float*>(smem + region0);
  int* qi_all = reinterpret_cast<int*>(smem + region0 + kScanWaves * 256);
  int* ptab = reinterpret_cast<int*>(smem + region0 + kScanWaves * 512);
  ProbeTable tab{ptab, ptab + a.max_nprobe, ptab + 2 * a.max_nprobe};
  unsigned* tau_key = reinterpret_cast<unsigned*>(ptab + 3 * a.max_nprobe + 1);

  float* xq = reinterpret_cast<float*>(tau_key + 1);  // part1 built here: query [m*ds], |q_j|^2 [m]

  const int q = blockIdx.x;
  if (a.only_flagged && a.only_flagged[q] != a.epoch) return;  // exact redo of flagged queries only
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  int n_probe = (int)a.n_probe_list[q];
  n_probe = n_probe < 0 ? 0 : (n_probe > a.max_nprobe ? a.max_nprobe : n_probe);
  if (wave == 0) {
    build_probe_table(a, q, n_probe, tab);
    if (lane == 0) *tau_key = f2key(-INFINITY);
  }
  const bool build_part1 = !ra.full && !ra.part1;
  if (build_part1) stage_query(a, q, xq, kScanThreads);
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(qv_all + wave * 64, qi_all + wave * 64, a.k);
  const int G = a.m >> 2;
  const uint32_t* __restrict__ codes32 = reinterpret_cast<const uint32_t*>(a.codes);
  const int n4 = a.m * 64;  // float4 count of one LUT

  for (int p = 0; p < n_probe; ++p) {
    const int sz = tab.size[p];
    if (sz == 0) continue;  // empty, or same start as the previous probe (ivfpq_topk.cu:1092-1107)
    __syncthreads();        // every wave is done with the previous cell's LUT
    float4* dst = reinterpret_cast<float4*>(lut);
    if (ra.full) {
      const float4* __restrict__ src =
          reinterpret_cast<const float4*>(ra.full) + ((int64_t)q * a.max_nprobe + p) * n4;
      for (int i = threadIdx.x; i < n4; i += kScanThreads) dst[i] = src[i];
    } else {
      const float4* __restrict__ s1 = reinterpret_cast<const float4*>(ra.part1) + (int64_t)q * n4;
      const float4* __restrict__ s2 = reinterpret_cast<const float4*>(ra.part2) +
                                      ra.cells[(int64_t)q * a.max_nprobe + p] * (int64_t)n4;
      for (int i = threadIdx.x; i < n4; i += kScanThreads) {
        const float4 x = build_part1 ? fused_lut4(a, i >> 6, i & 63, xq) : s1[i];
        const float4 y = s2[i];
        dst[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
      }
    }
    __syncthreads();
    const float base = ra.base_sims[(int64_t)q * a.max_nprobe + p];
    const int start = tab.start[p];
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
          const float* row = lut + g * 1024;
          v += row[w & 255u];
          v += row[256 + ((w >> 8) & 255u)];
          v += row[512 + ((w >> 16) & 255u)];
          v += row[768 + (w >> 24)];
        }
      }
      const float tau_s = key2f(lds_poll_u32(tau_key));
      sel.tau = fmaxf(sel.tau, tau_s);
      const float tau_before = sel.tau;
      sel.push(live && (v >= sel.tau), v + 0.0f, s);
      if (sel.tau > tau_before && lane == 0) atomicMax(tau_key, f2key(sel.tau));
    }
  }
  sel.flush();
  finish_query<R>(a, q, 0, sel.top, reinterpret_cast<float*>(smem),
                  reinterpret_cast<int*>(smem + kScanWaves * R * 64 * 4));
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
