// Range search over the lists of IVFPQIndex (tpq_ivfpq_range_count / _fill and their residual forms).
//
// Every candidate of the top-k scan whose value is >= the query's threshold, in scan order.  Candidates, values and
// order are those of the exact reference-layout kernels (scan_ref.h): the codes are read as CellContainer stores them,
// u8 [m/4][n_slots][4] -- a lane owns one slot of a 64-slot tile and reads one dword per row of four sub-quantizers,
// 256 contiguous bytes per wave and row, kRowGroup rows in flight -- and the value is the ascending-j fp32 sum of the
// look-up table in LDS.  Two passes over the same tiles, as for IVFFlatIndex (scan_flat.hip): the count pass counts
// each wave's hits, the caller turns the counts into offsets, the fill pass computes the values again -- the same
// code, so the same bits -- and appends each wave's hits at its offset.  No global atomic, no sort, no selection.
//
//   plain PQ     one workgroup per (query, part); the query's table is staged once (a caller's table, or built from
//                query and codebook: stage_lut_linear / fused_lut4), the part's tiles are scan_ref_kernel's, and inside
//                the part a wave owns a CONTIGUOUS chunk of them: segment (q * n_split + part) * 8 + wave.
//   residual PQ  the table depends on the probed cell, so the work is cut by probe: one workgroup per (query, probe
//                rank) builds LUT_p as scan_residual_kernel does and its waves take contiguous chunks of that cell's
//                tiles: segment (q * max_nprobe + p) * 8 + wave.  A probe that is not scanned costs eight zero counts.
//
// LDS: the m KiB table, the staged query when the table is built here, the probe table (plain).  Nothing else: no
// candidate lists, no shared threshold, no barrier after staging.
#include "scan_list.h"

namespace tpq {
namespace pqrange {

// LDS: [table m KiB][query m * ds floats, when the table is built in the workgroup][probe table, plain only]
__host__ __device__ constexpr size_t query_bytes(int m, int ds) { return align16((size_t)m * ds * 4); }
static size_t lds_bytes(int m, int ds_staged, int probe_entries) {
  return (size_t)m * 1024 + query_bytes(m, ds_staged) + (probe_entries ? probe_table_bytes(probe_entries) : 0);
}

constexpr int kRowGroup = 4;  // row loads in flight per lane, as scan_ref_kernel's group

// The value of scan_ref_kernel / scan_residual_kernel: v starts at `v` (0.f, or the probe's base similarity) and adds
// lut[j][code_j] for j ascending, one fp32 add each.  `col` is the slot's dword of row 0, rows are `stride` dwords apart.
// (The look-ups stay written out, as in scan_ref_kernel: see lut_word, scan_list.h.)
__device__ __forceinline__ float slot_value(const uint32_t* __restrict__ col, int64_t stride, const float* lut, int G,
                                            float v) {
  int g = 0;
  for (; g + kRowGroup <= G; g += kRowGroup) {
    uint32_t w[kRowGroup];
#pragma unroll
    for (int u = 0; u < kRowGroup; ++u) w[u] = col[(int64_t)u * stride];
    col += (int64_t)kRowGroup * stride;
#pragma unroll
    for (int u = 0; u < kRowGroup; ++u) {
      const float* row = lut + (g + u) * 1024;
      v += row[w[u] & 255u];
      v += row[256 + ((w[u] >> 8) & 255u)];
      v += row[512 + ((w[u] >> 16) & 255u)];
      v += row[768 + (w[u] >> 24)];
    }
  }
  for (; g < G; ++g) {
    const uint32_t w = *col;
    col += stride;
    const float* row = lut + g * 1024;
    v += row[w & 255u];
    v += row[256 + ((w >> 8) & 255u)];
    v += row[512 + ((w >> 16) & 255u)];
    v += row[768 + (w >> 24)];
  }
  return v;
}

// One tile of one cell: the lane owns slot start + off.  Only slots inside [start, start + size) AND inside the storage
// are read (a cell that leaves the storage is cut); tombstones are skipped; NaN fails `v >= thr` on either side.
// RESIDUAL: the value is canonicalised with + 0.0f, as scan_residual_kernel pushes it.
template <bool RESIDUAL>
__device__ __forceinline__ bool tile_hit(const ScanArgs& a, const float* lut, int start, int size, int off, float base,
                                         float thr, float& v, int& s) {
  const int64_t s64 = (int64_t)start + off;
  s = (int)s64;
  v = 0.f;
  if (!(off < size && s64 >= 0 && s64 < a.n_slots)) return false;
  if (a.is_empty && a.is_empty[s64] != 0) return false;
  v = slot_value(reinterpret_cast<const uint32_t*>(a.codes) + s64, a.n_slots, lut, a.m >> 2, base);
  if (RESIDUAL) v = v + 0.0f;
  return v >= thr;
}

// ---- plain PQ ----------------------------------------------------------------------------------------------------
template <bool FILL>
__device__ __forceinline__ void range_body(const ScanArgs& a, const RangeArgs& r, char* smem) {
  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int64_t seg = (int64_t)blockIdx.x * kScanWaves;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  if (Segment<FILL>::no_hit(r, seg)) return;
  Segment<FILL> out(r, seg, wave);
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(smem + (size_t)a.m * 1024);
  const ProbeTable tab =
      probe_table_at(smem + (size_t)a.m * 1024 + (a.lut ? 0 : query_bytes(a.m, a.ds)), a.max_nprobe);
  const int n_probe = clamped_n_probe(a, q);
  if (wave == 0) build_probe_table(a, q, n_probe, tab);
  if (!a.lut) stage_query(a, q, xq, kScanThreads);
  stage_lut_linear(a, q, lut, xq);
  __syncthreads();
  if (out.empty()) return;  // no code is read
  // the part's tiles are scan_ref_kernel's; the wave's chunk of them is contiguous
  const TileRange t = part_tiles(tab.tile_begin[n_probe], part, a.n_split);
  const TileRange c = wave_chunk(t.begin, t.end, wave);
  const float thr = r.threshold[q];
  int p = 0;
  for (int T = c.begin; T < c.end; ++T) {
    float v;
    int s;
    p = probe_of(tab, p, T);
    // (the cell's extent is read ahead of the offset here: through tile_at, which reads the offset first, these two
    // kernels compile to other code)
    const bool hit = tile_hit<false>(a, lut, tab.start[p], tab.size[p], ((T - tab.tile_begin[p]) << 6) + lane, 0.f,
                                     thr, v, s);
    out.emit(a, hit, v, s);
  }
  out.close(r, seg, wave);
}

__global__ __launch_bounds__(kScanThreads) void ivfpq_range_count_kernel(ScanArgs a, RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  range_body<false>(a, r, smem);
}

__global__ __launch_bounds__(kScanThreads) void ivfpq_range_fill_kernel(ScanArgs a, RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  range_body<true>(a, r, smem);
}

// ---- residual PQ -------------------------------------------------------------------------------------------------
template <bool FILL>
__device__ __forceinline__ void residual_body(const ScanArgs& a, const ResidualArgs& ra, const RangeArgs& r,
                                              char* smem) {
  const int q = blockIdx.x / a.max_nprobe;
  const int p = blockIdx.x - q * a.max_nprobe;
  const int64_t seg = (int64_t)blockIdx.x * kScanWaves;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  if (Segment<FILL>::no_hit(r, seg)) return;
  Segment<FILL> out(r, seg, wave);
  // the probe's extent, by the rules of fetch_probes: beyond n_probe_list[q], empty, or the previous probe's start again
  const int n_probe = clamped_n_probe(a, q);
  int start = 0, size = 0;
  if (p < n_probe) {
    const int64_t at = (int64_t)q * a.max_nprobe + p;
    start = (int)a.cell_start[at];
    size = (int)a.cell_size[at];
    if (p > 0 && a.cell_start[at - 1] == (int64_t)start) size = 0;
    if (size < 0) size = 0;
  }
  if (size == 0) {  // (uniform) not scanned: eight zero counts, no table
    if constexpr (!FILL) {
      if (threadIdx.x < kScanWaves) r.wave_counts[seg + threadIdx.x] = 0;
    }
    return;
  }
  // LUT_p, entry for entry as scan_residual_kernel builds it
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(smem + (size_t)a.m * 1024);
  const bool build_part1 = !ra.full && !ra.part1;
  if (build_part1) stage_query(a, q, xq, kScanThreads);
  build_residual_lut(a, ra, q, p, lut, xq, build_part1);
  __syncthreads();
  if (out.empty()) return;  // no code is read
  const float base = ra.base_sims[(int64_t)q * a.max_nprobe + p];
  const float thr = r.threshold[q];
  const TileRange c = wave_chunk(0, (size + 63) >> 6, wave);
  for (int T = c.begin; T < c.end; ++T) {
    float v;
    int s;
    const bool hit = tile_hit<true>(a, lut, start, size, (T << 6) + lane, base, thr, v, s);
    out.emit(a, hit, v, s);
  }
  out.close(r, seg, wave);
}

__global__ __launch_bounds__(kScanThreads) void ivfpq_range_residual_count_kernel(ScanArgs a, ResidualArgs ra,
                                                                                  RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  residual_body<false>(a, ra, r, smem);
}

__global__ __launch_bounds__(kScanThreads) void ivfpq_range_residual_fill_kernel(ScanArgs a, ResidualArgs ra,
                                                                                 RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  residual_body<true>(a, ra, r, smem);
}

// ---- host --------------------------------------------------------------------------------------------------------
// what the four passes check alike (all of it before any HIP call); *done = 1: nothing to launch
static int check_common(const char* what, const uint8_t* codes, const int64_t* cell_start, const int64_t* cell_size,
                        const int64_t* n_probe_list, const float* threshold, const void* counts_or_offsets,
                        const float* out_vals, const int64_t* out_addr, bool fill, int64_t n_slots, int nq,
                        int max_nprobe, int m, int64_t groups_per_query, int* done) {
  *done = 0;
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  TPQ_REQUIRE(m >= 4 && m % 4 == 0, "%s: n_subvectors=%d must be a positive multiple of 4", what, m);
  if (int rc = check_n_slots(what, n_slots)) return rc;
  if (m > 156) {  // (the m KiB table and anything at all beside it: the limit of the top-k scan)
    set_error("%s: n_subvectors=%d > 156: the table does not fit the 160 KiB of LDS of a CU", what, m);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (nq == 0) {
    *done = 1;
    return TPQ_OK;
  }
  TPQ_REQUIRE(codes && cell_start && cell_size && n_probe_list && threshold && counts_or_offsets &&
                  (!fill || (out_vals && out_addr)),
              "%s: null pointer argument", what);
  TPQ_REQUIRE((int64_t)nq * groups_per_query < 0x7fffffffLL, "%s: %lld workgroups", what,
              (long long)nq * groups_per_query);
  return TPQ_OK;
}

static int range_pass(const char* what, const uint8_t* codes, const float* lut, const float* query,
                      const float* codebook, int ds, int metric, const uint8_t* is_empty, const int64_t* cell_start,
                      const int64_t* cell_size, const int64_t* n_probe_list, const float* threshold, int* wave_counts,
                      const int64_t* wave_offsets, float* out_vals, int64_t* out_addr, bool fill, int64_t n_slots,
                      int nq, int max_nprobe, int m, int n_split, tpq_stream_t stream) {
  TPQ_REQUIRE(n_split >= 1 && n_split <= 1024, "%s: n_split=%d out of range", what, n_split);
  int done;
  if (int rc = check_common(what, codes, cell_start, cell_size, n_probe_list, threshold,
                            fill ? (const void*)wave_offsets : (const void*)wave_counts, out_vals, out_addr, fill,
                            n_slots, nq, max_nprobe, m, n_split, &done))
    return rc;
  if (done) return TPQ_OK;
  TPQ_REQUIRE(lut || (query && codebook), "%s: need either lut or (query, codebook)", what);
  if (!lut) {
    TPQ_REQUIRE(ds >= 1 && ds <= 1024, "%s: bad sub-vector length %d", what, ds);
    TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "%s: metric=%d", what, metric);
  }
  const size_t lds = lds_bytes(m, lut ? 0 : ds, max_nprobe);
  if (int rc = check_lds(what, lds)) return rc;
  ScanArgs a = scan_args(codes, nullptr, lut, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr, nullptr,
                         nullptr, n_slots, nq, max_nprobe, m, 0, n_split);
  if (!lut) {
    a.query = query;
    a.codebook = codebook;
    a.ds = ds;
    a.euclid = metric == TPQ_METRIC_NEG_SQ_L2 ? 1 : 0;
  }
  const RangeArgs r{threshold, wave_counts, fill ? wave_offsets : nullptr};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nq * n_split), block(kScanThreads);
  return fill ? launch_with_lds(ivfpq_range_fill_kernel, "ivfpq_range_fill_kernel", grid, block, lds, st, a, r)
              : launch_with_lds(ivfpq_range_count_kernel, "ivfpq_range_count_kernel", grid, block, lds, st, a, r);
}

static int residual_pass(const char* what, const uint8_t* codes, const float* part1, const float* query,
                         const float* codebook, int ds, const float* part2, const float* full_lut,
                         const int64_t* cells, const float* base_sims, const uint8_t* is_empty,
                         const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                         const float* threshold, int* wave_counts, const int64_t* wave_offsets, float* out_vals,
                         int64_t* out_addr, bool fill, int64_t n_slots, int nq, int max_nprobe, int m,
                         tpq_stream_t stream) {
  int done;
  if (int rc = check_common(what, codes, cell_start, cell_size, n_probe_list, threshold,
                            fill ? (const void*)wave_offsets : (const void*)wave_counts, out_vals, out_addr, fill,
                            n_slots, nq, max_nprobe, m, max_nprobe, &done))
    return rc;
  if (done) return TPQ_OK;
  TPQ_REQUIRE(base_sims != nullptr, "%s: base_sims is required", what);
  TPQ_REQUIRE(full_lut || (part2 && cells && (part1 || (query && codebook))),
              "%s: need either full_lut or (part1 or (query, codebook), part2, cells)", what);
  const bool build_part1 = !full_lut && !part1;
  if (build_part1) TPQ_REQUIRE(ds >= 1 && ds <= 1024, "%s: bad sub-vector length %d", what, ds);
  const size_t lds = lds_bytes(m, build_part1 ? ds : 0, 0);
  if (int rc = check_lds(what, lds)) return rc;
  ScanArgs a = scan_args(codes, nullptr, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         nullptr, nullptr, n_slots, nq, max_nprobe, m, 0, 1);
  if (build_part1) {
    a.query = query;
    a.codebook = codebook;
    a.ds = ds;
    a.euclid = 2;  // part1 = 2 q_j . r_jc (fused_lut4)
  }
  const ResidualArgs ra{full_lut ? nullptr : part1, part2, full_lut, cells, base_sims, nullptr, nullptr};
  const RangeArgs r{threshold, wave_counts, fill ? wave_offsets : nullptr};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nq * max_nprobe), block(kScanThreads);
  return fill ? launch_with_lds(ivfpq_range_residual_fill_kernel, "ivfpq_range_residual_fill_kernel", grid, block, lds,
                                st, a, ra, r)
              : launch_with_lds(ivfpq_range_residual_count_kernel, "ivfpq_range_residual_count_kernel", grid, block,
                                lds, st, a, ra, r);
}

}  // namespace pqrange
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq_range_segments(int nq, int n_split) {
  if (nq <= 0 || n_split < 1 || n_split > 1024) return 0;
  return (size_t)nq * n_split * kScanWaves;
}

extern "C" size_t tpq_ivfpq_range_residual_segments(int nq, int max_nprobe) {
  if (nq <= 0 || max_nprobe < 1) return 0;
  return (size_t)nq * max_nprobe * kScanWaves;
}

extern "C" int tpq_ivfpq_range_count(const uint8_t* codes, const float* lut, const float* query, const float* codebook,
                                     int ds, int metric, const uint8_t* is_empty, const int64_t* cell_start,
                                     const int64_t* cell_size, const int64_t* n_probe_list, const float* threshold,
                                     int32_t* wave_counts, int64_t n_slots, int nq, int max_nprobe, int m, int n_split,
                                     tpq_stream_t stream) {
  return pqrange::range_pass("ivfpq_range_count", codes, lut, query, codebook, ds, metric, is_empty, cell_start,
                             cell_size, n_probe_list, threshold, wave_counts, nullptr, nullptr, nullptr, false, n_slots,
                             nq, max_nprobe, m, n_split, stream);
}

extern "C" int tpq_ivfpq_range_fill(const uint8_t* codes, const float* lut, const float* query, const float* codebook,
                                    int ds, int metric, const uint8_t* is_empty, const int64_t* cell_start,
                                    const int64_t* cell_size, const int64_t* n_probe_list, const float* threshold,
                                    const int64_t* wave_offsets, float* out_vals, int64_t* out_addr, int64_t n_slots,
                                    int nq, int max_nprobe, int m, int n_split, tpq_stream_t stream) {
  return pqrange::range_pass("ivfpq_range_fill", codes, lut, query, codebook, ds, metric, is_empty, cell_start,
                             cell_size, n_probe_list, threshold, nullptr, wave_offsets, out_vals, out_addr, true,
                             n_slots, nq, max_nprobe, m, n_split, stream);
}

extern "C" int tpq_ivfpq_range_residual_count(const uint8_t* codes, const float* part1, const float* query,
                                              const float* codebook, int ds, const float* part2,
                                              const float* full_lut, const int64_t* cells, const float* base_sims,
                                              const uint8_t* is_empty, const int64_t* cell_start,
                                              const int64_t* cell_size, const int64_t* n_probe_list,
                                              const float* threshold, int32_t* wave_counts, int64_t n_slots, int nq,
                                              int max_nprobe, int m, tpq_stream_t stream) {
  return pqrange::residual_pass("ivfpq_range_residual_count", codes, part1, query, codebook, ds, part2, full_lut,
                                cells, base_sims, is_empty, cell_start, cell_size, n_probe_list, threshold,
                                wave_counts, nullptr, nullptr, nullptr, false, n_slots, nq, max_nprobe, m, stream);
}

extern "C" int tpq_ivfpq_range_residual_fill(const uint8_t* codes, const float* part1, const float* query,
                                             const float* codebook, int ds, const float* part2, const float* full_lut,
                                             const int64_t* cells, const float* base_sims, const uint8_t* is_empty,
                                             const int64_t* cell_start, const int64_t* cell_size,
                                             const int64_t* n_probe_list, const float* threshold,
                                             const int64_t* wave_offsets, float* out_vals, int64_t* out_addr,
                                             int64_t n_slots, int nq, int max_nprobe, int m, tpq_stream_t stream) {
  return pqrange::residual_pass("ivfpq_range_residual_fill", codes, part1, query, codebook, ds, part2, full_lut, cells,
                                base_sims, is_empty, cell_start, cell_size, n_probe_list, threshold, nullptr,
                                wave_offsets, out_vals, out_addr, true, n_slots, nq, max_nprobe, m, stream);
}
