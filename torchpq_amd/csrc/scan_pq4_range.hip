// Range search over the lists of IVFPQ4Index (tpq_ivfpq4_range_count / _fill and their residual forms),
// with an optional filter.
//
// Every candidate of the 4-bit top-k scan (scan_pq4.hip) whose value is >= the query's threshold, in scan order.  The
// parts are those units' own: the codes are read as CellContainer stores them (u32 [m / 8][n_slots], a lane owns one
// slot of a 64-slot tile), the table is built in the workgroup entry for entry as scan_pq4_kernel / build_group_luts
// build it, the value is pq4::code_value's ascending-j fp32 sum from 0.f -- so a hit carries the bits `search` returns
// for that slot under that probe.  Two passes over the same tiles on the protocol of scan_range.hip (Segment<FILL>,
// scan_list.h): the count pass counts each wave's hits, the caller turns the counts into offsets, the fill pass
// computes the values again and appends each wave's hits at its offset.  No global atomic, no sort, no selector.
//
//   plain codes     one workgroup per (query, part); the query's m x 16 table is built once, the part's tiles are
//                   scan_pq4_kernel's (part_tiles) and inside the part a wave owns a CONTIGUOUS chunk of them:
//                   segment (q * n_split + part) * 8 + wave.
//   residual codes  the table depends on the probed cell, so the work is cut by probe: one workgroup per (query, probe
//                   rank) builds that probe's table (build_group_luts with a group of one) and its waves take contiguous
//                   chunks of that cell's tiles: segment (q * max_nprobe + p) * 8 + wave.  A probe that is not scanned
//                   costs eight zero counts.  (The grouped two-buffer walk of scan_pq4_residual_kernel deals tiles
//                   round-robin, which would break the contiguous segments the order rests on.)
//
// Filter (FILTERED, the rows of scan_pq4_filtered.hip): a lane tests its bit before the tombstone byte and before any
// code word; a tile whose ballot of allowed live lanes is zero reads no code; every other tile is valued in place with
// the disallowed lanes off -- no compaction across tiles, which would have to keep scan order inside a segment.  A query
// whose row is outside [0, n_filters) has zero counts and reads neither the filter nor the codes.  The unfiltered
// instantiation holds no filter load.
//
// LDS: [table m x 16 floats][query m * ds floats][probe table, plain only].  Nothing else: no candidate lists, no
// shared threshold, no barrier after the table.
#include "scan_pq4.h"

namespace tpq {
namespace pq4range {

using filtered::FilterArgs;
using filtered::filter_row;
using filtered::Member;
using filtered::member;
using pq4::ResidualProbes;

__host__ __device__ constexpr size_t table_bytes(int m) { return (size_t)m * 64; }
__host__ __device__ constexpr size_t query_bytes(int m, int ds) { return align16((size_t)m * ds * 4); }
static size_t lds_bytes(int m, int ds, int probe_entries) {
  return table_bytes(m) + query_bytes(m, ds) + (probe_entries ? align16(probe_table_bytes(probe_entries)) : 0);
}

// the eight segments of a workgroup that scans nothing (count pass)
template <bool FILL>
__device__ __forceinline__ void no_counts(const RangeArgs& r, int64_t seg) {
  if constexpr (!FILL) {
    if (threadIdx.x < kScanWaves) r.wave_counts[seg + threadIdx.x] = 0;
  }
}

// The query's table, as scan_pq4_kernel builds it: thread t takes entries t, t + 512, ...; the same metric_step chain,
// i ascending from 0.f.  (That kernel keeps its own loop: its code is not touched by this unit.)
template <int METRIC>
__device__ __forceinline__ void build_lut(const ScanArgs& a, const float* xq, float* lut) {
  const int ds = a.ds;
  for (int e = threadIdx.x; e < a.m * 16; e += kScanThreads) {
    const int j = e >> 4;
    const float* __restrict__ cb = a.codebook + (int64_t)j * ds * 16 + (e & 15);
    const float* xj = xq + j * ds;
    float acc = 0.f;
    for (int i = 0; i < ds; ++i) acc = metric_step<METRIC>(acc, xj[i], cb[i * 16]);
    lut[e] = acc;
  }
}

// One tile of one cell: the lane owns slot start + off.  Only slots inside [start, start + size) AND inside the storage
// are read (a cell that leaves the storage is cut); with a filter the bit comes first, then the tombstone byte, then --
// unless no lane of the tile is left -- the code; NaN fails `v >= thr` on either side.
template <bool FILTERED>
__device__ __forceinline__ bool tile_hit(const ScanArgs& a, const uint32_t* __restrict__ frow, const float* lut,
                                         int start, int size, int off, float thr, float& v, int& s) {
  bool live;
  if constexpr (FILTERED) {
    const Member mb = member(frow, start, size, off, a.n_slots);
    s = mb.s;
    live = mb.ok;
  } else {
    const int64_t s64 = (int64_t)start + off;
    s = (int)s64;
    live = off < size && s64 >= 0 && s64 < a.n_slots;
  }
  if (live && a.is_empty) live = a.is_empty[s] == 0;
  v = 0.f;
  if constexpr (FILTERED) {
    if (__ballot(live) == 0ull) return false;  // (uniform) no allowed live slot: no code word is read
  }
  if (!live) return false;
  v = pq4::code_value(reinterpret_cast<const uint32_t*>(a.codes) + s, a.n_slots, lut, a.m >> 3);
  return v >= thr;
}

// ---- plain codes -------------------------------------------------------------------------------------------------
template <bool FILL, bool FILTERED, int METRIC>
__device__ __forceinline__ void plain_body(const ScanArgs& a, const RangeArgs& r, const FilterArgs& f, char* smem) {
  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int64_t seg = (int64_t)blockIdx.x * kScanWaves;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  if (Segment<FILL>::no_hit(r, seg)) return;
  Segment<FILL> out(r, seg, wave);
  const uint32_t* __restrict__ frow = nullptr;
  if constexpr (FILTERED) {
    frow = filter_row(f, q);  // (uniform)
    if (!frow) {              // no such row: no candidate, nothing staged, neither the filter nor the codes are read
      no_counts<FILL>(r, seg);
      return;
    }
  }
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(smem + table_bytes(a.m));
  const ProbeTable tab = probe_table_at(smem + table_bytes(a.m) + query_bytes(a.m, a.ds), a.max_nprobe);
  const int n_probe = clamped_n_probe(a, q);
  if (wave == 0) build_probe_table(a, q, n_probe, tab);
  stage_query(a, q, xq, kScanThreads);
  build_lut<METRIC>(a, xq, lut);
  __syncthreads();
  if (out.empty()) return;  // no code is read
  // the part's tiles are scan_pq4_kernel's; the wave's chunk of them is contiguous
  const TileRange t = part_tiles(tab.tile_begin[n_probe], part, a.n_split);
  const TileRange c = wave_chunk(t.begin, t.end, wave);
  const float thr = r.threshold[q];
  int p = 0;
  for (int T = c.begin; T < c.end; ++T) {
    float v;
    int s;
    p = probe_of(tab, p, T);
    const Tile tile = tile_at(tab, p, T, lane);
    const bool hit = tile_hit<FILTERED>(a, frow, lut, tile.start, tile.size, tile.off, thr, v, s);
    out.emit(a, hit, v, s);
  }
  out.close(r, seg, wave);
}

template <bool FILL, bool FILTERED, int METRIC>
__global__ __launch_bounds__(kScanThreads) void ivfpq4_range_kernel(ScanArgs a, RangeArgs r, FilterArgs f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  plain_body<FILL, FILTERED, METRIC>(a, r, f, smem);
}

// ---- residual codes ----------------------------------------------------------------------------------------------
template <bool FILL, bool FILTERED, int METRIC>
__device__ __forceinline__ void residual_body(const ScanArgs& a, const ResidualProbes& rp, const RangeArgs& r,
                                              const FilterArgs& f, char* smem) {
  const int q = blockIdx.x / a.max_nprobe;
  const int p = blockIdx.x - q * a.max_nprobe;
  const int64_t seg = (int64_t)blockIdx.x * kScanWaves;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  if (Segment<FILL>::no_hit(r, seg)) return;
  Segment<FILL> out(r, seg, wave);
  const uint32_t* __restrict__ frow = nullptr;
  if constexpr (FILTERED) {
    frow = filter_row(f, q);  // (uniform)
    if (!frow) {
      no_counts<FILL>(r, seg);
      return;
    }
  }
  // the probe's extent, by the rules of fetch_probes: beyond n_probe_list[q], empty, or the previous probe's start again
  const int n_probe = clamped_n_probe(a, q);
  const int64_t at = (int64_t)q * a.max_nprobe + p;
  int start = 0, size = 0;
  if (p < n_probe) {
    start = (int)a.cell_start[at];
    size = (int)a.cell_size[at];
    if (p > 0 && a.cell_start[at - 1] == (int64_t)start) size = 0;
    if (size < 0) size = 0;
  }
  if (size == 0) {  // (uniform) not scanned: eight zero counts, no table
    no_counts<FILL>(r, seg);
    return;
  }
  // the probe's table, entry for entry as scan_pq4_residual_kernel builds it: a group of one
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(smem + table_bytes(a.m));
  // (a cell index outside [0, n_cells) is the caller's error: clamped, so that nothing outside `centroids` is read)
  const int64_t c64 = rp.cells[at];
  const int cell = c64 < 0 ? 0 : (c64 >= rp.n_cells ? rp.n_cells - 1 : (int)c64);
  stage_query(a, q, xq, kScanThreads);
  pq4::build_group_luts<METRIC>(a, rp.centroids, &cell, 0, 1, xq, lut);
  __syncthreads();
  if (out.empty()) return;  // no code is read
  const float thr = r.threshold[q];
  const int n_tiles = (int)(((int64_t)size + 63) >> 6);
  const TileRange c = wave_chunk(0, n_tiles, wave);
  for (int T = c.begin; T < c.end; ++T) {
    float v;
    int s;
    const bool hit = tile_hit<FILTERED>(a, frow, lut, start, size, (T << 6) + lane, thr, v, s);
    out.emit(a, hit, v, s);
  }
  out.close(r, seg, wave);
}

template <bool FILL, bool FILTERED, int METRIC>
__global__ __launch_bounds__(kScanThreads) void ivfpq4_range_residual_kernel(ScanArgs a, ResidualProbes rp, RangeArgs r,
                                                                             FilterArgs f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  residual_body<FILL, FILTERED, METRIC>(a, rp, r, f, smem);
}

// ---- host --------------------------------------------------------------------------------------------------------
template <bool FILL, bool FILTERED, int METRIC>
static int launch(const ScanArgs& a, const ResidualProbes* rp, const RangeArgs& r, const FilterArgs& f, size_t lds,
                  hipStream_t st) {
  const dim3 block(kScanThreads);
  if (rp)
    return launch_with_lds(ivfpq4_range_residual_kernel<FILL, FILTERED, METRIC>, "ivfpq4_range_residual_kernel",
                           dim3((unsigned)a.nq * a.max_nprobe), block, lds, st, a, *rp, r, f);
  return launch_with_lds(ivfpq4_range_kernel<FILL, FILTERED, METRIC>, "ivfpq4_range_kernel",
                         dim3((unsigned)a.nq * a.n_split), block, lds, st, a, r, f);
}

template <bool FILL, bool FILTERED>
static int launch_metric(int metric, const ScanArgs& a, const ResidualProbes* rp, const RangeArgs& r,
                         const FilterArgs& f, size_t lds, hipStream_t st) {
  return metric == TPQ_METRIC_NEG_SQ_L2 ? launch<FILL, FILTERED, TPQ_METRIC_NEG_SQ_L2>(a, rp, r, f, lds, st)
                                        : launch<FILL, FILTERED, TPQ_METRIC_INNER>(a, rp, r, f, lds, st);
}

// The four entry points: `rp` is null for plain codes, `fill` chooses the pass.  The checks of tpq_ivfpq4_scan_topk in
// its order, the filter's when there is one, the pointers, the grid, the LDS; all of them before any HIP call.
static int range_pass(const char* what, const ResidualProbes* rp, bool fill, const uint8_t* codes, const float* query,
                      const float* codebook, const uint8_t* is_empty, const int64_t* cell_start,
                      const int64_t* cell_size, const int64_t* n_probe_list, const uint32_t* filter_bits,
                      const int32_t* filter_of_query, int n_filters, int64_t filter_stride, const float* threshold,
                      int32_t* wave_counts, const int64_t* wave_offsets, float* out_vals, int64_t* out_addr,
                      int64_t n_slots, int m, int ds, int nq, int max_nprobe, int metric, int n_split,
                      tpq_stream_t stream) {
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  if (m < pq4::kMinM || m > pq4::kMaxM || m % 8 != 0 || ds < 1) {
    set_error("%s: m=%d, ds=%d: m must be a multiple of 8 in [8, 256], ds >= 1", what, m, ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (int rc = check_lists(what, metric, n_split, n_slots)) return rc;
  if ((int64_t)m * ds > (1 << 20)) {  // (far beyond the LDS; keeps m * ds * 4 inside an int)
    set_error("%s: d = m * ds = %lld is not supported", what, (long long)m * ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (rp) TPQ_REQUIRE(rp->n_cells >= 1, "%s: n_cells=%d", what, rp->n_cells);
  if (filter_bits) {
    TPQ_REQUIRE(n_filters >= 1, "%s: n_filters=%d", what, n_filters);
    TPQ_REQUIRE(filter_stride >= (n_slots + 31) / 32, "%s: filter_stride=%lld < ceil(n_slots / 32) = %lld", what,
                (long long)filter_stride, (long long)((n_slots + 31) / 32));
  }
  if (nq == 0) return TPQ_OK;
  const int groups = rp ? max_nprobe : n_split;  // workgroups per query
  if (int rc = check_grid(what,
                          codes && query && codebook && cell_start && cell_size && n_probe_list && threshold &&
                              (fill ? (wave_offsets && out_vals && out_addr) : wave_counts != nullptr) &&
                              (!rp || (rp->centroids && rp->cells)),
                          nq, groups))
    return rc;
  const size_t lds = lds_bytes(m, ds, rp ? 0 : max_nprobe);
  if (int rc = check_lds(what, lds)) return rc;
  ScanArgs a = scan_args(codes, nullptr, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         nullptr, nullptr, n_slots, nq, max_nprobe, m, 0, n_split);
  a.query = query;
  a.codebook = codebook;
  a.ds = ds;
  const RangeArgs r{threshold, wave_counts, fill ? wave_offsets : nullptr};
  const FilterArgs f{filter_bits, filter_of_query, filter_stride, n_filters};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (fill)
    return filter_bits ? launch_metric<true, true>(metric, a, rp, r, f, lds, st)
                       : launch_metric<true, false>(metric, a, rp, r, f, lds, st);
  return filter_bits ? launch_metric<false, true>(metric, a, rp, r, f, lds, st)
                     : launch_metric<false, false>(metric, a, rp, r, f, lds, st);
}

}  // namespace pq4range
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq4_range_segments(int nq, int n_split) {
  if (nq <= 0 || n_split < 1 || n_split > 1024) return 0;
  return (size_t)nq * n_split * kScanWaves;
}

extern "C" size_t tpq_ivfpq4_range_residual_segments(int nq, int max_nprobe) {
  if (nq <= 0 || max_nprobe < 1) return 0;
  return (size_t)nq * max_nprobe * kScanWaves;
}

extern "C" int tpq_ivfpq4_range_count(const uint8_t* codes, const float* query, const float* codebook,
                                      const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                                      const int64_t* n_probe_list, const uint32_t* filter_bits,
                                      const int32_t* filter_of_query, int n_filters, int64_t filter_stride,
                                      const float* threshold, int32_t* wave_counts, int64_t n_slots, int m, int ds,
                                      int nq, int max_nprobe, int metric, int n_split, tpq_stream_t stream) {
  return pq4range::range_pass("ivfpq4_range_count", nullptr, false, codes, query, codebook, is_empty, cell_start,
                              cell_size, n_probe_list, filter_bits, filter_of_query, n_filters, filter_stride,
                              threshold, wave_counts, nullptr, nullptr, nullptr, n_slots, m, ds, nq, max_nprobe,
                              metric, n_split, stream);
}

extern "C" int tpq_ivfpq4_range_fill(const uint8_t* codes, const float* query, const float* codebook,
                                     const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                                     const int64_t* n_probe_list, const uint32_t* filter_bits,
                                     const int32_t* filter_of_query, int n_filters, int64_t filter_stride,
                                     const float* threshold, const int64_t* wave_offsets, float* out_vals,
                                     int64_t* out_addr, int64_t n_slots, int m, int ds, int nq, int max_nprobe,
                                     int metric, int n_split, tpq_stream_t stream) {
  return pq4range::range_pass("ivfpq4_range_fill", nullptr, true, codes, query, codebook, is_empty, cell_start,
                              cell_size, n_probe_list, filter_bits, filter_of_query, n_filters, filter_stride,
                              threshold, nullptr, wave_offsets, out_vals, out_addr, n_slots, m, ds, nq, max_nprobe,
                              metric, n_split, stream);
}

extern "C" int tpq_ivfpq4_range_residual_count(const uint8_t* codes, const float* query, const float* codebook,
                                               const float* centroids, const int64_t* cells, int n_cells,
                                               const uint8_t* is_empty, const int64_t* cell_start,
                                               const int64_t* cell_size, const int64_t* n_probe_list,
                                               const uint32_t* filter_bits, const int32_t* filter_of_query,
                                               int n_filters, int64_t filter_stride, const float* threshold,
                                               int32_t* wave_counts, int64_t n_slots, int m, int ds, int nq,
                                               int max_nprobe, int metric, tpq_stream_t stream) {
  const pq4::ResidualProbes rp{centroids, cells, n_cells};
  return pq4range::range_pass("ivfpq4_range_residual_count", &rp, false, codes, query, codebook, is_empty, cell_start,
                              cell_size, n_probe_list, filter_bits, filter_of_query, n_filters, filter_stride,
                              threshold, wave_counts, nullptr, nullptr, nullptr, n_slots, m, ds, nq, max_nprobe,
                              metric, 1, stream);
}

extern "C" int tpq_ivfpq4_range_residual_fill(const uint8_t* codes, const float* query, const float* codebook,
                                              const float* centroids, const int64_t* cells, int n_cells,
                                              const uint8_t* is_empty, const int64_t* cell_start,
                                              const int64_t* cell_size, const int64_t* n_probe_list,
                                              const uint32_t* filter_bits, const int32_t* filter_of_query,
                                              int n_filters, int64_t filter_stride, const float* threshold,
                                              const int64_t* wave_offsets, float* out_vals, int64_t* out_addr,
                                              int64_t n_slots, int m, int ds, int nq, int max_nprobe, int metric,
                                              tpq_stream_t stream) {
  const pq4::ResidualProbes rp{centroids, cells, n_cells};
  return pq4range::range_pass("ivfpq4_range_residual_fill", &rp, true, codes, query, codebook, is_empty, cell_start,
                              cell_size, n_probe_list, filter_bits, filter_of_query, n_filters, filter_stride,
                              threshold, nullptr, wave_offsets, out_vals, out_addr, n_slots, m, ds, nq, max_nprobe,
                              metric, 1, stream);
}
