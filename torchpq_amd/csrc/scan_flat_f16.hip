// List scan and range search of IVFFlat16Index (tpq_ivf_flat16_scan_topk / _range_count / _range_fill): the probed
// cells hold the vectors as fp16, two components per dword.
//
// A vector of d components is rows = ceil(d / 2) dwords: dword r holds component 2r in its low half and 2r + 1 in its
// high half (an odd d leaves the last high half +0; it is never read into a value).  The container stores that as
// 4 rows code bytes, so the storage read as 32-bit words is row-major and slot-contiguous: vectors[r * n_slots + s] is
// dimension pair r of slot s.  A lane that owns a slot issues one dword load per row and a wave reads 256 contiguous
// bytes per load -- the access shape of the fp32 scan (scan_flat.hip) with half as many loads per slot.
//
// Value: each half is converted to fp32 (exact, v_cvt_f32_f16; the high half through the instruction's word select,
// so no shift) and goes through the chain of tpq_ivfflat_scan_topk in component order -- low half, then high half, rows
// ascending; the build has -ffp-contract=off.  The result is bit for bit the fp32 scan's over float(half(x)).
// kRowsInFlight row loads are issued before the first of their 2 kRowsInFlight chain steps; the query lies in LDS as
// fp32 and a row's two components are neighbours there.
//
// Frame: one workgroup per (query, part), eight waves, 64-slot tiles round-robin, the selector, the shared threshold,
// the pending list of the masked form, the finisher and the split merge are the list kernels' (scan_list.h,
// scan_device.h); the masked form keeps scan_flat.hip's contract -- mask byte before any vector byte, an empty tile reads
// nothing, a tile below kCompactBelow live slots goes through the pending list, any other is valued in place.
// Range search: count and fill passes over a wave's contiguous chunk of tiles with the same value code; no global atomic.
// (low_half / high_half, pair_step and slot_value are in scan_flat_f16.h: the cell-major route's finish kernel,
// scan_flat_f16_cells.hip, values its candidates with the same definition.)
#include "scan_device.h"
#include "scan_flat_f16.h"
#include "scan_ref.h"

namespace tpq {
namespace flat16 {

constexpr int kMaskTilesAhead = 4;  // tiles whose mask bytes are loaded together (as scan_flat.hip)
constexpr int kCompactBelow = 4;    // a tile with fewer live slots than this is compacted (as scan_flat.hip)

struct Flat16Args {
  const uint32_t* vectors;  // [ceil(d / 2)][n_slots]
  int d;
};

__host__ __device__ constexpr size_t query_bytes(int d) { return align16((size_t)d * 4); }

// every thread of the workgroup takes its share of the query's d floats (the caller's barrier publishes them)
__device__ __forceinline__ void stage_query(const ScanArgs& a, int q, int d, float* xq) {
  for (int i = threadIdx.x; i < d; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
}

// (a cell that leaves the storage is cut)
__device__ __forceinline__ bool in_storage(const ScanArgs& a, int s) { return s >= 0 && (int64_t)s < a.n_slots; }

// LDS: [query d floats | the finisher's merge lists, which start once the scan is over][queues][probe table][threshold]
// and, MASKED, the pending lists behind them
template <int R, int METRIC, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void scan_flat16_kernel(ScanArgs a, Flat16Args f, size_t region0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xq = reinterpret_cast<float*>(smem);
  const ListLds lds(smem, region0, a.max_nprobe);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int d = f.d;
  const int n_probe = clamped_n_probe(a, q);

  lds.init(a, q, n_probe, wave, lane);
  stage_query(a, q, d, xq);
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);

  const TileRange t = part_tiles(lds.tab.tile_begin[n_probe], part, a.n_split);
  const int64_t stride = a.n_slots;

  int p = 0;
  if constexpr (MASKED) {
    Pending pend{reinterpret_cast<int*>(lds.tail) + wave * kPendingPerWave, 0};
    for (int T0 = t.begin + wave; T0 < t.end; T0 += kScanWaves * kMaskTilesAhead) {
      // a tile's first slot and how many of its lanes lie inside the cell: wave-uniform
      int first[kMaskTilesAhead], inside[kMaskTilesAhead];
#pragma unroll
      for (int u = 0; u < kMaskTilesAhead; ++u) {
        const int T = T0 + u * kScanWaves;
        first[u] = inside[u] = 0;
        if (T < t.end) {  // (uniform)
          p = probe_of(lds.tab, p, T);
          const Tile tile = tile_at(lds.tab, p, T, 0);
          first[u] = __builtin_amdgcn_readfirstlane(tile.slot());
          inside[u] = __builtin_amdgcn_readfirstlane(tile.size - tile.off);
        }
      }
      // the mask bytes of the four tiles, in flight together, before any vector byte
      unsigned long long live_mask[kMaskTilesAhead], valid_mask[kMaskTilesAhead];  // (uniform)
      {
        uint8_t dead[kMaskTilesAhead];
#pragma unroll
        for (int u = 0; u < kMaskTilesAhead; ++u) {
          const int s = first[u] + lane;
          const bool valid = lane < inside[u] && in_storage(a, s);
          valid_mask[u] = __ballot(valid);
          dead[u] = valid ? a.is_empty[s] : (uint8_t)1;
        }
#pragma unroll
        for (int u = 0; u < kMaskTilesAhead; ++u) live_mask[u] = __ballot(dead[u] == 0);
      }
#pragma unroll
      for (int u = 0; u < kMaskTilesAhead; ++u) {
        if (live_mask[u] == 0ull) continue;  // no vector is read
        int s = first[u] + lane;
        bool live = (live_mask[u] >> lane) & 1ull;
        if (live_mask[u] != valid_mask[u] && __popcll(live_mask[u]) < kCompactBelow) {
          // a sparse tile: its live slots wait until 64 are pending
          pend.append(live, s);
          if (pend.n < 64) continue;
          s = pend.take(64);
          live = true;
        }
        float v = 0.f;
        if (live) v = slot_value<METRIC, 1>(f.vectors + s, xq, d, stride);
        admit(sel, lds.tau_key, live, v, s);
      }
    }
    if (pend.n > 0) {  // the drain: what is left, one slot per lane
      const int count = pend.n;
      const int s = pend.take(count);
      const bool live = lane < count;
      float v = 0.f;
      if (live) v = slot_value<METRIC, 1>(f.vectors + s, xq, d, stride);
      admit(sel, lds.tau_key, live, v, s);
    }
  } else {
    for (int T = t.begin + wave; T < t.end; T += kScanWaves) {
      p = probe_of(lds.tab, p, T);
      const Tile tile = tile_at(lds.tab, p, T, lane);
      const int s = tile.slot();
      const bool live = tile.in_cell() && in_storage(a, s);
      float v = 0.f;
      if (live) v = slot_value<METRIC, 2>(f.vectors + s, xq, d, stride);
      admit(sel, lds.tau_key, live, v, s);
    }
  }
  sel.flush();
  finish_list_scan<R>(a, q, part, sel.top, smem);
}

template <int METRIC>
static int dispatch(const ScanArgs& a, const Flat16Args& f, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    const size_t region0 = list_region0(query_bytes(f.d), RC);
    if (a.is_empty)
      return launch_list_scan(scan_flat16_kernel<RC, METRIC, true>, scan_merge_kernel<RC>,
                              "scan_flat16_kernel (masked)", a,
                              list_scan_lds_bytes(region0, a.max_nprobe, kPendingBytes), st, f, region0);
    return launch_list_scan(scan_flat16_kernel<RC, METRIC, false>, scan_merge_kernel<RC>, "scan_flat16_kernel", a,
                            list_scan_lds_bytes(region0, a.max_nprobe, 0), st, f, region0);
  });
}

// ---- range search ------------------------------------------------------------------------------------------------
// Every candidate of the top-k scan whose value is >= the query's threshold, in scan order: the two-pass protocol of
// tpq_ivfflat_range_count / _fill (Segment, scan_list.h).  Inside a part a wave owns a CONTIGUOUS chunk of the tiles, so
// the segments in (query, part, wave) order are tile-ascending whatever n_split is.  LDS: the query and the probe table.
template <int METRIC, bool FILL>
__global__ __launch_bounds__(kScanThreads) void range_flat16_kernel(ScanArgs a, Flat16Args f, RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int64_t seg = (int64_t)blockIdx.x * kScanWaves;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  if (Segment<FILL>::no_hit(r, seg)) return;  // (uniform over the workgroup: before the barrier)
  Segment<FILL> out(r, seg, wave);
  float* xq = reinterpret_cast<float*>(smem);
  const ProbeTable tab = probe_table_at(smem + query_bytes(f.d), a.max_nprobe);
  const int n_probe = clamped_n_probe(a, q);
  if (wave == 0) build_probe_table(a, q, n_probe, tab);
  stage_query(a, q, f.d, xq);
  __syncthreads();
  const TileRange t = part_tiles(tab.tile_begin[n_probe], part, a.n_split);
  const TileRange c = wave_chunk(t.begin, t.end, wave);
  const float thr = r.threshold[q];
  if (out.empty()) return;  // no vector is read
  int p = 0;
  for (int T = c.begin; T < c.end; ++T) {
    p = probe_of(tab, p, T);
    const Tile tile = tile_at(tab, p, T, lane);
    const int s = tile.slot();
    bool hit = false;
    float v = 0.f;
    if (tile.in_cell() && in_storage(a, s) && !(a.is_empty && a.is_empty[s] != 0)) {
      v = slot_value<METRIC, 1>(f.vectors + s, xq, f.d, a.n_slots);
      hit = v >= thr;  // a NaN value and a NaN threshold fail
    }
    out.emit(a, hit, v, s);  // once per tile, wave-uniformly
  }
  out.close(r, seg, wave);
}

template <int METRIC>
static int launch_range(const ScanArgs& a, const Flat16Args& f, const RangeArgs& r, hipStream_t st) {
  const size_t lds = query_bytes(f.d) + probe_table_bytes(a.max_nprobe);
  const bool fill = r.wave_offsets != nullptr;
  const char* name = fill ? "range_flat16_kernel (fill)" : "range_flat16_kernel (count)";
  if (int rc = check_lds(name, lds)) return rc;
  const dim3 grid((unsigned)a.nq * a.n_split), block(kScanThreads);
  return fill ? launch_with_lds(range_flat16_kernel<METRIC, true>, name, grid, block, lds, st, a, f, r)
              : launch_with_lds(range_flat16_kernel<METRIC, false>, name, grid, block, lds, st, a, f, r);
}

// the arguments of the three entry points, once their checks have passed
static ScanArgs list_args(const float* query, const uint8_t* is_empty, const int64_t* cell_start,
                          const int64_t* cell_size, const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                          int64_t n_slots, int nq, int max_nprobe, int k, int n_split) {
  ScanArgs a = scan_args(nullptr, nullptr, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         nullptr, nullptr, n_slots, nq, max_nprobe, 0, k, n_split);
  a.query = query;
  return a;
}

// what the two range entry points share: the checks of the top-k scan in its order (all before any HIP call), then the
// launch -- the fill pass when `fill`
static int range_pass(const char* what, const uint32_t* vectors, const float* query, const uint8_t* is_empty,
                      const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                      const float* threshold, int* wave_counts, const int64_t* wave_offsets, float* out_vals,
                      int64_t* out_addr, bool fill, int64_t n_slots, int d, int nq, int max_nprobe, int metric,
                      int n_split, tpq_stream_t stream) {
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  TPQ_REQUIRE(d >= 1, "%s: d=%d", what, d);
  if (int rc = check_lists(what, metric, n_split, n_slots)) return rc;
  if (nq == 0) return TPQ_OK;
  if (int rc = check_grid(what,
                          vectors && query && cell_start && cell_size && n_probe_list && threshold &&
                              (fill ? (wave_offsets && out_vals && out_addr) : wave_counts != nullptr),
                          nq, n_split))
    return rc;
  const ScanArgs a = list_args(query, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr, n_slots, nq,
                               max_nprobe, 0, n_split);
  const Flat16Args f{vectors, d};
  const RangeArgs r{threshold, wave_counts, fill ? wave_offsets : nullptr};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? launch_range<TPQ_METRIC_NEG_SQ_L2>(a, f, r, st)
                                        : launch_range<TPQ_METRIC_INNER>(a, f, r, st);
}

}  // namespace flat16
}  // namespace tpq

using namespace tpq;

// tpq_ivf_flat16_scan_topk over each query's first min(n_probe_list[q], probe_cap) probes (ScanArgs::probe_cap; 0: no
// cap): the threshold pass of the cell-major route (scan_flat_f16_cells.hip) -- the same kernels, checks and launches
int tpq::ivf_flat16_scan_topk_capped(const uint32_t* vectors, const float* query, const uint8_t* is_empty,
                                     const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                     float* out_vals, int64_t* out_addr, int64_t n_slots, int d, int nq, int max_nprobe,
                                     int k, int metric, int n_split, int probe_cap, void* workspace,
                                     size_t workspace_bytes, tpq_stream_t stream) {
  const char* what = "ivf_flat16_scan";
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  TPQ_REQUIRE(d >= 1, "ivf_flat16_scan: d=%d", d);
  TPQ_REQUIRE(k >= 1 && k <= 1024, "ivf_flat16_scan: k=%d out of range (0, 1024]", k);
  if (int rc = check_lists(what, metric, n_split, n_slots)) return rc;
  if (nq == 0) return TPQ_OK;
  if (int rc = check_grid(what, vectors && query && cell_start && cell_size && n_probe_list && out_vals && out_addr, nq,
                          n_split))
    return rc;
  const int R = list_regs(k);
  ScanArgs a = flat16::list_args(query, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr, n_slots, nq,
                                 max_nprobe, k, n_split);
  a.probe_cap = probe_cap;
  if (int rc = take_list_ws(a, R, workspace, workspace_bytes, what)) return rc;
  const flat16::Flat16Args f{vectors, d};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? flat16::dispatch<TPQ_METRIC_NEG_SQ_L2>(a, f, R, st)
                                        : flat16::dispatch<TPQ_METRIC_INNER>(a, f, R, st);
}

extern "C" int tpq_ivf_flat16_scan_topk(const uint32_t* vectors, const float* query, const uint8_t* is_empty,
                                        const int64_t* cell_start, const int64_t* cell_size,
                                        const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                        int64_t n_slots, int d, int nq, int max_nprobe, int k, int metric, int n_split,
                                        void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  return ivf_flat16_scan_topk_capped(vectors, query, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                                     n_slots, d, nq, max_nprobe, k, metric, n_split, 0, workspace, workspace_bytes,
                                     stream);
}

extern "C" int tpq_ivf_flat16_range_count(const uint32_t* vectors, const float* query, const uint8_t* is_empty,
                                          const int64_t* cell_start, const int64_t* cell_size,
                                          const int64_t* n_probe_list, const float* threshold, int32_t* wave_counts,
                                          int64_t n_slots, int d, int nq, int max_nprobe, int metric, int n_split,
                                          tpq_stream_t stream) {
  return flat16::range_pass("ivf_flat16_range_count", vectors, query, is_empty, cell_start, cell_size, n_probe_list,
                            threshold, wave_counts, nullptr, nullptr, nullptr, false, n_slots, d, nq, max_nprobe,
                            metric, n_split, stream);
}

extern "C" int tpq_ivf_flat16_range_fill(const uint32_t* vectors, const float* query, const uint8_t* is_empty,
                                         const int64_t* cell_start, const int64_t* cell_size,
                                         const int64_t* n_probe_list, const float* threshold,
                                         const int64_t* wave_offsets, float* out_vals, int64_t* out_addr,
                                         int64_t n_slots, int d, int nq, int max_nprobe, int metric, int n_split,
                                         tpq_stream_t stream) {
  return flat16::range_pass("ivf_flat16_range_fill", vectors, query, is_empty, cell_start, cell_size, n_probe_list,
                            threshold, nullptr, wave_offsets, out_vals, out_addr, true, n_slots, d, nq, max_nprobe,
                            metric, n_split, stream);
}
