// List scan of IVFFlatIndex (tpq_ivfflat_scan_topk): the probed cells hold the vectors themselves.
//
// The container stores a vector of d floats as 4 d code bytes, so the storage read as fp32 is dimension-major and
// slot-contiguous: vectors[i * n_slots + s] is component i of slot s.  One workgroup per (query, part), eight waves,
// on the frame of the list kernels (scan_list.h): the query lies in LDS (d floats), a wave takes the 64-slot tiles of
// the probed cells round-robin, a lane owns one slot of the tile and walks the dimensions in ascending order -- a wave
// reads 256 contiguous bytes per dimension, kFlatUnroll rows in flight -- and the value goes through the per-wave
// selector and the workgroup-shared threshold of the code scans.  The summation order of the value definition
// (include/torchpq_amd.h) is the loop order; the build has -ffp-contract=off, so no product is fused into its sum.
// A query's tiles are cut into n_split parts when the batch is small; scan_merge_kernel merges the parts' lists.
//
// This is the per-query streaming scan: 4 d bytes per scanned slot, read again by every query that probes the cell
// (from L2 or the Infinity Cache while the index fits them).  Grouping the queries that probe one cell into a matrix
// tile is not done here.
//
// Range search over the same candidates and values (tpq_ivfflat_range_count / _fill) follows the scan.
#include "scan_device.h"
#include "scan_ref.h"

namespace tpq {
namespace flat {

constexpr int kFlatUnroll = 8;  // row loads in flight per lane: 8 x 256 B per wave, 16 waves per CU = 32 KiB per CU

struct FlatArgs {
  const float* vectors;  // [d][n_slots]
  int d;
};

__host__ __device__ constexpr size_t query_bytes(int d) { return align16((size_t)d * 4); }

// the value of scan_flat_kernel: `col` is component 0 of the slot, rows are `stride` floats apart; GROUPS groups of
// kFlatUnroll rows per trip (the order of the sum is the same whatever GROUPS is)
template <int METRIC, int GROUPS = 2>
__device__ __forceinline__ float slot_value(const float* __restrict__ col, const float* xq, int d, int64_t stride) {
  float v = 0.f;
  int i = 0;
  // two groups of kFlatUnroll rows per trip is what the compiler makes of the unmasked scan_flat_kernel's loop on its
  // own; left alone it unrolled the inner-product fill kernel further, to 78 VGPRs (44 / 48 with this,
  // tools/kernel_regs.py).  The masked scan takes one group: 61 - 71 VGPRs, seven waves per SIMD, against 73 - 81.
#pragma unroll GROUPS
  for (; i + kFlatUnroll <= d; i += kFlatUnroll) {
    float x[kFlatUnroll];
#pragma unroll
    for (int u = 0; u < kFlatUnroll; ++u) x[u] = col[(int64_t)u * stride];
    col += (int64_t)kFlatUnroll * stride;
#pragma unroll
    for (int u = 0; u < kFlatUnroll; ++u) v = metric_step<METRIC>(v, xq[i + u], x[u]);
  }
  for (; i < d; ++i) {
    v = metric_step<METRIC>(v, xq[i], *col);
    col += stride;
  }
  return v;
}

// ---- the masked scan: is_empty != nullptr -----------------------------------------------------------------------------
// The mask is any set of slots to skip -- the container's tombstones, or those OR-ed with a filter's complement -- so
// it may be dense.  A lane reads the mask byte of its slot BEFORE any row of the vector, kMaskTilesAhead tiles' bytes in
// flight together, and the wave ballots:
//   no live slot                 the tile reads no vector
//   kCompactBelow live or more   the tile is valued in place, as the unmasked scan values it; its dead lanes load nothing
//   fewer                        the live slots are appended to the wave's pending list (Pending, scan_list.h); whenever
//                                64 are pending the wave takes 64 and every lane values one slot; the rest is drained
//                                after the wave's last tile
// Keys are (value, address): the order in which slots reach the selector does not change the result.
// kCompactBelow is measured: compacting every partial tile cost 14 % at a mask that is 99 % live and 17 %
// at 50 %, where nearly every 128-byte line of a tile holds a live slot anyway; compacting none cost 64 % at 0.1 %,
// where a tile that is not empty holds one live slot and a wave would run its d row loads for that lane alone.
constexpr int kMaskTilesAhead = 4;  // tiles whose mask bytes are loaded together
constexpr int kCompactBelow = 4;    // a tile with fewer live slots than this is compacted

// `count` pending slots are valued, one per lane, and go through the admission step
template <int R, int METRIC>
__device__ __forceinline__ void value_pending(const FlatArgs& f, const float* xq, int64_t stride, Pending& pend,
                                              int count, WaveSelector<R>& sel, unsigned* tau_key) {
  const int s = pend.take(count);
  const bool live = lane_id() < count;
  float v = 0.f;
  if (live) v = slot_value<METRIC, 1>(f.vectors + s, xq, f.d, stride);
  admit(sel, tau_key, live, v, s);
}

// LDS: [query d floats | the finisher's merge lists, which start once the scan is over][queues][probe table][threshold]
// and, MASKED, the pending lists (8 waves x 128 slots = 4 KiB) behind them
template <int R, int METRIC, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void scan_flat_kernel(ScanArgs a, FlatArgs f, size_t region0) {
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
  for (int i = threadIdx.x; i < d; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);

  const TileRange t = part_tiles(lds.tab.tile_begin[n_probe], part, a.n_split);
  const int64_t stride = a.n_slots;

  int p = 0;
  if constexpr (MASKED) {
    Pending pend{reinterpret_cast<int*>(lds.tail) + wave * kPendingPerWave, 0};
    for (int T0 = t.begin + wave; T0 < t.end; T0 += kScanWaves * kMaskTilesAhead) {
      // a tile's first slot and how many of its lanes lie inside the cell: the same for every lane, so kept as scalars
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
      unsigned long long live_mask[kMaskTilesAhead], valid_mask[kMaskTilesAhead];  // (uniform)
      {
        uint8_t dead[kMaskTilesAhead];
#pragma unroll
        for (int u = 0; u < kMaskTilesAhead; ++u) {
          const int s = first[u] + lane;
          const bool valid = lane < inside[u] && s >= 0 && (int64_t)s < a.n_slots;  // (a cell that leaves the storage is cut)
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
        if (live_mask[u] != valid_mask[u] && __popcll(live_mask[u]) < kCompactBelow) {  // a sparse tile: its live slots wait until 64 are pending
          pend.append(live, s);
          if (pend.n < 64) continue;
          s = pend.take(64);
          live = true;
        }
        // a tile is valued in place, as the unmasked scan values it; 64 pending slots one per lane
        float v = 0.f;
        if (live) v = slot_value<METRIC, 1>(f.vectors + s, xq, d, stride);
        admit(sel, lds.tau_key, live, v, s);
      }
    }
    if (pend.n > 0) value_pending<R, METRIC>(f, xq, stride, pend, pend.n, sel, lds.tau_key);
  } else {
    for (int T = t.begin + wave; T < t.end; T += kScanWaves) {
      p = probe_of(lds.tab, p, T);
      const Tile tile = tile_at(lds.tab, p, T, lane);
      const int s = tile.slot();
      const bool valid = tile.in_cell() && s >= 0 && (int64_t)s < a.n_slots;  // (a cell that leaves the storage is cut)
      float v = 0.f;
      bool live = valid;
      if (valid) {
        // (never taken: a call with a mask runs the MASKED form.  The test stays so that this form compiles to the
        // instructions it had before there was another)
        if (a.is_empty) live = (a.is_empty[s] == 0);
        // (the loop of slot_value above, written out: with that function's `#pragma unroll 2` this kernel compiles to
        // other code)
        const float* __restrict__ col = f.vectors + s;
        int i = 0;
        for (; i + kFlatUnroll <= d; i += kFlatUnroll) {
          float x[kFlatUnroll];
#pragma unroll
          for (int u = 0; u < kFlatUnroll; ++u) x[u] = col[(int64_t)u * stride];
          col += (int64_t)kFlatUnroll * stride;
#pragma unroll
          for (int u = 0; u < kFlatUnroll; ++u) v = metric_step<METRIC>(v, xq[i + u], x[u]);
        }
        for (; i < d; ++i) {
          v = metric_step<METRIC>(v, xq[i], *col);
          col += stride;
        }
      }
      admit(sel, lds.tau_key, live, v, s);
    }
  }
  sel.flush();
  finish_list_scan<R>(a, q, part, sel.top, smem);
}

template <int METRIC>
static int dispatch(const ScanArgs& a, const FlatArgs& f, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    const size_t region0 = list_region0(query_bytes(f.d), RC);
    if (a.is_empty)
      return launch_list_scan(scan_flat_kernel<RC, METRIC, true>, scan_merge_kernel<RC>, "scan_flat_kernel (masked)", a,
                              list_scan_lds_bytes(region0, a.max_nprobe, kPendingBytes), st, f, region0);
    return launch_list_scan(scan_flat_kernel<RC, METRIC, false>, scan_merge_kernel<RC>, "scan_flat_kernel", a,
                            list_scan_lds_bytes(region0, a.max_nprobe, 0), st, f, region0);
  });
}

// ---- range search (tpq_ivfflat_range_count / tpq_ivfflat_range_fill) -------------------------------------------
// Every candidate of the top-k scan whose value is >= the query's threshold, in scan order.  Two passes over the
// same tiles: range_count_kernel counts a wave's hits, the caller turns the counts into offsets, range_fill_kernel
// computes the values again -- the same code, so the same bits -- and appends each wave's hits at its offset
// (Segment, scan_list.h).  No global atomic, no sort.  Workgroup, probe table and the part's tile range are
// scan_flat_kernel's; inside the part a wave owns a CONTIGUOUS chunk of the tiles, not every eighth one, so the
// segments in (query, part, wave) order are tile-ascending whatever n_split is.  LDS: the query and the probe table.

static size_t range_lds_bytes(int d, int max_nprobe) { return query_bytes(d) + probe_table_bytes(max_nprobe); }

// One pass of one (query, part).  A NaN value and a NaN threshold fail `v >= thr`.
template <int METRIC, bool FILL>
__device__ __forceinline__ void range_body(const ScanArgs& a, const FlatArgs& f, const RangeArgs& r, char* smem) {
  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int64_t seg = (int64_t)blockIdx.x * kScanWaves;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  if (Segment<FILL>::no_hit(r, seg)) return;
  Segment<FILL> out(r, seg, wave);
  // the query and the probe table (every thread of the workgroup gets here: the barrier)
  float* xq = reinterpret_cast<float*>(smem);
  const ProbeTable tab = probe_table_at(smem + query_bytes(f.d), a.max_nprobe);
  const int n_probe = clamped_n_probe(a, q);
  if (wave == 0) build_probe_table(a, q, n_probe, tab);
  for (int i = threadIdx.x; i < f.d; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
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
    const bool valid = tile.in_cell() && s >= 0 && (int64_t)s < a.n_slots;  // (a cell that leaves the storage is cut)
    bool hit = false;
    float v = 0.f;
    if (valid && !(a.is_empty && a.is_empty[s] != 0)) {
      v = slot_value<METRIC>(f.vectors + s, xq, f.d, a.n_slots);
      hit = v >= thr;
    }
    out.emit(a, hit, v, s);  // once per tile, wave-uniformly
  }
  out.close(r, seg, wave);
}

template <int METRIC>
__global__ __launch_bounds__(kScanThreads) void range_count_kernel(ScanArgs a, FlatArgs f, RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  range_body<METRIC, false>(a, f, r, smem);
}

template <int METRIC>
__global__ __launch_bounds__(kScanThreads) void range_fill_kernel(ScanArgs a, FlatArgs f, RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  range_body<METRIC, true>(a, f, r, smem);
}

template <int METRIC>
static int launch_range(const ScanArgs& a, const FlatArgs& f, const RangeArgs& r, hipStream_t st) {
  const size_t lds = range_lds_bytes(f.d, a.max_nprobe);
  const bool fill = r.wave_offsets != nullptr;
  const char* name = fill ? "range_fill_kernel" : "range_count_kernel";
  if (int rc = check_lds(name, lds)) return rc;
  const dim3 grid((unsigned)a.nq * a.n_split), block(kScanThreads);
  return fill ? launch_with_lds(range_fill_kernel<METRIC>, name, grid, block, lds, st, a, f, r)
              : launch_with_lds(range_count_kernel<METRIC>, name, grid, block, lds, st, a, f, r);
}

// the arguments of the three entry points, once their checks have passed
static ScanArgs flat_args(const float* query, const uint8_t* is_empty, const int64_t* cell_start,
                          const int64_t* cell_size, const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                          int64_t n_slots, int nq, int max_nprobe, int k, int n_split) {
  ScanArgs a = scan_args(nullptr, nullptr, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         nullptr, nullptr, n_slots, nq, max_nprobe, 0, k, n_split);
  a.query = query;
  return a;
}

// what tpq_ivfflat_range_count and tpq_ivfflat_range_fill share: the checks of tpq_ivfflat_scan_topk (all of them
// before any HIP call), then the launch -- the fill pass when `fill`
static int range_pass(const char* what, const float* vectors, const float* query, const uint8_t* is_empty,
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
  const ScanArgs a = flat_args(query, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr, n_slots, nq,
                               max_nprobe, 0, n_split);
  const FlatArgs f{vectors, d};
  const RangeArgs r{threshold, wave_counts, fill ? wave_offsets : nullptr};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? launch_range<TPQ_METRIC_NEG_SQ_L2>(a, f, r, st)
                                        : launch_range<TPQ_METRIC_INNER>(a, f, r, st);
}

}  // namespace flat
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfflat_scan_workspace_bytes(int nq, int k, int n_split) {
  if (nq <= 0 || k <= 0 || k > 1024) return 0;
  return list_ws_bytes(nq, list_regs(k), n_split);
}

extern "C" int tpq_ivfflat_scan_topk(const float* vectors, const float* query, const uint8_t* is_empty,
                                     const int64_t* cell_start, const int64_t* cell_size,
                                     const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                     int64_t n_slots, int d, int nq, int max_nprobe, int k, int metric, int n_split,
                                     void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  const char* what = "ivfflat_scan";
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  TPQ_REQUIRE(d >= 1, "ivfflat_scan: d=%d", d);
  TPQ_REQUIRE(k >= 1 && k <= 1024, "ivfflat_scan: k=%d out of range (0, 1024]", k);
  if (int rc = check_lists(what, metric, n_split, n_slots)) return rc;
  if (nq == 0) return TPQ_OK;
  if (int rc = check_grid(what, vectors && query && cell_start && cell_size && n_probe_list && out_vals && out_addr, nq,
                          n_split))
    return rc;
  const int R = list_regs(k);
  ScanArgs a = flat::flat_args(query, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr, n_slots, nq,
                               max_nprobe, k, n_split);
  if (int rc = take_list_ws(a, R, workspace, workspace_bytes, what)) return rc;
  const flat::FlatArgs f{vectors, d};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? flat::dispatch<TPQ_METRIC_NEG_SQ_L2>(a, f, R, st)
                                        : flat::dispatch<TPQ_METRIC_INNER>(a, f, R, st);
}

extern "C" size_t tpq_ivfflat_range_segments(int nq, int n_split) {
  if (nq <= 0 || n_split < 1 || n_split > 1024) return 0;
  return (size_t)nq * n_split * kScanWaves;
}

extern "C" int tpq_ivfflat_range_count(const float* vectors, const float* query, const uint8_t* is_empty,
                                       const int64_t* cell_start, const int64_t* cell_size,
                                       const int64_t* n_probe_list, const float* threshold, int32_t* wave_counts,
                                       int64_t n_slots, int d, int nq, int max_nprobe, int metric, int n_split,
                                       tpq_stream_t stream) {
  return flat::range_pass("ivfflat_range_count", vectors, query, is_empty, cell_start, cell_size, n_probe_list,
                          threshold, wave_counts, nullptr, nullptr, nullptr, false, n_slots, d, nq, max_nprobe,
                          metric, n_split, stream);
}

extern "C" int tpq_ivfflat_range_fill(const float* vectors, const float* query, const uint8_t* is_empty,
                                      const int64_t* cell_start, const int64_t* cell_size,
                                      const int64_t* n_probe_list, const float* threshold,
                                      const int64_t* wave_offsets, float* out_vals, int64_t* out_addr,
                                      int64_t n_slots, int d, int nq, int max_nprobe, int metric, int n_split,
                                      tpq_stream_t stream) {
  return flat::range_pass("ivfflat_range_fill", vectors, query, is_empty, cell_start, cell_size, n_probe_list,
                          threshold, nullptr, wave_offsets, out_vals, out_addr, true, n_slots, d, nq, max_nprobe,
                          metric, n_split, stream);
}
