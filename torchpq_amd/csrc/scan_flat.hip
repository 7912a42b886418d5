// List scan of IVFFlatIndex (tpq_ivfflat_scan_topk): the probed cells hold the vectors themselves.
//
// The container stores a vector of d floats as 4 d code bytes, so the storage read as fp32 is dimension-major and
// slot-contiguous: vectors[i * n_slots + s] is component i of slot s.  One workgroup per (query, part), eight waves,
// as scan_ref_kernel (scan_ref.h): the query lies in LDS (d floats), a wave takes the 64-slot tiles of the probed
// cells round-robin, a lane owns one slot of the tile and walks the dimensions in ascending order -- a wave reads 256
// contiguous bytes per dimension, kFlatUnroll rows in flight -- and the value goes through the per-wave selector and
// the workgroup-shared threshold of the code scans.  The summation order of the value definition
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

// LDS: [query d floats | the finisher's merge lists, which start once the scan is over][queues][probe table][threshold]
static size_t region0_bytes(int d, int R) {
  const size_t q = ((size_t)d * 4 + 15) & ~(size_t)15, lists = (size_t)kScanWaves * R * 64 * 8;
  return q > lists ? q : lists;
}
static size_t lds_bytes(int d, int R, int max_nprobe) {
  const size_t b = region0_bytes(d, R) + kScanWaves * 512 + (size_t)(3 * max_nprobe + 1) * 4 + 4;
  return (b + 15) & ~(size_t)15;
}
static size_t ws_bytes(int nq, int R, int n_split) {
  return n_split > 1 ? (size_t)nq * n_split * R * 64 * 8 : 0;
}

template <int METRIC>
__device__ __forceinline__ float step(float acc, float q, float x) {
  if constexpr (METRIC == TPQ_METRIC_NEG_SQ_L2) {
    const float t = __fsub_rn(q, x);
    return __fsub_rn(acc, __fmul_rn(t, t));
  } else {
    return __fadd_rn(acc, __fmul_rn(q, x));
  }
}

template <int R, int METRIC>
__global__ __launch_bounds__(kScanThreads) void scan_flat_kernel(ScanArgs a, FlatArgs f, size_t region0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xq = reinterpret_cast<float*>(smem);
  float* qv_all = reinterpret_cast<float*>(smem + region0);
  int* qi_all = reinterpret_cast<int*>(smem + region0 + kScanWaves * 256);
  int* ptab = reinterpret_cast<int*>(smem + region0 + kScanWaves * 512);
  ProbeTable tab{ptab, ptab + a.max_nprobe, ptab + 2 * a.max_nprobe};
  unsigned* tau_key = reinterpret_cast<unsigned*>(ptab + 3 * a.max_nprobe + 1);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int d = f.d;
  int n_probe = (int)a.n_probe_list[q];
  n_probe = n_probe < 0 ? 0 : (n_probe > a.max_nprobe ? a.max_nprobe : n_probe);

  if (wave == 0) {
    build_probe_table(a, q, n_probe, tab);
    if (lane == 0) *tau_key = f2key(-INFINITY);
  }
  for (int i = threadIdx.x; i < d; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(qv_all + wave * 64, qi_all + wave * 64, a.k);

  const int total_tiles = tab.tile_begin[n_probe];
  const int t_begin = (int)(((int64_t)total_tiles * part) / a.n_split);
  const int t_end = (int)(((int64_t)total_tiles * (part + 1)) / a.n_split);
  const int64_t stride = a.n_slots;

  int p = 0;
  for (int T = t_begin + wave; T < t_end; T += kScanWaves) {
    while (T >= tab.tile_begin[p + 1]) ++p;
    const int off = ((T - tab.tile_begin[p]) << 6) + lane;
    const int s = tab.start[p] + off;
    const bool valid = off < tab.size[p] && s >= 0 && (int64_t)s < a.n_slots;  // (a cell that leaves the storage is cut)
    float v = 0.f;
    bool live = valid;
    if (valid) {
      if (a.is_empty) live = (a.is_empty[s] == 0);
      const float* __restrict__ col = f.vectors + s;
      int i = 0;
      for (; i + kFlatUnroll <= d; i += kFlatUnroll) {
        float x[kFlatUnroll];
#pragma unroll
        for (int u = 0; u < kFlatUnroll; ++u) x[u] = col[(int64_t)u * stride];
        col += (int64_t)kFlatUnroll * stride;
#pragma unroll
        for (int u = 0; u < kFlatUnroll; ++u) v = step<METRIC>(v, xq[i + u], x[u]);
      }
      for (; i < d; ++i) {
        v = step<METRIC>(v, xq[i], *col);
        col += stride;
      }
    }
    // workgroup-shared admission threshold, as scan_ref_kernel; a NaN value fails `v >= tau` and never enters
    const float tau_s = key2f(lds_poll_u32(tau_key));
    sel.tau = fmaxf(sel.tau, tau_s);
    const float tau_before = sel.tau;
    sel.push(live && (v >= sel.tau), v, s);
    if (sel.tau > tau_before && lane == 0) atomicMax(tau_key, f2key(sel.tau));
  }
  sel.flush();
  finish_query<R>(a, q, part, sel.top, reinterpret_cast<float*>(smem),
                  reinterpret_cast<int*>(smem + kScanWaves * R * 64 * 4));
}

template <int R, int METRIC>
static int launch(const ScanArgs& a, const FlatArgs& f, hipStream_t st) {
  const size_t lds = lds_bytes(f.d, R, a.max_nprobe);
  int rc = set_lds(scan_flat_kernel<R, METRIC>, lds, "scan_flat_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((scan_flat_kernel<R, METRIC>), dim3((unsigned)a.nq * a.n_split), dim3(kScanThreads), lds, st, a,
                     f, region0_bytes(f.d, R));
  TPQ_LAUNCH_CHECK("scan_flat_kernel");
  if (a.n_split > 1) {
    hipLaunchKernelGGL(scan_merge_kernel<R>, dim3(a.nq), dim3(64), 0, st, a);
    TPQ_LAUNCH_CHECK("scan_merge_kernel");
  }
  return TPQ_OK;
}

template <int METRIC>
static int dispatch(const ScanArgs& a, const FlatArgs& f, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) { return launch<decltype(r_c)::value, METRIC>(a, f, st); });
}

// ---- range search (tpq_ivfflat_range_count / tpq_ivfflat_range_fill) -------------------------------------------
// Every candidate of the top-k scan whose value is >= the query's threshold, in scan order.  Two passes over the
// same tiles: range_count_kernel counts a wave's hits, the caller turns the counts into offsets, range_fill_kernel
// computes the values again -- the same code, so the same bits -- and appends each wave's hits at its offset.  No
// global atomic, no sort.  Workgroup, probe table and the part's tile range [t_begin, t_end) are scan_flat_kernel's;
// inside the part a wave owns a CONTIGUOUS chunk of the tiles, not every eighth one, so the segments in
// (query, part, wave) order are tile-ascending whatever n_split is.  LDS: the query and the probe table.

struct RangeArgs {
  const float* threshold;       // [nq]
  int* wave_counts;             // count pass: [nq][n_split][kScanWaves]
  const int64_t* wave_offsets;  // fill pass: [nq * n_split * kScanWaves + 1] exclusive prefix sums of the counts
};

static size_t range_lds_bytes(int d, int max_nprobe) {
  return (((size_t)d * 4 + 15) & ~(size_t)15) + (size_t)(3 * max_nprobe + 1) * 4;
}

// the value of scan_flat_kernel: `col` is component 0 of the slot, rows are `stride` floats apart
template <int METRIC>
__device__ __forceinline__ float slot_value(const float* __restrict__ col, const float* xq, int d, int64_t stride) {
  float v = 0.f;
  int i = 0;
  // two groups of kFlatUnroll rows per trip, which is what the compiler makes of scan_flat_kernel's loop on its own;
  // left alone it unrolled the inner-product fill kernel further, to 78 VGPRs (44 / 48 with this, tools/kernel_regs.py)
#pragma unroll 2
  for (; i + kFlatUnroll <= d; i += kFlatUnroll) {
    float x[kFlatUnroll];
#pragma unroll
    for (int u = 0; u < kFlatUnroll; ++u) x[u] = col[(int64_t)u * stride];
    col += (int64_t)kFlatUnroll * stride;
#pragma unroll
    for (int u = 0; u < kFlatUnroll; ++u) v = step<METRIC>(v, xq[i + u], x[u]);
  }
  for (; i < d; ++i) {
    v = step<METRIC>(v, xq[i], *col);
    col += stride;
  }
  return v;
}

// A wave's share of a (query, part): its contiguous chunk [T0, T1) of the part's tiles, over the staged query and table
struct RangeChunk {
  ProbeTable tab;
  const float* xq;
  int T0, T1;
  float thr;
};

// Stages the query and the probe table in LDS (every thread of the workgroup calls it: it holds the barrier)
__device__ __forceinline__ RangeChunk range_stage(const ScanArgs& a, const FlatArgs& f, const RangeArgs& r, char* smem,
                                                  int q, int part) {
  float* xq = reinterpret_cast<float*>(smem);
  int* ptab = reinterpret_cast<int*>(smem + (((size_t)f.d * 4 + 15) & ~(size_t)15));
  const ProbeTable tab{ptab, ptab + a.max_nprobe, ptab + 2 * a.max_nprobe};
  const int wave = threadIdx.x >> 6;
  int n_probe = (int)a.n_probe_list[q];
  n_probe = n_probe < 0 ? 0 : (n_probe > a.max_nprobe ? a.max_nprobe : n_probe);
  if (wave == 0) build_probe_table(a, q, n_probe, tab);
  for (int i = threadIdx.x; i < f.d; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  __syncthreads();
  const int total_tiles = tab.tile_begin[n_probe];
  const int t_begin = (int)(((int64_t)total_tiles * part) / a.n_split);
  const int t_end = (int)(((int64_t)total_tiles * (part + 1)) / a.n_split);
  const int n_tiles = t_end - t_begin;
  return RangeChunk{tab, xq, t_begin + (int)(((int64_t)n_tiles * wave) / kScanWaves),
                    t_begin + (int)(((int64_t)n_tiles * (wave + 1)) / kScanWaves), r.threshold[q]};
}

// Walks the chunk: emit(hit, value, slot) once per tile, wave-uniformly.  A NaN value and a NaN threshold fail `v >= thr`.
template <int METRIC, class Emit>
__device__ __forceinline__ void range_tiles(const ScanArgs& a, const FlatArgs& f, const RangeChunk& c, Emit emit) {
  const int lane = lane_id();
  int p = 0;
  for (int T = c.T0; T < c.T1; ++T) {
    while (T >= c.tab.tile_begin[p + 1]) ++p;
    const int off = ((T - c.tab.tile_begin[p]) << 6) + lane;
    const int s = c.tab.start[p] + off;
    const bool valid = off < c.tab.size[p] && s >= 0 && (int64_t)s < a.n_slots;  // (a cell that leaves the storage is cut)
    bool hit = false;
    float v = 0.f;
    if (valid && !(a.is_empty && a.is_empty[s] != 0)) {
      v = slot_value<METRIC>(f.vectors + s, c.xq, f.d, a.n_slots);
      hit = v >= c.thr;
    }
    emit(hit, v, s);
  }
}

template <int METRIC>
__global__ __launch_bounds__(kScanThreads) void range_count_kernel(ScanArgs a, FlatArgs f, RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const RangeChunk c = range_stage(a, f, r, smem, q, part);
  int n = 0;
  range_tiles<METRIC>(a, f, c, [&](bool hit, float, int) { n += __popcll(__ballot(hit)); });
  if (lane_id() == 0) r.wave_counts[(int64_t)blockIdx.x * kScanWaves + (threadIdx.x >> 6)] = n;
}

template <int METRIC>
__global__ __launch_bounds__(kScanThreads) void range_fill_kernel(ScanArgs a, FlatArgs f, RangeArgs r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int64_t seg = (int64_t)blockIdx.x * kScanWaves;
  // a workgroup without a hit leaves before it stages anything (the same two words for every thread: uniform)
  if (r.wave_offsets[seg + kScanWaves] <= r.wave_offsets[seg]) return;
  const int wave = threadIdx.x >> 6;
  int64_t pos = r.wave_offsets[seg + wave];
  // what the count pass saw is all this wave may write: with other inputs than the count pass had (or offsets that are
  // not its prefix sums) hits are dropped, never stored at or beyond the next segment's offset
  const int64_t end = r.wave_offsets[seg + wave + 1];
  const RangeChunk c = range_stage(a, f, r, smem, q, part);
  if (pos < 0 || end <= pos) return;  // an empty segment: no vector is read
  range_tiles<METRIC>(a, f, c, [&](bool hit, float v, int s) {
    const unsigned long long mask = __ballot(hit);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
    const int64_t o = pos + rank;
    if (hit && o < end) {
      a.out_vals[o] = v;
      a.out_addr[o] = (int64_t)s;
    }
    pos += __popcll(mask);
  });
}

template <int METRIC>
static int launch_range(const ScanArgs& a, const FlatArgs& f, const RangeArgs& r, hipStream_t st) {
  const size_t lds = range_lds_bytes(f.d, a.max_nprobe);
  const bool fill = r.wave_offsets != nullptr;
  const char* name = fill ? "range_fill_kernel" : "range_count_kernel";
  if (int rc = fill ? set_lds(range_fill_kernel<METRIC>, lds, name) : set_lds(range_count_kernel<METRIC>, lds, name))
    return rc;
  const dim3 grid((unsigned)a.nq * a.n_split), block(kScanThreads);
  if (fill)
    hipLaunchKernelGGL(range_fill_kernel<METRIC>, grid, block, lds, st, a, f, r);
  else
    hipLaunchKernelGGL(range_count_kernel<METRIC>, grid, block, lds, st, a, f, r);
  TPQ_LAUNCH_CHECK(name);
  return TPQ_OK;
}

// what tpq_ivfflat_range_count and tpq_ivfflat_range_fill share: the checks of tpq_ivfflat_scan_topk (all of them
// before any HIP call), then the launch -- the fill pass when `fill`
static int range_pass(const char* what, const float* vectors, const float* query, const uint8_t* is_empty,
                      const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                      const float* threshold, int* wave_counts, const int64_t* wave_offsets, float* out_vals,
                      int64_t* out_addr, bool fill, int64_t n_slots, int d, int nq, int max_nprobe, int metric,
                      int n_split, tpq_stream_t stream) {
  TPQ_REQUIRE(nq >= 0 && max_nprobe >= 1, "%s: bad nq/max_nprobe (%d, %d)", what, nq, max_nprobe);
  TPQ_REQUIRE(d >= 1, "%s: d=%d", what, d);
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "%s: metric=%d", what, metric);
  TPQ_REQUIRE(n_split >= 1 && n_split <= 1024, "%s: n_split=%d out of range", what, n_split);
  TPQ_REQUIRE(n_slots >= 0, "%s: n_slots=%lld", what, (long long)n_slots);
  if (n_slots >= (int64_t)kPadIdx) {
    set_error("%s: n_slots=%lld >= 2^31-1 is not supported", what, (long long)n_slots);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (nq == 0) return TPQ_OK;
  TPQ_REQUIRE(vectors && query && cell_start && cell_size && n_probe_list && threshold &&
                  (fill ? (wave_offsets && out_vals && out_addr) : wave_counts != nullptr),
              "%s: null pointer argument", what);
  TPQ_REQUIRE((int64_t)nq * n_split < 0x7fffffffLL, "%s: nq * n_split = %lld workgroups", what,
              (long long)nq * n_split);
  ScanArgs a{};
  a.query = query;
  a.is_empty = is_empty;
  a.cell_start = cell_start;
  a.cell_size = cell_size;
  a.n_probe_list = n_probe_list;
  a.out_vals = out_vals;
  a.out_addr = out_addr;
  a.n_slots = n_slots;
  a.nq = nq;
  a.max_nprobe = max_nprobe;
  a.n_split = n_split;
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
  return flat::ws_bytes(nq, list_regs(k), n_split);
}

extern "C" int tpq_ivfflat_scan_topk(const float* vectors, const float* query, const uint8_t* is_empty,
                                     const int64_t* cell_start, const int64_t* cell_size,
                                     const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                     int64_t n_slots, int d, int nq, int max_nprobe, int k, int metric, int n_split,
                                     void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(nq >= 0 && max_nprobe >= 1, "ivfflat_scan: bad nq/max_nprobe (%d, %d)", nq, max_nprobe);
  TPQ_REQUIRE(d >= 1, "ivfflat_scan: d=%d", d);
  TPQ_REQUIRE(k >= 1 && k <= 1024, "ivfflat_scan: k=%d out of range (0, 1024]", k);
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "ivfflat_scan: metric=%d", metric);
  TPQ_REQUIRE(n_split >= 1 && n_split <= 1024, "ivfflat_scan: n_split=%d out of range", n_split);
  TPQ_REQUIRE(n_slots >= 0, "ivfflat_scan: n_slots=%lld", (long long)n_slots);
  if (n_slots >= (int64_t)kPadIdx) {
    set_error("ivfflat_scan: n_slots=%lld >= 2^31-1 is not supported", (long long)n_slots);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (nq == 0) return TPQ_OK;
  TPQ_REQUIRE(vectors && query && cell_start && cell_size && n_probe_list && out_vals && out_addr,
              "ivfflat_scan: null pointer argument");
  TPQ_REQUIRE((int64_t)nq * n_split < 0x7fffffffLL, "ivfflat_scan: nq * n_split = %lld workgroups",
              (long long)nq * n_split);
  const int R = list_regs(k);
  const size_t need = flat::ws_bytes(nq, R, n_split);
  if (int rc = need_ws(workspace, workspace_bytes, need, "ivfflat_scan")) return rc;
  ScanArgs a{};
  a.query = query;
  a.is_empty = is_empty;
  a.cell_start = cell_start;
  a.cell_size = cell_size;
  a.n_probe_list = n_probe_list;
  a.out_vals = out_vals;
  a.out_addr = out_addr;
  a.n_slots = n_slots;
  a.nq = nq;
  a.max_nprobe = max_nprobe;
  a.k = k;
  a.n_split = n_split;
  if (need) {
    a.ws_vals = reinterpret_cast<float*>(workspace);
    a.ws_idx = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + need / 2);
  }
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
