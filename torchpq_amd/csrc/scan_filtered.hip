// Filtered top-k over the lists of IVFPQIndex (tpq_ivfpq_scan_filtered_topk / _residual_topk, tpq_slot_filter_build,
// DESIGN 3.14): the k best candidates of the top-k scan AMONG the slots a filter allows.
//
// A filter is a row of bits over the slot addresses, bit s & 31 of word s >> 5 for slot s; every query names its row.
// Candidates are those of the range search (scan_range.hip): the slots of the probed cells inside the storage that are
// not tombstoned -- and whose bit is set.  The value is that of the exact reference-layout kernels (scan_ref.h), bit
// for bit; the selection is theirs (WaveSelector, the workgroup-shared threshold, the split merge).
//
// What differs is the tile loop, which tests a slot's bit BEFORE it touches the slot's m bytes of code:
//   membership  a lane reads the filter word of its slot of the tile (two or three distinct words per wave), the
//               tombstone byte only where the bit is set, and the wave ballots; kTilesAhead tiles' words are in flight
//               together.  A tile without an allowed live slot reads no code.
//   compaction  the allowed slots are appended, by ballot and mbcnt rank, to a list of pending slots the wave owns in
//               LDS (no barrier); whenever 64 or more are pending the wave takes 64 and every lane values one slot --
//               the look-ups run on full waves however sparse the filter is.  Plain PQ drains the rest once, after
//               the wave's last tile; residual PQ at the end of every probe, before the barrier that lets the table be
//               rebuilt.
// Keys are (value, address): the order in which slots reach the selector does not change the result.
//
// LDS: the frame of a list kernel (scan_list.h) with, behind it, the pending lists (8 waves x 128 slots = 4 KiB) and the
// staged query when the table is built here.  m KiB of table + 4 KiB of queues + 4 KiB of pending lists + the probe
// table must fit 160 KiB: m <= kMaxM = 148.
#include "scan_ref.h"

namespace tpq {
namespace filtered {

constexpr int kMaxM = 148;      // 148 KiB + 4 KiB + 4 KiB = 156 KiB: 4 KiB left for the probe table and the query
constexpr int kTilesAhead = 4;  // tiles whose filter words (then tombstone bytes) are loaded together
constexpr int kRowGroup = 4;    // row loads in flight per lane, as scan_ref_kernel's group

// The value of scan_ref_kernel / scan_residual_kernel (and of pqrange::slot_value, scan_range.hip): v starts at `v` and
// adds lut[j][code_j] for j ascending, one fp32 add each.  `col` is the slot's dword of row 0, rows `stride` dwords apart.
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

// `count` pending slots are valued, one per lane, and go through the admission step
template <int R, bool RESIDUAL>
__device__ __forceinline__ void value_pending(const ScanArgs& a, const float* lut, Pending& pend, int count,
                                              WaveSelector<R>& sel, unsigned* tau_key, float base) {
  const int s = pend.take(count);
  const bool live = lane_id() < count;
  float v = base;
  if (live) v = slot_value(reinterpret_cast<const uint32_t*>(a.codes) + s, a.n_slots, lut, a.m >> 2, base);
  // (residual: the test is on the raw v, what enters is canonical, as scan_residual_kernel pushes it)
  admit(sel, tau_key, live, v, s, RESIDUAL ? v + 0.0f : v);
}

// kTilesAhead tiles of one wave: their members (the filter words' loads together), the tombstones of the members, the
// appends; 64 pending slots are valued as soon as they are there
template <int R, bool RESIDUAL>
__device__ __forceinline__ void admit_members(const ScanArgs& a, const float* lut, Member (&mb)[kTilesAhead],
                                              Pending& pend, WaveSelector<R>& sel, unsigned* tau_key, float base) {
  if (a.is_empty) {
#pragma unroll
    for (int u = 0; u < kTilesAhead; ++u)
      if (mb[u].ok) mb[u].ok = a.is_empty[mb[u].s] == 0;
  }
#pragma unroll
  for (int u = 0; u < kTilesAhead; ++u) {
    pend.append(mb[u].ok, mb[u].s);
    if (pend.n >= 64) value_pending<R, RESIDUAL>(a, lut, pend, 64, sel, tau_key, base);
  }
}

// ---- plain PQ ----------------------------------------------------------------------------------------------------
// LDS tail: [pending 8 x 128][query m * ds floats, when the table is built in the workgroup]
template <int R>
__global__ __launch_bounds__(kScanThreads) void scan_filtered_kernel(ScanArgs a, FilterArgs f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ListLds lds(smem, list_region0<size_t>((size_t)a.m * 1024, R), a.max_nprobe);
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(lds.tail + kPendingBytes);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const uint32_t* __restrict__ row = filter_row(f, q);  // (uniform)
  const int n_probe = row ? clamped_n_probe(a, q) : 0;   // no row: no tile, no table, k pads

  lds.init(a, q, n_probe, wave, lane);
  if (row) {
    if (!a.lut) stage_query(a, q, xq, kScanThreads);
    stage_lut_linear(a, q, lut, xq);
  }
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);
  Pending pend{reinterpret_cast<int*>(lds.tail) + wave * kPendingPerWave, 0};

  const TileRange t = part_tiles(lds.tab.tile_begin[n_probe], part, a.n_split);
  int p = 0;
  for (int T0 = t.begin + wave; T0 < t.end; T0 += kScanWaves * kTilesAhead) {
    Member mb[kTilesAhead];
#pragma unroll
    for (int u = 0; u < kTilesAhead; ++u) {
      const int T = T0 + u * kScanWaves;
      mb[u] = Member{0, false};
      if (T < t.end) {  // (uniform)
        p = probe_of(lds.tab, p, T);
        const Tile tile = tile_at(lds.tab, p, T, lane);
        mb[u] = member(row, tile.start, tile.size, tile.off, a.n_slots);
      }
    }
    admit_members<R, false>(a, lut, mb, pend, sel, lds.tau_key, 0.f);
  }
  if (pend.n > 0) value_pending<R, false>(a, lut, pend, pend.n, sel, lds.tau_key, 0.f);
  sel.flush();
  finish_list_scan<R>(a, q, part, sel.top, smem);
}

// ---- residual PQ -------------------------------------------------------------------------------------------------
// One workgroup per query walks its probes as scan_residual_kernel does: barrier, LUT_p, barrier, the cell's tiles.
// LDS tail: [pending 8 x 128][query m * ds floats, when part1 is built in the workgroup]
template <int R>
__global__ __launch_bounds__(kScanThreads) void scan_filtered_residual_kernel(ScanArgs a, ResidualArgs ra,
                                                                              FilterArgs f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ListLds lds(smem, list_region0<size_t>((size_t)a.m * 1024, R), a.max_nprobe);
  float* lut = reinterpret_cast<float*>(smem);
  float* xq = reinterpret_cast<float*>(lds.tail + kPendingBytes);

  const int q = blockIdx.x;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const uint32_t* __restrict__ row = filter_row(f, q);  // (uniform)
  const int n_probe = row ? clamped_n_probe(a, q) : 0;
  lds.init(a, q, n_probe, wave, lane);
  const bool build_part1 = !ra.full && !ra.part1;
  if (build_part1 && row) stage_query(a, q, xq, kScanThreads);
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);
  Pending pend{reinterpret_cast<int*>(lds.tail) + wave * kPendingPerWave, 0};

  for (int p = 0; p < n_probe; ++p) {
    const int sz = lds.tab.size[p];
    if (sz == 0) continue;  // empty, or the previous probe's start again
    __syncthreads();        // every wave is done with the previous cell's table: its pending slots are drained
    build_residual_lut(a, ra, q, p, lut, xq, build_part1);
    __syncthreads();
    const float base = ra.base_sims[(int64_t)q * a.max_nprobe + p];
    const int start = lds.tab.start[p];
    const int tiles = (sz + 63) >> 6;
    for (int T0 = wave; T0 < tiles; T0 += kScanWaves * kTilesAhead) {
      Member mb[kTilesAhead];
#pragma unroll
      for (int u = 0; u < kTilesAhead; ++u) {
        const int T = T0 + u * kScanWaves;
        mb[u] = Member{0, false};
        if (T < tiles) mb[u] = member(row, start, sz, (T << 6) + lane, a.n_slots);
      }
      admit_members<R, true>(a, lut, mb, pend, sel, lds.tau_key, base);
    }
    if (pend.n > 0) value_pending<R, true>(a, lut, pend, pend.n, sel, lds.tau_key, base);
  }
  sel.flush();
  finish_list_scan<R>(a, q, 0, sel.top, smem);
}

// ---- the bits ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slot_filter_build_kernel(const int64_t* __restrict__ address, int64_t n,
                                                                uint32_t* bits, int64_t n_slots) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t s = address[i];
    if (s >= 0 && s < n_slots) atomicOr(bits + (s >> 5), 1u << (unsigned)(s & 31));
  }
}

// ---- host --------------------------------------------------------------------------------------------------------
// what both entry points check alike, in this order, all of it before any HIP call; *done = 1: nothing to launch
static int check_common(const char* what, bool pointers, const void* filter_bits, int n_filters, int64_t filter_stride,
                        const int64_t* address2id, const int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                        int m, int k, int n_split, int* done) {
  *done = 0;
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  TPQ_REQUIRE(m >= 4 && m % 4 == 0, "%s: n_subvectors=%d must be a positive multiple of 4", what, m);
  TPQ_REQUIRE(k >= 1 && k <= 1024, "%s: k=%d out of range [1, 1024]", what, k);
  TPQ_REQUIRE(n_split >= 1 && n_split <= 1024, "%s: n_split=%d out of range", what, n_split);
  if (int rc = check_n_slots(what, n_slots)) return rc;
  if (m > kMaxM) {
    set_error("%s: n_subvectors=%d > %d: the table, the candidate queues and the pending lists do not fit the 160 KiB "
              "of LDS of a CU", what, m, kMaxM);
    return TPQ_ERR_UNSUPPORTED;
  }
  TPQ_REQUIRE(n_filters >= 1, "%s: n_filters=%d", what, n_filters);
  TPQ_REQUIRE(filter_stride >= (n_slots + 31) / 32, "%s: filter_stride=%lld < ceil(n_slots / 32) = %lld", what,
              (long long)filter_stride, (long long)((n_slots + 31) / 32));
  if (nq == 0) {
    *done = 1;
    return TPQ_OK;
  }
  if (int rc = check_grid(what, pointers && filter_bits, nq, n_split)) return rc;
  TPQ_REQUIRE(!out_ids || address2id, "%s: out_ids needs address2id", what);
  return TPQ_OK;
}

}  // namespace filtered
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq_scan_filtered_workspace_bytes(int nq, int k, int n_split) {
  if (nq <= 0 || k <= 0 || k > 1024 || n_split < 1 || n_split > 1024) return 0;
  return list_ws_bytes(nq, list_regs(k), n_split);
}

extern "C" int tpq_ivfpq_scan_filtered_topk(const uint8_t* codes, const float* lut, const float* query,
                                            const float* codebook, int ds, int metric, const uint8_t* is_empty,
                                            const int64_t* cell_start, const int64_t* cell_size,
                                            const int64_t* n_probe_list, const uint32_t* filter_bits,
                                            const int32_t* filter_of_query, int n_filters, int64_t filter_stride,
                                            float* out_vals, int64_t* out_addr, const int64_t* address2id,
                                            int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe, int m, int k,
                                            int n_split, void* workspace, size_t workspace_bytes,
                                            tpq_stream_t stream) {
  const char* what = "ivfpq_scan_filtered";
  int done;
  if (int rc = filtered::check_common(what, codes && cell_start && cell_size && n_probe_list && out_vals && out_addr,
                                      filter_bits, n_filters, filter_stride, address2id, out_ids, n_slots, nq,
                                      max_nprobe, m, k, n_split, &done))
    return rc;
  if (done) return TPQ_OK;
  TPQ_REQUIRE(lut || (query && codebook), "%s: need either lut or (query, codebook)", what);
  if (!lut) {
    TPQ_REQUIRE(ds >= 1 && ds <= 1024, "%s: bad sub-vector length %d", what, ds);
    TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "%s: metric=%d", what, metric);
  }
  const int R = list_regs(k);
  const size_t lds = list_scan_lds_bytes(list_region0<size_t>((size_t)m * 1024, R), max_nprobe,
                                         kPendingBytes + (lut ? 0 : (size_t)m * ds * 4));
  if (int rc = check_lds(what, lds)) return rc;
  ScanArgs a = scan_args(codes, nullptr, lut, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         address2id, out_ids, n_slots, nq, max_nprobe, m, k, n_split);
  if (!lut) {
    a.query = query;
    a.codebook = codebook;
    a.ds = ds;
    a.euclid = metric == TPQ_METRIC_NEG_SQ_L2 ? 1 : 0;
  }
  if (int rc = take_list_ws(a, R, workspace, workspace_bytes, what)) return rc;
  const filtered::FilterArgs f{filter_bits, filter_of_query, filter_stride, n_filters};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    return launch_list_scan(filtered::scan_filtered_kernel<RC>, scan_merge_kernel<RC>, "scan_filtered_kernel", a, lds,
                            st, f);
  });
}

extern "C" int tpq_ivfpq_scan_filtered_residual_topk(
    const uint8_t* codes, const float* part1, const float* query, const float* codebook, int ds, const float* part2,
    const float* full_lut, const int64_t* cells, const float* base_sims, const uint8_t* is_empty,
    const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list, const uint32_t* filter_bits,
    const int32_t* filter_of_query, int n_filters, int64_t filter_stride, float* out_vals, int64_t* out_addr,
    const int64_t* address2id, int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe, int m, int k,
    tpq_stream_t stream) {
  const char* what = "ivfpq_scan_filtered_residual";
  int done;
  if (int rc = filtered::check_common(what, codes && cell_start && cell_size && n_probe_list && out_vals && out_addr,
                                      filter_bits, n_filters, filter_stride, address2id, out_ids, n_slots, nq,
                                      max_nprobe, m, k, 1, &done))
    return rc;
  if (done) return TPQ_OK;
  TPQ_REQUIRE(base_sims != nullptr, "%s: base_sims is required", what);
  TPQ_REQUIRE(full_lut || (part2 && cells && (part1 || (query && codebook))),
              "%s: need either full_lut or (part1 or (query, codebook), part2, cells)", what);
  const bool build_part1 = !full_lut && !part1;
  if (build_part1) TPQ_REQUIRE(ds >= 1 && ds <= 1024, "%s: bad sub-vector length %d", what, ds);
  const int R = list_regs(k);
  const size_t lds = list_scan_lds_bytes(list_region0<size_t>((size_t)m * 1024, R), max_nprobe,
                                         kPendingBytes + (build_part1 ? (size_t)m * ds * 4 : 0));
  if (int rc = check_lds(what, lds)) return rc;
  ScanArgs a = scan_args(codes, nullptr, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         address2id, out_ids, n_slots, nq, max_nprobe, m, k, 1);
  if (build_part1) {
    a.query = query;
    a.codebook = codebook;
    a.ds = ds;
    a.euclid = 2;  // part1 = 2 q_j . r_jc (fused_lut4)
  }
  const ResidualArgs ra{full_lut ? nullptr : part1, part2, full_lut, cells, base_sims, nullptr, nullptr};
  const filtered::FilterArgs f{filter_bits, filter_of_query, filter_stride, n_filters};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    return launch_list_scan(filtered::scan_filtered_residual_kernel<RC>, scan_merge_kernel<RC>,
                            "scan_filtered_residual_kernel", a, lds, st, ra, f);
  });
}

extern "C" int tpq_slot_filter_build(const int64_t* address, int64_t n, uint32_t* bits, int64_t n_slots,
                                     tpq_stream_t stream) {
  TPQ_REQUIRE(n >= 0, "slot_filter_build: n=%lld", (long long)n);
  if (int rc = check_n_slots("slot_filter_build", n_slots)) return rc;
  if (n == 0 || n_slots == 0) return TPQ_OK;
  TPQ_REQUIRE(address && bits, "slot_filter_build: null pointer argument");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(filtered::slot_filter_build_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), address, n, bits, n_slots);
  TPQ_LAUNCH_CHECK("slot_filter_build_kernel");
  return TPQ_OK;
}
