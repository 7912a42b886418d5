// Filtered top-k over the lists of IVFPQ4Index (tpq_ivfpq4_scan_filtered_topk / _residual_topk): the k best
// candidates of the 4-bit list scan (scan_pq4.hip) AMONG the slots a filter allows.
//
// A filter is a row of bits over the slot addresses, bit s & 31 of word s >> 5 for slot s; every query names its row
// (scan_list.h: FilterArgs, the format of scan_filtered.hip).  Candidates, values, order and padding are those of
// tpq_ivfpq4_scan_topk / _residual_topk called with is_empty | ~allowed_row(q) as the tombstone mask of query q, bit for
// bit: the frame, the table build, the word loop (scan_pq4.h: code_value) and the finisher are those kernels' own.
//
// What differs is the tile loop, that of scan_filtered.hip, which tests a slot's bit BEFORE it touches the slot's m / 2
// bytes of code:
//   membership  a lane reads the filter word of its slot of the tile, the tombstone byte only where the bit is set;
//               kTilesAhead tiles' words are in flight together.  A tile without an allowed live slot reads no code.
//   compaction  the allowed live slots are appended, by ballot and mbcnt rank, to a list of pending slots the wave owns
//               in LDS (no barrier); whenever 64 or more are pending the wave takes 64 and every lane values one slot.
//               Plain codes drain the rest once, after the wave's last tile.
// Residual codes keep up to eight probes' tables live per barrier (the group walk of scan_pq4_residual_kernel), so 64
// pending slots may belong to different tables: a pending entry carries, next to the slot, the index p - g0 of the table
// of the probe that scans it, and a lane looks its slot up in its own table.  A wave drains its list at the end of
// every group, BEFORE the barrier that lets the other waves overwrite the group's buffer two groups later -- and that
// retires the reads of this one.
// (Measured and not kept, DESIGN 3.16, tools/experiments/pq4_filtered_ab.patch: a membership pass ahead of the walk
// that lets it skip the tables of probes without an allowed live slot, and a drain per probe instead of per group.)
// Keys are (value, address): the order in which slots reach the selector does not change the result.
//
// LDS: the frame of a list kernel (scan_list.h) with, behind it, the pending lists (plain: 8 waves x 128 slots = 4 KiB;
// residual: slot and table index, 8 KiB), then the staged query (and, residual, the probes' cell indices).
#include "scan_pq4.h"

namespace tpq {
namespace pq4 {

using filtered::FilterArgs;
using filtered::filter_row;
using filtered::Member;
using filtered::member;

constexpr int kTilesAhead = 4;  // tiles whose filter words (then tombstone bytes) are loaded together

// the pending slots of residual codes: two words per entry, the slot and the table it is looked up in
constexpr size_t kTablePendingBytes = 2 * kPendingBytes;
struct TablePending {
  int* at;  // the wave's [2][kPendingPerWave] words: the slots, then the table index of each
  int n;    // wave-uniform, < 64 between tiles
  __device__ __forceinline__ void append(bool ok, int s, int g) {
    const unsigned long long mask = __ballot(ok);
    if (mask == 0ull) return;
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
    if (ok) {
      at[n + rank] = s;
      at[kPendingPerWave + n + rank] = g;
    }
    n += __popcll(mask);
  }
  // the last `count` (<= 64) pending entries, one per lane below `count`
  __device__ __forceinline__ int take(int count, int& g) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    n -= count;
    const int lane = lane_id();
    const int s = lane < count ? at[n + lane] : 0;
    g = lane < count ? at[kPendingPerWave + n + lane] : 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    return s;
  }
};

// the payload sizes, one expression for host and device
__host__ __device__ constexpr size_t plain_tail_bytes(int m, int ds) { return kPendingBytes + (size_t)m * ds * 4; }
__host__ __device__ constexpr size_t residual_tail_bytes(int m, int ds, int max_nprobe) {
  return kTablePendingBytes + ((size_t)m * ds + max_nprobe) * 4;
}

// the tombstones of the members: read only where the bit is set
__device__ __forceinline__ void drop_tombstones(const ScanArgs& a, Member (&mb)[kTilesAhead]) {
  if (a.is_empty) {
#pragma unroll
    for (int u = 0; u < kTilesAhead; ++u)
      if (mb[u].ok) mb[u].ok = a.is_empty[mb[u].s] == 0;
  }
}

// ---- plain codes ---------------------------------------------------------------------------------------------------
// `count` pending slots are valued, one per lane, and go through the admission step
template <int R>
__device__ __forceinline__ void value_pending(const ScanArgs& a, const float* lut, Pending& pend, int count,
                                              WaveSelector<R>& sel, unsigned* tau_key) {
  const int s = pend.take(count);
  const bool live = lane_id() < count;
  float v = 0.f;
  if (live) v = code_value(reinterpret_cast<const uint32_t*>(a.codes) + s, a.n_slots, lut, a.m >> 3);
  admit(sel, tau_key, live, v, s);
}

// LDS: [table m x 16 floats | the finisher's merge lists][queues][probe table][threshold][pending 8 x 128]
//      [query d floats]
template <int R, int METRIC>
__global__ __launch_bounds__(kScanThreads) void scan_pq4_filtered_kernel(ScanArgs a, size_t region0, FilterArgs f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lut = reinterpret_cast<float*>(smem);
  const ListLds lds(smem, region0, a.max_nprobe);
  float* xq = reinterpret_cast<float*>(lds.tail + kPendingBytes);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int ds = a.ds;
  const uint32_t* __restrict__ row = filter_row(f, q);  // (uniform)
  const int n_probe = row ? clamped_n_probe(a, q) : 0;   // no row: no tile, no table, k pads

  lds.init(a, q, n_probe, wave, lane);
  if (row)
    for (int i = threadIdx.x; i < a.m * ds; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  __syncthreads();
  // the table, as scan_pq4_kernel builds it
  if (row)
    for (int e = threadIdx.x; e < a.m * 16; e += kScanThreads) {
      const int j = e >> 4;
      const float* __restrict__ cb = a.codebook + (int64_t)j * ds * 16 + (e & 15);
      const float* xj = xq + j * ds;
      float acc = 0.f;
      for (int i = 0; i < ds; ++i) acc = metric_step<METRIC>(acc, xj[i], cb[i * 16]);
      lut[e] = acc;
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
    drop_tombstones(a, mb);
#pragma unroll
    for (int u = 0; u < kTilesAhead; ++u) {
      pend.append(mb[u].ok, mb[u].s);
      if (pend.n >= 64) value_pending<R>(a, lut, pend, 64, sel, lds.tau_key);
    }
  }
  if (pend.n > 0) value_pending<R>(a, lut, pend, pend.n, sel, lds.tau_key);
  sel.flush();
  // (the finisher starts with a barrier: no wave overwrites the table with its list before the last slot is valued)
  finish_list_scan<R>(a, q, part, sel.top, smem);
}

// ---- residual codes ------------------------------------------------------------------------------------------------
// `count` pending entries are valued, one per lane, each in the table of the probe that scans its slot
template <int R>
__device__ __forceinline__ void value_pending(const ScanArgs& a, const float* tables, int lut_floats, TablePending& pend,
                                              int count, WaveSelector<R>& sel, unsigned* tau_key) {
  int g;
  const int s = pend.take(count, g);
  const bool live = lane_id() < count;
  float v = 0.f;
  if (live)
    v = code_value(reinterpret_cast<const uint32_t*>(a.codes) + s, a.n_slots, tables + g * lut_floats, a.m >> 3);
  admit(sel, tau_key, live, v, s);
}

// LDS: [buffer A: G tables of m x 16 floats][buffer B] | the finisher's merge lists ... [queues][probe table]
//      [threshold][pending 8 x 2 x 128][query d floats][the probes' cell indices max_nprobe ints]
template <int R, int METRIC>
__global__ __launch_bounds__(kScanThreads) void scan_pq4_filtered_residual_kernel(ScanArgs a, size_t region0,
                                                                                  ResidualProbes rp, FilterArgs f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lut = reinterpret_cast<float*>(smem);
  const int lut_floats = a.m * 16;
  const int G = residual_group(a.m, a.max_nprobe);
  const ListLds lds(smem, region0, a.max_nprobe);
  float* xq = reinterpret_cast<float*>(lds.tail + kTablePendingBytes);
  int* cell = reinterpret_cast<int*>(xq + a.m * a.ds);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const uint32_t* __restrict__ row = filter_row(f, q);  // (uniform)
  const int n_probe = row ? clamped_n_probe(a, q) : 0;   // no row: no tile, no table, k pads

  lds.init(a, q, n_probe, wave, lane);
  if (row)
    for (int i = threadIdx.x; i < a.m * a.ds; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  // (a cell index outside [0, n_cells) is the caller's error: clamped, so that nothing outside `centroids` is read)
  for (int p = threadIdx.x; p < n_probe; p += kScanThreads) {
    const int64_t c = rp.cells[(int64_t)q * a.max_nprobe + p];
    cell[p] = c < 0 ? 0 : (c >= rp.n_cells ? rp.n_cells - 1 : (int)c);
  }
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);
  TablePending pend{reinterpret_cast<int*>(lds.tail) + wave * 2 * kPendingPerWave, 0};

  const TileRange t = part_tiles(lds.tab.tile_begin[n_probe], part, a.n_split);

  // the part's probes and their groups: scan_pq4_residual_kernel's walk (the same numbers in every thread)
  int g0 = next_scanned_probe(lds.tab, 0, n_probe, t);
  int p_end = g0;
  while (p_end < n_probe && lds.tab.tile_begin[p_end] < t.end) ++p_end;
  if (g0 < p_end) build_group_luts<METRIC>(a, rp.centroids, cell, g0, min(G, p_end - g0), xq, lut);
  __syncthreads();
  int cur = 0;
  while (g0 < p_end) {
    const int g1 = min(g0 + G, p_end);  // this group: probes [g0, g1)
    const int g_next = next_scanned_probe(lds.tab, g1, p_end, t);
    // (the other buffer was last read before the barrier that ended the previous group: every wave had drained)
    if (g_next < p_end)
      build_group_luts<METRIC>(a, rp.centroids, cell, g_next, min(G, p_end - g_next), xq,
                               lut + (cur ^ 1) * G * lut_floats);
    const float* tables = lut + cur * G * lut_floats;
    const int lo = max(lds.tab.tile_begin[g0], t.begin), hi = min(lds.tab.tile_begin[g1], t.end);
    int p = g0;
    for (int T0 = lo + ((wave - (lo - t.begin)) & (kScanWaves - 1)); T0 < hi; T0 += kScanWaves * kTilesAhead) {
      Member mb[kTilesAhead];
      int tb[kTilesAhead];  // (uniform) the table of the tile's probe
#pragma unroll
      for (int u = 0; u < kTilesAhead; ++u) {
        const int T = T0 + u * kScanWaves;
        mb[u] = Member{0, false};
        tb[u] = 0;
        if (T < hi) {  // (uniform)
          p = probe_of(lds.tab, p, T);
          const Tile tile = tile_at(lds.tab, p, T, lane);
          mb[u] = member(row, tile.start, tile.size, tile.off, a.n_slots);
          tb[u] = p - g0;
        }
      }
      drop_tombstones(a, mb);
#pragma unroll
      for (int u = 0; u < kTilesAhead; ++u) {
        pend.append(mb[u].ok, mb[u].s, tb[u]);
        if (pend.n >= 64) value_pending<R>(a, tables, lut_floats, pend, 64, sel, lds.tau_key);
      }
    }
    // the group's tables are read for the last time here: nothing stays pending across the barrier
    if (pend.n > 0) value_pending<R>(a, tables, lut_floats, pend, pend.n, sel, lds.tau_key);
    if (g_next >= p_end) break;  // (the finisher's opening barrier ends the last group)
    __syncthreads();
    g0 = g_next;
    cur ^= 1;
  }
  sel.flush();
  // (the finisher starts with a barrier: no wave overwrites a table with its list before the last slot is valued)
  finish_list_scan<R>(a, q, part, sel.top, smem);
}

// ---- host ----------------------------------------------------------------------------------------------------------
static size_t plain_region0(int m, int R) { return list_region0((size_t)m * 64, R); }
static size_t residual_region0(int m, int max_nprobe, int R) {
  return list_region0((size_t)2 * residual_group(m, max_nprobe) * m * 64, R);  // two buffers
}
// the LDS of a call, for the check that comes before any HIP call and for the launch
static size_t lds_bytes(bool residual, int m, int ds, int max_nprobe, int R) {
  return residual ? list_scan_lds_bytes(residual_region0(m, max_nprobe, R), max_nprobe,
                                        residual_tail_bytes(m, ds, max_nprobe))
                  : list_scan_lds_bytes(plain_region0(m, R), max_nprobe, plain_tail_bytes(m, ds));
}

template <int METRIC>
static int dispatch(const ScanArgs& a, const FilterArgs& f, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    return launch_list_scan(scan_pq4_filtered_kernel<RC, METRIC>, scan_merge_kernel<RC>, "scan_pq4_filtered_kernel", a,
                            lds_bytes(false, a.m, a.ds, a.max_nprobe, RC), st, plain_region0(a.m, RC), f);
  });
}

template <int METRIC>
static int dispatch_residual(const ScanArgs& a, const ResidualProbes& rp, const FilterArgs& f, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    return launch_list_scan(scan_pq4_filtered_residual_kernel<RC, METRIC>, scan_merge_kernel<RC>,
                            "scan_pq4_filtered_residual_kernel", a, lds_bytes(true, a.m, a.ds, a.max_nprobe, RC), st,
                            residual_region0(a.m, a.max_nprobe, RC), rp, f);
  });
}

}  // namespace pq4
}  // namespace tpq

using namespace tpq;

// both entry points: `rp` is null for plain codes.  The checks of tpq_ivfpq4_scan_topk in its order, the filter's, then
// the LDS; all of them before any HIP call.
static int pq4_scan_filtered_topk(const char* what, const pq4::ResidualProbes* rp, const uint8_t* codes,
                                  const float* query, const float* codebook, const uint8_t* is_empty,
                                  const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                  const uint32_t* filter_bits, const int32_t* filter_of_query, int n_filters,
                                  int64_t filter_stride, float* out_vals, int64_t* out_addr, int64_t n_slots, int m,
                                  int ds, int nq, int max_nprobe, int k, int metric, int n_split, void* workspace,
                                  size_t workspace_bytes, tpq_stream_t stream) {
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  if (m < pq4::kMinM || m > pq4::kMaxM || m % 8 != 0 || ds < 1) {
    set_error("%s: m=%d, ds=%d: m must be a multiple of 8 in [8, 256], ds >= 1", what, m, ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (k < 1 || k > 1024) {
    set_error("%s: k=%d out of range (0, 1024]", what, k);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (int rc = check_lists(what, metric, n_split, n_slots)) return rc;
  if ((int64_t)m * ds > (1 << 20)) {  // (far beyond the LDS; keeps m * ds * 4 inside an int)
    set_error("%s: d = m * ds = %lld is not supported", what, (long long)m * ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (rp) TPQ_REQUIRE(rp->n_cells >= 1, "%s: n_cells=%d", what, rp->n_cells);
  TPQ_REQUIRE(n_filters >= 1, "%s: n_filters=%d", what, n_filters);
  TPQ_REQUIRE(filter_stride >= (n_slots + 31) / 32, "%s: filter_stride=%lld < ceil(n_slots / 32) = %lld", what,
              (long long)filter_stride, (long long)((n_slots + 31) / 32));
  if (nq == 0) return TPQ_OK;
  if (int rc = check_grid(what,
                          codes && query && codebook && cell_start && cell_size && n_probe_list && out_vals &&
                              out_addr && filter_bits && (!rp || (rp->centroids && rp->cells)),
                          nq, n_split))
    return rc;
  const int R = list_regs(k);
  if (int rc = check_lds(what, pq4::lds_bytes(rp != nullptr, m, ds, max_nprobe, R))) return rc;
  ScanArgs a = scan_args(codes, nullptr, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         nullptr, nullptr, n_slots, nq, max_nprobe, m, k, n_split);
  a.query = query;
  a.codebook = codebook;
  a.ds = ds;
  if (int rc = take_list_ws(a, R, workspace, workspace_bytes, what)) return rc;
  const filtered::FilterArgs f{filter_bits, filter_of_query, filter_stride, n_filters};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (rp)
    return metric == TPQ_METRIC_NEG_SQ_L2 ? pq4::dispatch_residual<TPQ_METRIC_NEG_SQ_L2>(a, *rp, f, R, st)
                                          : pq4::dispatch_residual<TPQ_METRIC_INNER>(a, *rp, f, R, st);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? pq4::dispatch<TPQ_METRIC_NEG_SQ_L2>(a, f, R, st)
                                        : pq4::dispatch<TPQ_METRIC_INNER>(a, f, R, st);
}

extern "C" int tpq_ivfpq4_scan_filtered_topk(const uint8_t* codes, const float* query, const float* codebook,
                                             const uint8_t* is_empty, const int64_t* cell_start,
                                             const int64_t* cell_size, const int64_t* n_probe_list,
                                             const uint32_t* filter_bits, const int32_t* filter_of_query,
                                             int n_filters, int64_t filter_stride, float* out_vals, int64_t* out_addr,
                                             int64_t n_slots, int m, int ds, int nq, int max_nprobe, int k, int metric,
                                             int n_split, void* workspace, size_t workspace_bytes,
                                             tpq_stream_t stream) {
  return pq4_scan_filtered_topk("ivfpq4_scan_filtered", nullptr, codes, query, codebook, is_empty, cell_start,
                                cell_size, n_probe_list, filter_bits, filter_of_query, n_filters, filter_stride,
                                out_vals, out_addr, n_slots, m, ds, nq, max_nprobe, k, metric, n_split, workspace,
                                workspace_bytes, stream);
}

extern "C" int tpq_ivfpq4_scan_filtered_residual_topk(
    const uint8_t* codes, const float* query, const float* codebook, const float* centroids, const int64_t* cells,
    int n_cells, const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
    const int64_t* n_probe_list, const uint32_t* filter_bits, const int32_t* filter_of_query, int n_filters,
    int64_t filter_stride, float* out_vals, int64_t* out_addr, int64_t n_slots, int m, int ds, int nq, int max_nprobe,
    int k, int metric, int n_split, void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  const pq4::ResidualProbes rp{centroids, cells, n_cells};
  return pq4_scan_filtered_topk("ivfpq4_scan_filtered_residual", &rp, codes, query, codebook, is_empty, cell_start,
                                cell_size, n_probe_list, filter_bits, filter_of_query, n_filters, filter_stride,
                                out_vals, out_addr, n_slots, m, ds, nq, max_nprobe, k, metric, n_split, workspace,
                                workspace_bytes, stream);
}
