// List scan of IVFPQ4Index (tpq_ivfpq4_scan_topk): product-quantized lists with 16 centroids per sub-quantizer.
//
// A code is m / 2 bytes, two sub-quantizers per byte, low nibble first; the container stores it with contiguous_size
// = 4, so the storage read as 32-bit words is [m / 8][n_slots]: word w of slot s holds sub-quantizers 8 w ... 8 w + 7,
// lowest nibble first (include/torchpq_amd.h).  One workgroup per (query, part), eight waves, on the frame of the list
// kernels (scan_list.h): the workgroup first builds its query's table lut[m][16] in LDS from the query and the codebook
// (16 d multiply-adds, the codebook is 64 d bytes and stays in L2) -- the table never exists in HBM --, then a wave
// takes the 64-slot tiles of the probed cells round-robin, a lane owns one slot of the tile, loads its m / 8 words
// (a wave reads 256 contiguous bytes per word row, kPq4Unroll rows in flight) and adds the m table entries in ascending
// j, one fp32 add each.  The value goes through the per-wave selector and the workgroup-shared threshold of the other
// scans.  A query's tiles are cut into n_split parts when the batch is small; scan_merge_kernel merges the parts' lists.
//
// LDS banks: a 16-entry fp32 row is 64 bytes, 16 consecutive banks; ds_read_b32 conflicts only between DIFFERENT
// addresses on one bank within a group of 32 lanes, and all lanes of a wave read the same row at the same time, so the
// look-ups are conflict-free whatever the codes are -- with the container's own layout, no scan-layout copy.
//
// Residual codes (tpq_ivfpq4_scan_residual_topk, IVFPQ4Index(pq_use_residual=True)): scan_pq4_residual_kernel below, on
// the same frame and the same word loop, rebuilds the table for every probe.
#include "scan_pq4.h"

namespace tpq {
namespace pq4 {

// LDS: [table m x 16 floats | the finisher's merge lists, which start once the scan is over][queues][probe table]
//      [threshold][query d floats]

template <int R, int METRIC>
__global__ __launch_bounds__(kScanThreads) void scan_pq4_kernel(ScanArgs a, size_t region0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lut = reinterpret_cast<float*>(smem);
  const ListLds lds(smem, region0, a.max_nprobe);
  float* xq = reinterpret_cast<float*>(lds.tail);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int ds = a.ds;
  const int n_probe = clamped_n_probe(a, q);

  lds.init(a, q, n_probe, wave, lane);
  for (int i = threadIdx.x; i < a.m * ds; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  __syncthreads();
  // the table: thread t takes entries t, t + 512, ... -- sixteen consecutive threads write one row, and read sixteen
  // consecutive floats of the codebook per dimension
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

  const TileRange t = part_tiles(lds.tab.tile_begin[n_probe], part, a.n_split);
  const int64_t stride = a.n_slots;
  const int W = a.m >> 3;
  const uint32_t* __restrict__ codes32 = reinterpret_cast<const uint32_t*>(a.codes);

  int p = 0;
  for (int T = t.begin + wave; T < t.end; T += kScanWaves) {
    p = probe_of(lds.tab, p, T);
    const Tile tile = tile_at(lds.tab, p, T, lane);
    const int s = tile.slot();
    const bool valid = tile.in_cell() && s >= 0 && (int64_t)s < a.n_slots;  // (a cell that leaves the storage is cut)
    float v = 0.f;
    bool live = valid;
    if (valid) {
      if (a.is_empty) live = (a.is_empty[s] == 0);
      const uint32_t* __restrict__ col = codes32 + s;
      const float* row = lut;
      int w = 0;
      for (; w + kPq4Unroll <= W; w += kPq4Unroll) {
        v = add_words<kPq4Unroll>(v, col, stride, row);
        col += (int64_t)kPq4Unroll * stride;
        row += kPq4Unroll * 128;
      }
      // the last W mod 8 words, still in ascending order: four, two, one
      if (W & 4) {
        v = add_words<4>(v, col, stride, row);
        col += 4 * stride;
        row += 4 * 128;
      }
      if (W & 2) {
        v = add_words<2>(v, col, stride, row);
        col += 2 * stride;
        row += 2 * 128;
      }
      if (W & 1) v = add_words<1>(v, col, stride, row);
    }
    admit(sel, lds.tau_key, live, v, s);
  }
  sel.flush();
  // (the finisher starts with a barrier: no wave overwrites the table with its list before the last tile is done)
  finish_list_scan<R>(a, q, part, sel.top, smem);
}

// ---- residual codes (tpq_ivfpq4_scan_residual_topk): the table changes with the probe --------------------------------
// A code quantizes x - centroid(cell(x)), so the table of probe p is built from the query, the codebook AND the probed
// cell's centroid: entry (j, c) is the metric between q_j and centroids[cell_p][j] + codebook[j][.][c].  At 16 entries a
// row that is m x 16 floats per probe -- 16 d adds and 16 d metric steps, next to 64-slot tiles of m look-ups each -- so
// the workgroup rebuilds it for every probe and no table exists in HBM here either.
//
// The part's probes are walked in GROUPS of up to G consecutive probes (G = residual_group(m, max_nprobe): as many
// tables as fit 32 KiB, eight at most).  region0 holds two buffers of G tables: while the waves scan the tiles of one
// group -- round-robin over the whole group, each tile in the table of its own probe --, every thread has already
// written its share of the next group's tables into the other buffer; ONE barrier per group then both publishes those
// tables and retires the reads of the old ones.  A thread builds the same entry (j, c) of all the group's tables at
// once: the codebook entry is loaded once and the G centroid components together, so a group costs one memory latency
// per (entry, dimension) rather than one per probe, and at most ceil(n_probe / G) + 1 barriers per workgroup replace
// one per probe (with one table per barrier the latency of the build stood between any two probes: 1.37 x the plain
// kernel at 977-slot cells, 3.2 x at cells of one or two tiles).  Which probes form a group is decided
// from the LDS probe table and the part's bounds alone, by every thread alike: the groups start at the first probe
// with a tile in [t.begin, t.end) -- a part that begins inside a probe starts with that probe's table -- and end at
// the last; a wave with no tile in a group still takes the group's barrier.
// LDS: [buffer A: G tables of m x 16 floats][buffer B] | the finisher's merge lists ... [queues][probe table]
//      [threshold][query d floats][the probes' cell indices max_nprobe ints]
template <int R, int METRIC>
__global__ __launch_bounds__(kScanThreads) void scan_pq4_residual_kernel(ScanArgs a, size_t region0,
                                                                         ResidualProbes rp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lut = reinterpret_cast<float*>(smem);
  const int lut_floats = a.m * 16;
  const int G = residual_group(a.m, a.max_nprobe);
  const ListLds lds(smem, region0, a.max_nprobe);
  float* xq = reinterpret_cast<float*>(lds.tail);
  int* cell = reinterpret_cast<int*>(xq + a.m * a.ds);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int n_probe = clamped_n_probe(a, q);

  lds.init(a, q, n_probe, wave, lane);
  for (int i = threadIdx.x; i < a.m * a.ds; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  // (a cell index outside [0, n_cells) is the caller's error: clamped, so that nothing outside `centroids` is read)
  for (int p = threadIdx.x; p < n_probe; p += kScanThreads) {
    const int64_t c = rp.cells[(int64_t)q * a.max_nprobe + p];
    cell[p] = c < 0 ? 0 : (c >= rp.n_cells ? rp.n_cells - 1 : (int)c);
  }
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(lds.qv + wave * 64, lds.qi + wave * 64, a.k);

  const TileRange t = part_tiles(lds.tab.tile_begin[n_probe], part, a.n_split);
  const int64_t stride = a.n_slots;
  const int W = a.m >> 3;
  const uint32_t* __restrict__ codes32 = reinterpret_cast<const uint32_t*>(a.codes);

  // the part's probes: from the first with a tile of the part to the last (the same two numbers in every thread)
  int g0 = next_scanned_probe(lds.tab, 0, n_probe, t);
  int p_end = g0;
  while (p_end < n_probe && lds.tab.tile_begin[p_end] < t.end) ++p_end;
  if (g0 < p_end) build_group_luts<METRIC>(a, rp.centroids, cell, g0, min(G, p_end - g0), xq, lut);
  __syncthreads();
  int cur = 0;
  while (g0 < p_end) {
    const int g1 = min(g0 + G, p_end);  // this group: probes [g0, g1)
    const int g_next = next_scanned_probe(lds.tab, g1, p_end, t);
    // (the other buffer was last read before the barrier that ended the previous group)
    if (g_next < p_end)
      build_group_luts<METRIC>(a, rp.centroids, cell, g_next, min(G, p_end - g_next), xq,
                               lut + (cur ^ 1) * G * lut_floats);
    const float* tables = lut + cur * G * lut_floats;
    const int lo = max(lds.tab.tile_begin[g0], t.begin), hi = min(lds.tab.tile_begin[g1], t.end);
    int p = g0;
    // (tile T belongs to wave (T - t.begin) mod 8, as in scan_pq4_kernel: groups of few tiles still spread over the waves)
    for (int T = lo + ((wave - (lo - t.begin)) & (kScanWaves - 1)); T < hi; T += kScanWaves) {
      p = probe_of(lds.tab, p, T);
      const Tile tile = tile_at(lds.tab, p, T, lane);
      const int s = tile.slot();
      const bool valid = tile.in_cell() && s >= 0 && (int64_t)s < a.n_slots;  // (a cell that leaves the storage is cut)
      float v = 0.f;
      bool live = valid;
      if (valid) {
        if (a.is_empty) live = (a.is_empty[s] == 0);
        v = code_value(codes32 + s, stride, tables + (p - g0) * lut_floats, W);
      }
      admit(sel, lds.tau_key, live, v, s);
    }
    if (g_next >= p_end) break;  // (the finisher's opening barrier ends the last group)
    __syncthreads();
    g0 = g_next;
    cur ^= 1;
  }
  sel.flush();
  // (the finisher starts with a barrier: no wave overwrites a table with its list before the last tile is done)
  finish_list_scan<R>(a, q, part, sel.top, smem);
}

template <int METRIC>
static int dispatch(const ScanArgs& a, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    const size_t region0 = list_region0((size_t)a.m * 64, RC);
    return launch_list_scan(scan_pq4_kernel<RC, METRIC>, scan_merge_kernel<RC>, "scan_pq4_kernel", a,
                            list_scan_lds_bytes(region0, a.max_nprobe, (size_t)a.m * a.ds * 4), st, region0);
  });
}

template <int METRIC>
static int dispatch_residual(const ScanArgs& a, const ResidualProbes& rp, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    const size_t region0 = list_region0((size_t)2 * residual_group(a.m, a.max_nprobe) * a.m * 64, RC);  // two buffers
    return launch_list_scan(scan_pq4_residual_kernel<RC, METRIC>, scan_merge_kernel<RC>, "scan_pq4_residual_kernel", a,
                            list_scan_lds_bytes(region0, a.max_nprobe, ((size_t)a.m * a.ds + a.max_nprobe) * 4), st,
                            region0, rp);
  });
}

}  // namespace pq4
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq4_scan_workspace_bytes(int nq, int k, int n_split) {
  if (nq <= 0 || k <= 0 || k > 1024) return 0;
  return list_ws_bytes(nq, list_regs(k), n_split);
}

// both entry points: `rp` is null for plain codes
static int pq4_scan_topk(const char* what, const pq4::ResidualProbes* rp, const uint8_t* codes, const float* query,
                         const float* codebook, const uint8_t* is_empty, const int64_t* cell_start,
                         const int64_t* cell_size, const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                         int64_t n_slots, int m, int ds, int nq, int max_nprobe, int k, int metric, int n_split,
                         void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
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
  if (nq == 0) return TPQ_OK;
  if (int rc = check_grid(what,
                          codes && query && codebook && cell_start && cell_size && n_probe_list && out_vals &&
                              out_addr && (!rp || (rp->centroids && rp->cells)),
                          nq, n_split))
    return rc;
  const int R = list_regs(k);
  ScanArgs a = scan_args(codes, nullptr, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         nullptr, nullptr, n_slots, nq, max_nprobe, m, k, n_split);
  a.query = query;
  a.codebook = codebook;
  a.ds = ds;
  if (int rc = take_list_ws(a, R, workspace, workspace_bytes, what)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (rp)
    return metric == TPQ_METRIC_NEG_SQ_L2 ? pq4::dispatch_residual<TPQ_METRIC_NEG_SQ_L2>(a, *rp, R, st)
                                          : pq4::dispatch_residual<TPQ_METRIC_INNER>(a, *rp, R, st);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? pq4::dispatch<TPQ_METRIC_NEG_SQ_L2>(a, R, st)
                                        : pq4::dispatch<TPQ_METRIC_INNER>(a, R, st);
}

extern "C" int tpq_ivfpq4_scan_topk(const uint8_t* codes, const float* query, const float* codebook,
                                    const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                                    const int64_t* n_probe_list, float* out_vals, int64_t* out_addr, int64_t n_slots,
                                    int m, int ds, int nq, int max_nprobe, int k, int metric, int n_split,
                                    void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  return pq4_scan_topk("ivfpq4_scan", nullptr, codes, query, codebook, is_empty, cell_start, cell_size, n_probe_list,
                       out_vals, out_addr, n_slots, m, ds, nq, max_nprobe, k, metric, n_split, workspace,
                       workspace_bytes, stream);
}

extern "C" int tpq_ivfpq4_scan_residual_topk(const uint8_t* codes, const float* query, const float* codebook,
                                             const float* centroids, const int64_t* cells, int n_cells,
                                             const uint8_t* is_empty, const int64_t* cell_start,
                                             const int64_t* cell_size, const int64_t* n_probe_list, float* out_vals,
                                             int64_t* out_addr, int64_t n_slots, int m, int ds, int nq, int max_nprobe,
                                             int k, int metric, int n_split, void* workspace, size_t workspace_bytes,
                                             tpq_stream_t stream) {
  const pq4::ResidualProbes rp{centroids, cells, n_cells};
  return pq4_scan_topk("ivfpq4_scan_residual", &rp, codes, query, codebook, is_empty, cell_start, cell_size,
                       n_probe_list, out_vals, out_addr, n_slots, m, ds, nq, max_nprobe, k, metric, n_split, workspace,
                       workspace_bytes, stream);
}
