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
#include "scan_device.h"
#include "scan_ref.h"

namespace tpq {
namespace pq4 {

constexpr int kPq4Unroll = 8;  // word loads in flight per lane: 8 x 256 B per wave (m = 64: the whole code)
constexpr int kMinM = 8, kMaxM = 256;

// LDS: [table m x 16 floats | the finisher's merge lists, which start once the scan is over][queues][probe table]
//      [threshold][query d floats]

template <int POS>
__device__ __forceinline__ unsigned nibble(uint32_t w) {
  return (w >> POS) & 15u;
}

// the eight table entries of one word: rows 8 w ... 8 w + 7 start at `r`, sixteen entries each
__device__ __forceinline__ void read_word(float (&e)[8], const float* r, uint32_t w) {
  e[0] = r[0 * 16 + nibble<0>(w)];
  e[1] = r[1 * 16 + nibble<4>(w)];
  e[2] = r[2 * 16 + nibble<8>(w)];
  e[3] = r[3 * 16 + nibble<12>(w)];
  e[4] = r[4 * 16 + nibble<16>(w)];
  e[5] = r[5 * 16 + nibble<20>(w)];
  e[6] = r[6 * 16 + nibble<24>(w)];
  e[7] = r[7 * 16 + nibble<28>(w)];
}

// U words of a slot (rows `stride` words apart, all loads issued first) looked up in the U x 8 table rows at `row` and
// added in ascending order.  A word's look-ups are issued ahead of the previous word's adds and a scheduling barrier
// keeps them there: left to itself the scheduler sank every ds_read_b32 next to its add -- read, wait, add, one LDS
// latency per look-up (read off the ISA).  As built the compiler issues all of a group's reads back to back, then the
// adds (104-111 VGPRs, four waves per SIMD); 7 % faster at the bench shape than the serial schedule.
template <int U>
__device__ __forceinline__ float add_words(float v, const uint32_t* __restrict__ col, int64_t stride,
                                           const float* row) {
  uint32_t w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) w[u] = col[(int64_t)u * stride];
  float e[2][8];
  read_word(e[0], row, w[0]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (u + 1 < U) read_word(e[(u + 1) & 1], row + (u + 1) * 128, w[u + 1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < 8; ++n) v = __fadd_rn(v, e[u & 1][n]);
  }
  return v;
}

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

template <int METRIC>
static int dispatch(const ScanArgs& a, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    const size_t region0 = list_region0((size_t)a.m * 64, RC);
    return launch_list_scan(scan_pq4_kernel<RC, METRIC>, scan_merge_kernel<RC>, "scan_pq4_kernel", a,
                            list_scan_lds_bytes(region0, a.max_nprobe, (size_t)a.m * a.ds * 4), st, region0);
  });
}

}  // namespace pq4
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq4_scan_workspace_bytes(int nq, int k, int n_split) {
  if (nq <= 0 || k <= 0 || k > 1024) return 0;
  return list_ws_bytes(nq, list_regs(k), n_split);
}

extern "C" int tpq_ivfpq4_scan_topk(const uint8_t* codes, const float* query, const float* codebook,
                                    const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                                    const int64_t* n_probe_list, float* out_vals, int64_t* out_addr, int64_t n_slots,
                                    int m, int ds, int nq, int max_nprobe, int k, int metric, int n_split,
                                    void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  const char* what = "ivfpq4_scan";
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  if (m < pq4::kMinM || m > pq4::kMaxM || m % 8 != 0 || ds < 1) {
    set_error("ivfpq4_scan: m=%d, ds=%d: m must be a multiple of 8 in [8, 256], ds >= 1", m, ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (k < 1 || k > 1024) {
    set_error("ivfpq4_scan: k=%d out of range (0, 1024]", k);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (int rc = check_lists(what, metric, n_split, n_slots)) return rc;
  if ((int64_t)m * ds > (1 << 20)) {  // (far beyond the LDS; keeps m * ds * 4 inside an int)
    set_error("ivfpq4_scan: d = m * ds = %lld is not supported", (long long)m * ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (nq == 0) return TPQ_OK;
  if (int rc = check_grid(what,
                          codes && query && codebook && cell_start && cell_size && n_probe_list && out_vals && out_addr,
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
  return metric == TPQ_METRIC_NEG_SQ_L2 ? pq4::dispatch<TPQ_METRIC_NEG_SQ_L2>(a, R, st)
                                        : pq4::dispatch<TPQ_METRIC_INNER>(a, R, st);
}
