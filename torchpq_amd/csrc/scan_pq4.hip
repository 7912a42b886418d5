// List scan of IVFPQ4Index (tpq_ivfpq4_scan_topk): product-quantized lists with 16 centroids per sub-quantizer.
//
// A code is m / 2 bytes, two sub-quantizers per byte, low nibble first; the container stores it with contiguous_size
// = 4, so the storage read as 32-bit words is [m / 8][n_slots]: word w of slot s holds sub-quantizers 8 w ... 8 w + 7,
// lowest nibble first (include/torchpq_amd.h).  One workgroup per (query, part), eight waves, as scan_flat_kernel
// (scan_flat.hip): the workgroup first builds its query's table lut[m][16] in LDS from the query and the codebook
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
static size_t region0_bytes(int m, int R) {
  const size_t t = (size_t)m * 64, lists = (size_t)kScanWaves * R * 64 * 8;
  return t > lists ? t : lists;
}
static size_t lds_bytes(int m, int ds, int R, int max_nprobe) {
  const size_t b = region0_bytes(m, R) + kScanWaves * 512 + (size_t)(3 * max_nprobe + 1) * 4 + 4 + (size_t)m * ds * 4;
  return (b + 15) & ~(size_t)15;
}
static size_t ws_bytes(int nq, int R, int n_split) {
  return n_split > 1 ? (size_t)nq * n_split * R * 64 * 8 : 0;
}

// one dimension of a table entry: the arithmetic of flat::step (scan_flat.hip)
template <int METRIC>
__device__ __forceinline__ float step(float acc, float q, float x) {
  if constexpr (METRIC == TPQ_METRIC_NEG_SQ_L2) {
    const float t = __fsub_rn(q, x);
    return __fsub_rn(acc, __fmul_rn(t, t));
  } else {
    return __fadd_rn(acc, __fmul_rn(q, x));
  }
}

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
  float* qv_all = reinterpret_cast<float*>(smem + region0);
  int* qi_all = reinterpret_cast<int*>(smem + region0 + kScanWaves * 256);
  int* ptab = reinterpret_cast<int*>(smem + region0 + kScanWaves * 512);
  ProbeTable tab{ptab, ptab + a.max_nprobe, ptab + 2 * a.max_nprobe};
  unsigned* tau_key = reinterpret_cast<unsigned*>(ptab + 3 * a.max_nprobe + 1);
  float* xq = reinterpret_cast<float*>(tau_key + 1);

  const int q = blockIdx.x / a.n_split;
  const int part = blockIdx.x - q * a.n_split;
  const int wave = threadIdx.x >> 6;
  const int lane = lane_id();
  const int ds = a.ds;
  int n_probe = (int)a.n_probe_list[q];
  n_probe = n_probe < 0 ? 0 : (n_probe > a.max_nprobe ? a.max_nprobe : n_probe);

  if (wave == 0) {
    build_probe_table(a, q, n_probe, tab);
    if (lane == 0) *tau_key = f2key(-INFINITY);
  }
  for (int i = threadIdx.x; i < a.m * ds; i += kScanThreads) xq[i] = a.query[(int64_t)i * a.nq + q];
  __syncthreads();
  // the table: thread t takes entries t, t + 512, ... -- sixteen consecutive threads write one row, and read sixteen
  // consecutive floats of the codebook per dimension
  for (int e = threadIdx.x; e < a.m * 16; e += kScanThreads) {
    const int j = e >> 4;
    const float* __restrict__ cb = a.codebook + (int64_t)j * ds * 16 + (e & 15);
    const float* xj = xq + j * ds;
    float acc = 0.f;
    for (int i = 0; i < ds; ++i) acc = step<METRIC>(acc, xj[i], cb[i * 16]);
    lut[e] = acc;
  }
  __syncthreads();

  WaveSelector<R> sel;
  sel.init(qv_all + wave * 64, qi_all + wave * 64, a.k);

  const int total_tiles = tab.tile_begin[n_probe];
  const int t_begin = (int)(((int64_t)total_tiles * part) / a.n_split);
  const int t_end = (int)(((int64_t)total_tiles * (part + 1)) / a.n_split);
  const int64_t stride = a.n_slots;
  const int W = a.m >> 3;
  const uint32_t* __restrict__ codes32 = reinterpret_cast<const uint32_t*>(a.codes);

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
    // workgroup-shared admission threshold, as scan_ref_kernel; a NaN value fails `v >= tau` and never enters
    const float tau_s = key2f(lds_poll_u32(tau_key));
    sel.tau = fmaxf(sel.tau, tau_s);
    const float tau_before = sel.tau;
    sel.push(live && (v >= sel.tau), v, s);
    if (sel.tau > tau_before && lane == 0) atomicMax(tau_key, f2key(sel.tau));
  }
  sel.flush();
  // (finish_query starts with a barrier: no wave overwrites the table with its list before the last tile is done)
  finish_query<R>(a, q, part, sel.top, reinterpret_cast<float*>(smem),
                  reinterpret_cast<int*>(smem + kScanWaves * R * 64 * 4));
}

template <int R, int METRIC>
static int launch(const ScanArgs& a, hipStream_t st) {
  const size_t lds = lds_bytes(a.m, a.ds, R, a.max_nprobe);
  int rc = set_lds(scan_pq4_kernel<R, METRIC>, lds, "scan_pq4_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((scan_pq4_kernel<R, METRIC>), dim3((unsigned)a.nq * a.n_split), dim3(kScanThreads), lds, st, a,
                     region0_bytes(a.m, R));
  TPQ_LAUNCH_CHECK("scan_pq4_kernel");
  if (a.n_split > 1) {
    hipLaunchKernelGGL(scan_merge_kernel<R>, dim3(a.nq), dim3(64), 0, st, a);
    TPQ_LAUNCH_CHECK("scan_merge_kernel");
  }
  return TPQ_OK;
}

template <int METRIC>
static int dispatch(const ScanArgs& a, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) { return launch<decltype(r_c)::value, METRIC>(a, st); });
}

}  // namespace pq4
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq4_scan_workspace_bytes(int nq, int k, int n_split) {
  if (nq <= 0 || k <= 0 || k > 1024) return 0;
  return pq4::ws_bytes(nq, list_regs(k), n_split);
}

extern "C" int tpq_ivfpq4_scan_topk(const uint8_t* codes, const float* query, const float* codebook,
                                    const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                                    const int64_t* n_probe_list, float* out_vals, int64_t* out_addr, int64_t n_slots,
                                    int m, int ds, int nq, int max_nprobe, int k, int metric, int n_split,
                                    void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(nq >= 0 && max_nprobe >= 1, "ivfpq4_scan: bad nq/max_nprobe (%d, %d)", nq, max_nprobe);
  if (m < pq4::kMinM || m > pq4::kMaxM || m % 8 != 0 || ds < 1) {
    set_error("ivfpq4_scan: m=%d, ds=%d: m must be a multiple of 8 in [8, 256], ds >= 1", m, ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (k < 1 || k > 1024) {
    set_error("ivfpq4_scan: k=%d out of range (0, 1024]", k);
    return TPQ_ERR_UNSUPPORTED;
  }
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "ivfpq4_scan: metric=%d", metric);
  TPQ_REQUIRE(n_split >= 1 && n_split <= 1024, "ivfpq4_scan: n_split=%d out of range", n_split);
  TPQ_REQUIRE(n_slots >= 0, "ivfpq4_scan: n_slots=%lld", (long long)n_slots);
  if (n_slots >= (int64_t)kPadIdx) {
    set_error("ivfpq4_scan: n_slots=%lld >= 2^31-1 is not supported", (long long)n_slots);
    return TPQ_ERR_UNSUPPORTED;
  }
  if ((int64_t)m * ds > (1 << 20)) {  // (far beyond the LDS; keeps m * ds * 4 inside an int)
    set_error("ivfpq4_scan: d = m * ds = %lld is not supported", (long long)m * ds);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (nq == 0) return TPQ_OK;
  TPQ_REQUIRE(codes && query && codebook && cell_start && cell_size && n_probe_list && out_vals && out_addr,
              "ivfpq4_scan: null pointer argument");
  TPQ_REQUIRE((int64_t)nq * n_split < 0x7fffffffLL, "ivfpq4_scan: nq * n_split = %lld workgroups",
              (long long)nq * n_split);
  const int R = list_regs(k);
  const size_t need = pq4::ws_bytes(nq, R, n_split);
  if (int rc = need_ws(workspace, workspace_bytes, need, "ivfpq4_scan")) return rc;
  ScanArgs a{};
  a.codes = codes;
  a.query = query;
  a.codebook = codebook;
  a.ds = ds;
  a.is_empty = is_empty;
  a.cell_start = cell_start;
  a.cell_size = cell_size;
  a.n_probe_list = n_probe_list;
  a.out_vals = out_vals;
  a.out_addr = out_addr;
  a.n_slots = n_slots;
  a.nq = nq;
  a.max_nprobe = max_nprobe;
  a.m = m;
  a.k = k;
  a.n_split = n_split;
  if (need) {
    a.ws_vals = reinterpret_cast<float*>(workspace);
    a.ws_idx = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + need / 2);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? pq4::dispatch<TPQ_METRIC_NEG_SQ_L2>(a, R, st)
                                        : pq4::dispatch<TPQ_METRIC_INNER>(a, R, st);
}
