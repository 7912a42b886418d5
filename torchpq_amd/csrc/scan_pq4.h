// The device code the 4-bit list scans share (scan_pq4.hip, scan_pq4_filtered.hip): the word loop over a 16-entry table
// row per sub-quantizer, the grouped per-probe tables of residual codes, and the constants.  Codes, table entry and value
// are defined in include/torchpq_amd.h; the schedule of the word loop and the group walk in DESIGN 3.13 / 3.13b.
#pragma once
#include "scan_device.h"
#include "scan_ref.h"

namespace tpq {
namespace pq4 {

constexpr int kPq4Unroll = 8;  // word loads in flight per lane: 8 x 256 B per wave (m = 64: the whole code)
constexpr int kMinM = 8, kMaxM = 256;

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

// ---- residual codes: the table changes with the probe -------------------------------------------------------------
struct ResidualProbes {
  const float* centroids;  // [n_cells][d]
  const int64_t* cells;    // [nq][max_nprobe]
  int n_cells;
};

constexpr int kMaxGroup = 8;
// tables per buffer (host and device agree: the host sizes region0 with it)
__host__ __device__ constexpr int residual_group(int m, int max_nprobe) {
  const int fit = (32 * 1024) / (m * 64);
  const int g = fit < 1 ? 1 : (fit > kMaxGroup ? kMaxGroup : fit);
  return g < max_nprobe ? g : max_nprobe;
}

// the first probe at or after `p` with a tile in [t.begin, t.end), or n_probe (the same answer in every thread)
__device__ __forceinline__ int next_scanned_probe(const ProbeTable& tab, int p, int n_probe, const TileRange& t) {
  for (; p < n_probe; ++p) {
    const int lo = tab.tile_begin[p], hi = tab.tile_begin[p + 1];
    if (lo >= t.end) break;  // (the prefix ascends: nor has any later probe)
    if (max(lo, t.begin) < min(hi, t.end)) return p;
  }
  return n_probe;
}

// The tables of probes g0 ... g0 + cnt - 1 (cnt <= kMaxGroup), table g at lut + g * m * 16: thread t takes entries t,
// t + 512, ... of every table, as in scan_pq4_kernel; the sixteen threads of a row read the same centroid components
// (one address per probe) and sixteen consecutive floats of the codebook per dimension.  `cell` holds the probes'
// cell indices, clamped to [0, n_cells) when they were staged.
template <int METRIC>
__device__ __forceinline__ void build_group_luts(const ScanArgs& a, const float* __restrict__ centroids, const int* cell,
                                                 int g0, int cnt, const float* xq, float* lut) {
  const int ds = a.ds;
  const int64_t d = (int64_t)a.m * ds;
  const float* __restrict__ cen[kMaxGroup];
#pragma unroll
  for (int g = 0; g < kMaxGroup; ++g)  // (uniform: kept in scalar registers; beyond cnt the last probe's, never read)
    cen[g] = centroids + (int64_t)__builtin_amdgcn_readfirstlane(cell[g0 + (g < cnt ? g : cnt - 1)]) * d;
  for (int e = threadIdx.x; e < a.m * 16; e += kScanThreads) {
    const int j = e >> 4;
    const float* __restrict__ cb = a.codebook + (int64_t)j * ds * 16 + (e & 15);
    const float* xj = xq + j * ds;
    float acc[kMaxGroup];
#pragma unroll
    for (int g = 0; g < kMaxGroup; ++g) acc[g] = 0.f;
    for (int i = 0; i < ds; ++i) {
      const float w = cb[i * 16], x = xj[i];
      float c[kMaxGroup];
#pragma unroll
      for (int g = 0; g < kMaxGroup; ++g)
        if (g < cnt) c[g] = cen[g][j * ds + i];
#pragma unroll
      for (int g = 0; g < kMaxGroup; ++g)
        if (g < cnt) acc[g] = metric_step<METRIC>(acc[g], x, __fadd_rn(c[g], w));
    }
#pragma unroll
    for (int g = 0; g < kMaxGroup; ++g)
      if (g < cnt) lut[g * a.m * 16 + e] = acc[g];
  }
}

// the value of the slot whose words start at `col`: scan_pq4_kernel's word loop (kept apart from it: that kernel's code
// is not touched by this one)
__device__ __forceinline__ float code_value(const uint32_t* __restrict__ col, int64_t stride, const float* row, int W) {
  float v = 0.f;
  int w = 0;
  for (; w + kPq4Unroll <= W; w += kPq4Unroll) {
    v = add_words<kPq4Unroll>(v, col, stride, row);
    col += (int64_t)kPq4Unroll * stride;
    row += kPq4Unroll * 128;
  }
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
  return v;
}

}  // namespace pq4
}  // namespace tpq
