// IVF list scan: device pieces shared by the reference-layout kernels, the packed kernel and the finishers.
#pragma once
#include "scan_args.h"

namespace tpq {

// ---- shared pieces -----------------------------------------------------------------------

// s_waitcnt vmcnt(N) alone (gfx9 encoding: vmcnt [3:0] and [15:14], expcnt [6:4] and lgkmcnt [11:8] left at their maxima)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "six bits");
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

struct ProbeTable {  // lives in LDS
  int* start;        // [max_nprobe]
  int* size;         // [max_nprobe]
  int* tile_begin;   // [max_nprobe + 1] exclusive prefix of ceil(size/64)
};

// wave 0 fills the probe table; cells whose start equals the previous probe's start are
// skipped (ivfpq_topk.cu:864-866)
struct ProbeRegs {  // the first 64 probes' extents, one per lane (fetch_probes: the loads are issued early)
  int st, sz;
};
__device__ __forceinline__ ProbeRegs fetch_probes(const ScanArgs& a, int q, int n_probe, int base) {
  const int p = base + lane_id();
  ProbeRegs r{0, 0};
  if (p < n_probe) {
    r.st = (int)a.cell_start[(int64_t)q * a.max_nprobe + p];
    r.sz = (int)a.cell_size[(int64_t)q * a.max_nprobe + p];
    if (p > 0 && a.cell_start[(int64_t)q * a.max_nprobe + p - 1] == (int64_t)r.st) r.sz = 0;
    if (r.sz < 0) r.sz = 0;
  }
  return r;
}
__device__ __forceinline__ void build_probe_table(const ScanArgs& a, int q, int n_probe,
                                                  ProbeTable t, int tile_shift = 6,
                                                  const ProbeRegs* first = nullptr) {
  const int lane = lane_id();
  int running = 0;
  for (int base = 0; base < n_probe; base += 64) {
    const int p = base + lane;
    const ProbeRegs r = (base == 0 && first) ? *first : fetch_probes(a, q, n_probe, base);
    const int st = r.st, sz = r.sz;
    int tiles = (sz + (1 << tile_shift) - 1) >> tile_shift;
    int incl = tiles;  // inclusive wave scan
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (p < n_probe) {
      t.start[p] = st;
      t.size[p] = sz;
      t.tile_begin[p] = running + incl - tiles;
    }
    running += readlane_i(incl, 63);
  }
  if (lane == 0) t.tile_begin[n_probe] = running;
}

// lists travel as keys: `lv` holds the high words (value images), `li` the low words (~index)
template <int R>
__device__ __forceinline__ void store_list(const WaveTopK<R>& top, float* lv, int* li) {
  const int lane = lane_id();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    reinterpret_cast<unsigned*>(lv)[r * 64 + lane] = top.k[r].hi;
    reinterpret_cast<unsigned*>(li)[r * 64 + lane] = top.k[r].lo;
  }
}

template <int R>
__device__ __forceinline__ void merge_list(WaveTopK<R>& top, const float* lv, const int* li) {
  const int lane = lane_id();
#pragma unroll
  for (int r = 0; r < R; ++r)
    top.insert_sorted(Key{reinterpret_cast<const unsigned*>(lv)[r * 64 + lane],
                          reinterpret_cast<const unsigned*>(li)[r * 64 + lane]});
}

template <int R>
__device__ __forceinline__ void write_final(const ScanArgs& a, int q, const WaveTopK<R>& top) {
  const int lane = lane_id();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = r * 64 + lane;
    if (e < a.k) {
      const int idx = key_index(top.k[r]);
      const bool pad = (idx == kPadIdx);
      const int64_t adr = pad ? -1 : (int64_t)idx;
      a.out_vals[(int64_t)q * a.k + e] = pad ? -INFINITY : key_value(top.k[r]);
      a.out_addr[(int64_t)q * a.k + e] = adr;
      if (a.out_ids) a.out_ids[(int64_t)q * a.k + e] = pad ? -1 : a.address2id[adr];
    }
  }
}

// Cross-wave tree merge through LDS (`lv`/`li` may alias the dead LUT), then output.
template <int R>
__device__ __forceinline__ void finish_query(const ScanArgs& a, int q, int part,
                                             WaveTopK<R>& top, float* lv, int* li) {
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // every wave is done with the LUT
  for (int stride = 1; stride < kScanWaves; stride <<= 1) {
    if ((wave & (2 * stride - 1)) == stride) store_list<R>(top, lv + wave * R * 64, li + wave * R * 64);
    __syncthreads();
    if ((wave & (2 * stride - 1)) == 0)
      merge_list<R>(top, lv + (wave + stride) * R * 64, li + (wave + stride) * R * 64);
    __syncthreads();
  }
  if (wave == 0) {
    if (a.n_split == 1) {
      write_final<R>(a, q, top);
    } else {
      const int64_t o = ((int64_t)q * a.n_split + part) * (R * 64);
      store_list<R>(top, a.ws_vals + o, a.ws_idx + o);
    }
  }
}

// ---- LUT built inside the workgroup ("fused") ------------------------------------------------
// Instead of reading a materialised [m][nq][256] table (a-3 writes 655 MB and the scan reads it
// back at C2), the workgroup computes its query's LUT from the query and the PQ codebook, which
// stays L2-resident (m*ds KiB).  The arithmetic is adc_lut_kernel's, operation for operation --
// dot, |q|^2 and |c|^2 as ascending-dimension fma chains, then 2*dot, -|q|^2, -|c|^2 -- so the
// entries are bit-identical to tpq_adc_lut's.
__device__ __forceinline__ void stage_query(const ScanArgs& a, int q, float* xq, int n_threads) {
  const int d = a.m * a.ds;
  for (int i = threadIdx.x; i < d; i += n_threads) xq[i] = a.query[(int64_t)i * a.nq + q];
  __syncthreads();
}

__device__ __forceinline__ float4 fused_lut4(const ScanArgs& a, int j, int c4, const float* xq) {
  const float4* __restrict__ cb = reinterpret_cast<const float4*>(a.codebook) + (int64_t)j * a.ds * 64 + c4;
  float4 dot = make_float4(0.f, 0.f, 0.f, 0.f), c2 = dot;
  float q2 = 0.f;  // |q_j|^2, the same ascending-dimension chain in every thread that needs it
  for (int e = 0; e < a.ds; ++e) {
    const float4 y = cb[e * 64];
    const float x = xq[j * a.ds + e];
    q2 = fmaf(x, x, q2);
    dot.x = fmaf(x, y.x, dot.x); dot.y = fmaf(x, y.y, dot.y);
    dot.z = fmaf(x, y.z, dot.z); dot.w = fmaf(x, y.w, dot.w);
    c2.x = fmaf(y.x, y.x, c2.x); c2.y = fmaf(y.y, y.y, c2.y);
    c2.z = fmaf(y.z, y.z, c2.z); c2.w = fmaf(y.w, y.w, c2.w);
  }
  if (!a.euclid) return dot;
  float4 v;
  v.x = 2.f * dot.x; v.y = 2.f * dot.y; v.z = 2.f * dot.z; v.w = 2.f * dot.w;
  if (a.euclid == 2) return v;  // residual part1 = 2 q_j.r_jc (residual_part1_kernel)
  v.x = v.x - q2; v.y = v.y - q2; v.z = v.z - q2; v.w = v.w - q2;
  v.x = v.x - c2.x; v.y = v.y - c2.y; v.z = v.z - c2.z; v.w = v.w - c2.w;
  return v;
}

__device__ __forceinline__ void stage_lut_linear(const ScanArgs& a, int q, float* lut,
                                                 const float* xq) {
  // lut[j*256 + c] <- a.lut[(j*nq + q)*256 + c]; 16-byte loads, 1 KiB rows
  const float4* __restrict__ src = reinterpret_cast<const float4*>(a.lut);
  float4* dst = reinterpret_cast<float4*>(lut);
  for (int i = threadIdx.x; i < a.m * 64; i += kScanThreads) {
    const int j = i >> 6, c4 = i & 63;
    dst[i] = a.lut ? src[((int64_t)j * a.nq + q) * 64 + c4] : fused_lut4(a, j, c4, xq);
  }
}

// Merge of L sorted lists (best first) of LEN keys each, lying in LDS as hi[l * LEN + i], lo[...], BY RANK:
// the position of an entry in the merged order is its own position plus, for every other list, the number of
// that list's entries that precede it -- a fixed-step binary search per list, eight lists' searches in
// flight per lane.  Equal keys (a slot scanned twice) rank by list: no two entries share a position.  Entries
// that land below `cap` are scattered into ohi / olo (pre-filled with pads by the caller); one barrier on
// either side instead of the 2 log2(L) of a tree of pairwise merges, and no serial chain of bitonic networks
// (the workgroup's 8 x 64: 4.6 -> 3.9 us, and 4 % of the C2 batch).
template <int LEN>
__device__ __forceinline__ void rank_merge(const unsigned* __restrict__ hi, const unsigned* __restrict__ lo, int L,
                                           unsigned* __restrict__ ohi, unsigned* __restrict__ olo, int cap, int tid,
                                           int n_threads) {
  static_assert((LEN & (LEN - 1)) == 0, "power of two");
  for (int e = tid; e < L * LEN; e += n_threads) {
    const int l = e / LEN;
    const Key x{hi[e], lo[e]};
    if (key_index(x) == kPadIdx) continue;
    const unsigned long long xu = key_u64(x);
    int rank = e - l * LEN;
    for (int l0 = 0; l0 < L; l0 += 8) {
      int cnt[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) cnt[j] = 0;
      // y precedes x: y > x, or y == x in an earlier list
      // (branch-free: a list beyond L or the entry's own list is searched like the others -- in bounds -- and
      // its count dropped; with a branch per list the eight searches ran one after the other, 90 cycles a read)
      int base[8];
      bool use[8], tie[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int l2 = l0 + j;
        use[j] = l2 < L && l2 != l;
        tie[j] = l2 < l;
        base[j] = (l2 < L ? l2 : L - 1) * LEN;
      }
#pragma unroll
      for (int s = LEN / 2; s >= 1; s >>= 1) {
        unsigned yh[8], yl[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          yh[j] = hi[base[j] + cnt[j] + s - 1];
          yl[j] = lo[base[j] + cnt[j] + s - 1];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned long long yu = ((unsigned long long)yh[j] << 32) | yl[j];
          cnt[j] += (yu > xu || (yu == xu && tie[j])) ? s : 0;
        }
      }
      {
        unsigned yh[8], yl[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          yh[j] = hi[base[j] + cnt[j]];
          yl[j] = lo[base[j] + cnt[j]];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned long long yu = ((unsigned long long)yh[j] << 32) | yl[j];
          const int c = cnt[j] + ((yu > xu || (yu == xu && tie[j])) ? 1 : 0);
          rank += use[j] ? c : 0;
        }
      }
    }
    if (rank < cap) {
      ohi[rank] = x.hi;
      olo[rank] = x.lo;
    }
  }
}

}  // namespace tpq
