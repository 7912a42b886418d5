// IVFFlat16Index, large batches: the probed cells scanned CELL BY CELL on the fp16 matrix cores
// (tpq_ivf_flat16_cells_topk).  The pipeline is that of tpq_ivf_flat_cells_topk (the head of scan_flat_cells.hip) and
// stages 2, 3 and 5 are its kernels (scan_flat_cells_stages.h): threshold pass (the fp16 query-major scan over the first
// P0 probes, ivf_flat16_scan_topk_capped), seed, inversion by cell, candidates, finish.  The results are the bits of
// tpq_ivf_flat16_scan_topk: the finish kernel values every candidate with that scan's chain (slot_value,
// scan_flat_f16.h).  What is new here is the candidate kernel and the band it selects with.
//
// The candidate kernel (fc16_cand_kernel).  The stored halves ARE the A operand of v_mfma_f32_32x32x16_f16: a lane holds
// the 8 halves -- 4 storage words -- of k-group 8 (lane >> 5) ... + 7 of row lane & 31.  They go from global memory to
// the matrix cores as they lie: no conversion, half the bytes of the fp32 route into LDS, one MFMA per 32-row tile and
// 16 dimensions where the fp32 tile (32x32x2f32) takes eight.
//   Work item, persistent workgroups, item counter, the four waves x 32 query columns and the chunk of 256 slots are
//   fc_cand_kernel's.  Thread i stages slot cell_start + c0 + i: per slab of 16 dimensions 8 words, one per dimension
//   pair, rows n_slots words apart (a wave reads 256 contiguous bytes per row).  The staging thread widens the 16
//   halves and adds their squares to the slot's |x|^2, an ascending fmaf chain (low half, high half, words ascending);
//   a row outside the cell or the storage gets +inf.  The mask byte is read beside the first slab; live rows reach the
//   epilogue as ballot words.
//   LDS layout of a slab: [k-group 2][slot 256] units of 16 bytes, 8 KiB, two buffers (16 KiB), + |x|^2 1 KiB; neither
//   LDS nor registers depend on d.  Unit (g, s) holds words 4 g ... 4 g + 3 of slot s, i.e. exactly the A operand of
//   lane (g, s & 31) for tile s >> 5.  Chosen because both sides are then CONTIGUOUS 128-bit accesses: the staging
//   thread writes units (0, tid) and (1, tid) with two ds_write_b128, consecutive threads 16 bytes apart, and the MFMA
//   loop reads unit (half, 32 t + l31) with one ds_read_b128, the 32 lanes of a half-wave covering 512 consecutive bytes
//   and the other half-wave 4 KiB further on (a multiple of the bank period) -- a 128-bit access is served a quarter-wave
//   at a time, and 16 consecutive 16-byte units touch every bank once, so neither side has a bank conflict.  A
//   word-major layout ([word][slot], the fp32 route's) would need four 32-bit reads per operand.
//   The B operand is the lane's query column: the 8 fp32 components of its k-group are loaded one slab ahead, scaled
//   by the query's power of two, rounded to halves and packed in registers.  A slab whose upper k-group lies beyond d
//   (d = 8, 24, 40: d is a multiple of 8) is zero on both sides.
//   Eight accumulators of 16 fp32 per lane; epilogue, reservation (one returning atomic per column and chunk), list
//   stores and the overflow flag are fc_cand_kernel's:  fast = 2 dot - |x|^2 - |q|^2  (euclidean)  or  dot  (inner),
//   appended when the row is live and  !(fast < tau'_q - kb (|q|^2 + |x|^2)).  No spin wait; every loop is bounded by the
//   item count, the cell size or d.
//
// The band.  u = 2^-24, S = |q|^2 + |x|^2 in real numbers, x the STORED vector (the halves, exact).
//   One product.  Per query s = 2^e, e = 14 - floor(log2 max_i |q_i|), so the largest scaled component lies in
//   [2^14, 2^15) -- under the fp16 maximum with room for the rounding --; q' = s q is exact (a power of two), h = the
//   nearest half of q', and dot16 = 2^-e sum h_i x_i.  The MFMA multiplies the stored halves by h: an fp16 x fp16 product
//   has 22 significant bits and is exact in fp32, so the stored side contributes NO error.  fp16 subnormals are kept by
//   the instruction on both operands (measured on gfx950: 2^-24 x 1 gives 2^-24, 2^-24 x 2^-24 gives 2^-48), so stored
//   subnormals need no term.
//   the query   |h_i - q'_i| <= 2^-11 |q'_i| for a normal half, <= 2^-25 for a subnormal one:
//               |sum (h_i - q'_i) x_i| / s <= 2^-11 sum |q_i x_i| + (2^-25 / s) sum |x_i|
//               <= 2^-12 S + 2^-39 max|q_i| sqrt(d) |x|  <=  (2^-12 + 2^-40 sqrt(d)) S      (1 / s <= 2^-14 max|q_i|)
//   the sum     the instruction's order and rounding of the 16 products and the accumulator are not specified; taken
//               as ANY order with truncation (2 u per operation): <= 2 d u sum |h_i x_i| / s <= d u S (1 + 2^-11),
//               where the fp32 route has d u S / 2 for its fmaf chain.
//   the rest    |x|^2, |q|^2, the two subtractions, the specified chain and the test itself are the fp32 route's lines:
//               (4 d + 14) u S together with ITS dot term.
//   euclidean   fast = 2 dot16 - ...: both dot lines double:  (5 d + 14) u S + (2^-11 + 2^-39 sqrt(d)) S
//   inner       (2 d + 2) u S + (2^-12 + 2^-40 sqrt(d)) S
//   kb = 8 (d + 4) u (1 + 2^-8) + (2^-11 or 2^-12) (1 + 2^-6) + 2^-38 sqrt(d): about 5.6e-4 of S at d = 128, twelve times
//   the fp32 route's 4.7e-5 -- the price of the single product.  It costs candidates only (the counts are in DESIGN 3.21).
//   A hi + lo split of the query (two MFMAs per tile) would bring the band back to the fp32 route's; it was not built:
//   the single product is the recommended design and its candidate counts stay far below cand_cap on the measured set.
//   Absolute terms, subtracted from tau_q by the seed kernel (tau'_q; the finish kernel never reads it):
//               2^-146 always -- the unscaling ldexp rounds a subnormal result by at most 2^-150, twice for euclidean;
//               a query whose largest component is below 2^-86 would need e > 100: e is held at 100, the scaled
//               components are then small halves, and the subnormal line is no longer relative: (2^-25 / s) sum |x_i|
//               <= 2^-125 d 2^16 over finite halves, twice: tau'_q = tau_q - d 2^-107.  (A stored +-inf or NaN makes
//               |x|^2 +inf or NaN: the compare is unordered or against -inf and the row is admitted.)
//   No finite query is flagged for its range: the scale is exact from 2^-149 to FLT_MAX, and q2 and tau are the fp32
//   route's.  Underflow inside the fp32 chains is ignored here as it is there.
//   With this, every live row whose specified value is >= tau_q is appended, and the argument of scan_flat_cells.hip
//   carries over: the top-k, ties at the k-th place included, is among seeds and candidates.
//
// Flags are the fp32 route's: a non-finite component or |q|^2, tau_q = +inf, a listed cell outside [0, n_cells), an
// overflowing list.  The caller redoes those queries with tpq_ivf_flat16_scan_topk.
#include <cmath>

#include "scan_flat_cells_stages.h"
#include "scan_flat_f16.h"

namespace tpq {
namespace fcells {

constexpr int kF16SlabWords = 8;  // storage words per slot and slab: 16 dimensions
constexpr int kF16MaxExp = 100;   // the largest scale exponent (2^-25 / 2^100 is a normal float)

struct Fc16Args : FcArgsT<uint32_t> {
  int* qe;  // [nq] the query's scale exponent e (the workspace, behind the shared regions)
};

// stage 2's share of this route: the query's scale, and its absolute band terms off the threshold
struct Fc16Prep {
  int* qe;
  float shift_always, shift_clamped;
  __device__ __forceinline__ float operator()(const FcArgsT<uint32_t>& a, int q, float tau) const {
    float qmax = 0.f;
    const float* __restrict__ p = a.query + q;
    for (int i = 0; i < a.d; ++i) {
      qmax = fmaxf(qmax, fabsf(*p));
      p += a.nq;
    }
    int e = 0;
    float shift = shift_always;
    if (qmax > 0.f && qmax <= FLT_MAX) {  // (a non-finite query is flagged and never scaled)
      int x;
      (void)frexpf(qmax, &x);  // qmax in [2^(x-1), 2^x)
      e = 15 - x;
      if (e > kF16MaxExp) {
        e = kF16MaxExp;
        shift = shift_clamped;
      }
    }
    qe[q] = e;
    return tau - shift;
  }
};

struct FcValue16 {
  template <int METRIC>
  static __device__ __forceinline__ float value(const FcArgsT<uint32_t>& a, int s, int q) {
    return flat16::slot_value<METRIC, 1>(a.vectors + s, a.query + q, a.d, a.n_slots, a.nq);
  }
};

// ---- stage 4 ---------------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256, 2) void fc16_cand_kernel(Fc16Args a) {
  __shared__ u32x4 xs[2][2][kCsRows];  // [buffer][k-group][slot]: a lane's A operand is one unit
  __shared__ float c2s[kCsRows];
  __shared__ unsigned lmask[8];  // live rows of tile t
  __shared__ int item_s;
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int n_items = a.blk_off[a.n_cells];
  const int words = a.d >> 1;
  const int n_slabs = (a.d + 15) >> 4;
  for (;;) {
    if (tid == 0) item_s = atomicAdd(&a.ctrl[1], 1);
    __syncthreads();
    const int w = item_s;
    __syncthreads();  // (read by all before the next draw)
    if (w >= n_items) break;
    const int c = fc_item_cell(a, w);
    const int pb = a.cell_off[c] + (w - a.blk_off[c]) * kFcBlock;
    const int pe = pb + kFcBlock < a.cell_off[c + 1] ? pb + kFcBlock : a.cell_off[c + 1];
    const int st = a.cell_st[c], sz = a.cell_sz[c];
    const int pi = pb + wave * 32 + l31;
    const bool qvalid = pi < pe;
    const int q = qvalid ? a.pairs[pi] : 0;
    const int e = qvalid ? a.qe[q] : 0;
    const float* __restrict__ xq = a.query + q;
    for (int c0 = 0; c0 < sz; c0 += kCsRows) {
      const int off = c0 + tid;
      const int64_t s64 = (int64_t)st + off;
      const int row = (off < sz && s64 >= 0 && s64 < (int64_t)a.n_slots) ? (int)s64 : -1;  // (a cell that leaves the storage is cut)
      const bool cv = row >= 0;
      // (the strides, formed per chunk as scalars: see flat_range_walk, flat_range.hip)
      int row_stride = a.n_slots, col_stride = a.nq;
      asm volatile("" : "+s"(row_stride), "+s"(col_stride));
      const uint32_t* __restrict__ col = a.vectors + (cv ? row : 0);
      uint32_t xw[kF16SlabWords];
      float yn[8];
      float csq = 0.f;
      auto load_slab = [&](int kw) {  // the slab from word row kw
        const uint32_t* __restrict__ p = col + (int64_t)kw * row_stride;
#pragma unroll
        for (int u = 0; u < kF16SlabWords; ++u) {
          xw[u] = (cv && kw + u < words) ? *p : 0u;
          p += row_stride;
        }
      };
      auto load_y = [&](int kb) {  // the lane's k-group of the slab from dimension kb
        const float* __restrict__ p = xq + (int64_t)(kb + 8 * half) * col_stride;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          yn[j] = (qvalid && kb + 8 * half + j < a.d) ? *p : 0.f;
          p += col_stride;
        }
      };
      auto pack_y = [&]() {
        f16x8 b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (_Float16)ldexpf(yn[j], e);  // exact scale, then round to nearest even
        return b;
      };
      auto square_slab = [&]() {
#pragma unroll
        for (int u = 0; u < kF16SlabWords; ++u) {
          const float lo = flat16::low_half(xw[u]), hi = flat16::high_half(xw[u]);
          csq = fmaf(lo, lo, csq);
          csq = fmaf(hi, hi, csq);
        }
      };
      auto store_slab = [&](int buf) {
        xs[buf][0][tid] = u32x4{xw[0], xw[1], xw[2], xw[3]};
        xs[buf][1][tid] = u32x4{xw[4], xw[5], xw[6], xw[7]};
      };
      load_slab(0);
      load_y(0);
      __syncthreads();  // every wave finished the previous chunk (reads of xs, c2s and lmask)
      {
        // the mask byte, while the first slab's loads are in flight; a wave's ballot is tiles 2 wave and 2 wave + 1
        bool live = cv;
        if (cv && a.is_empty) live = a.is_empty[row] == 0;
        const unsigned long long m = __ballot(live);
        if (lane == 0) {
          lmask[2 * wave] = (unsigned)m;
          lmask[2 * wave + 1] = (unsigned)(m >> 32);
        }
      }
      square_slab();
      if (n_slabs == 1) c2s[tid] = cv ? csq : INFINITY;
      store_slab(0);
      f16x8 b = pack_y();
      f32x16 acc[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[t] = zero_f32x16();
      __syncthreads();
      for (int sb = 0; sb < n_slabs; ++sb) {
        const bool more = sb + 1 < n_slabs;
        if (more) {
          load_slab((sb + 1) * kF16SlabWords);
          load_y((sb + 1) * 16);
        }
        const u32x4* cur = &xs[sb & 1][half][l31];
#pragma unroll
        for (int t = 0; t < 8; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, cur[t * 32]), b, acc[t], 0, 0, 0);
        if (more) {
          square_slab();
          if (sb + 2 == n_slabs) c2s[tid] = cv ? csq : INFINITY;
          store_slab((sb + 1) & 1);
          b = pack_y();
        }
        __syncthreads();
      }
      // acc[t][r] = 2^e x (slot st + c0 + 32 t + sims_tile_row(r, half)) . (query column l31)
      const float tau = a.tau[q];
      const float q2 = a.qn[q];
      unsigned pm[4] = {0u, 0u, 0u, 0u};  // tile t: bits 16 (t & 1) ... of word t / 2
      int mine = 0;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        asm volatile("" ::: "memory");  // one tile's |x|^2 at a time: no LDS load moves ahead of its tile
        // the live bits of this half-wave's rows, in register order: row sims_tile_row(r, half) -> bit r
        const unsigned lh = (qvalid ? lmask[t] : 0u) >> (4 * half);
        const unsigned live16 = (lh & 0xfu) | ((lh >> 4) & 0xf0u) | ((lh >> 8) & 0xf00u) | ((lh >> 12) & 0xf000u);
        unsigned m = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x2 = c2s[t * 32 + sims_tile_row(r, half)];
          // (the unscaling is exact but for a subnormal result: the band's 2^-146)
          const float fast = METRIC == TPQ_METRIC_INNER ? ldexpf(acc[t][r], -e) : (ldexpf(acc[t][r], 1 - e) - x2) - q2;
          const float thr = tau - a.kb * (q2 + x2);
          m |= !(fast < thr) ? (1u << r) : 0u;
        }
        m &= live16;
        pm[t >> 1] |= m << (16 * (t & 1));
        mine += __popc(m);
      }
      const int other = __shfl_xor(mine, 32, 64);
      if (__ballot(mine != 0) == 0ull) continue;
      // one returning atomic per column: the lower half-wave's lane reserves both halves' positions
      int base = 0;
      if (half == 0 && mine + other > 0) base = atomicAdd(&a.cnt[q], mine + other);
      base = __shfl(base, l31, 64);
      if (half == 0 && mine + other > 0 && base + mine + other > a.cand_cap) a.flags[q] = 1;
      int at = base + (half ? other : 0);
      int* __restrict__ list = a.cand + (int64_t)q * a.cand_cap;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        unsigned m = (pm[t >> 1] >> (16 * (t & 1))) & 0xffffu;
        while (m != 0u) {
          const int r = __builtin_ctz(m);
          m &= m - 1u;
          if (at < a.cand_cap) list[at] = st + c0 + 32 * t + sims_tile_row(r, half);
          ++at;
        }
      }
    }
  }
}

static size_t fc16_workspace_bytes(int nq, int max_nprobe, int n_cells, int cand_cap, int p0) {
  return fc_workspace_bytes(nq, max_nprobe, n_cells, cand_cap, p0) + fc_align((size_t)nq * 4);
}

template <int METRIC>
static int fc16_launch(const Fc16Args& a, hipStream_t st) {
  // (the absolute terms of `The band`)
  const Fc16Prep prep{a.qe, ldexpf(1.f, -146), ldexpf((float)a.d, -107)};
  return fc_launch<METRIC, FcValue16>(a, prep, 0, st, [&](dim3 grid) -> int {
    hipLaunchKernelGGL(fc16_cand_kernel<METRIC>, grid, dim3(256), 0, st, a);
    TPQ_LAUNCH_CHECK("fc16_cand_kernel");
    return TPQ_OK;
  });
}

}  // namespace fcells
}  // namespace tpq

using namespace tpq;

static bool fc16_declined(int nq, int max_nprobe, int n_cells, int k, int cand_cap, int first_probe) {
  return nq <= 0 || max_nprobe < 1 || n_cells < 1 || k < 1 || k > 256 || cand_cap < 64 || cand_cap % 64 != 0 ||
         first_probe < 1;
}

extern "C" size_t tpq_ivf_flat16_cells_workspace_bytes(int nq, int max_nprobe, int n_cells, int k, int cand_cap,
                                                       int first_probe) {
  if (fc16_declined(nq, max_nprobe, n_cells, k, cand_cap, first_probe)) return 0;
  return fcells::fc16_workspace_bytes(nq, max_nprobe, n_cells, cand_cap, first_probe);
}

extern "C" int tpq_ivf_flat16_cells_topk(const uint32_t* vectors, const float* query, const uint8_t* is_empty,
                                         const int64_t* cells, const int64_t* cell_start, const int64_t* cell_size,
                                         const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                         int64_t n_slots, int n_cells, int d, int nq, int max_nprobe, int k, int metric,
                                         int first_probe, int cand_cap, void* workspace, size_t workspace_bytes,
                                         tpq_stream_t stream) {
  const char* what = "ivf_flat16_cells";
  if (d >= 1 && d % 8 != 0) {
    set_error("%s: d=%d is not supported: the fp16 tile takes whole k-groups of 8 dimensions", what, d);
    return TPQ_ERR_UNSUPPORTED;
  }
  bool go = false;
  const int checked = fcells::fc_check(
      what, vectors && query && cells && cell_start && cell_size && n_probe_list && out_vals && out_addr, n_slots, n_cells,
      d, nq, max_nprobe, k, metric, first_probe, cand_cap, &go);
  if (!go) return checked;
  if (int rc = need_ws(workspace, workspace_bytes,
                       fcells::fc16_workspace_bytes(nq, max_nprobe, n_cells, cand_cap, first_probe), what))
    return rc;
  fcells::Fc16Args a{};
  a.vectors = vectors; a.query = query; a.is_empty = is_empty; a.cells = cells;
  a.cell_start = cell_start; a.cell_size = cell_size; a.n_probe_list = n_probe_list;
  a.out_vals = out_vals; a.out_addr = out_addr;
  a.n_slots = (int)n_slots; a.n_cells = n_cells; a.d = d; a.nq = nq; a.max_nprobe = max_nprobe; a.k = k;
  a.p0 = first_probe; a.cand_cap = cand_cap;
  const double u = 1.0 / 16777216.0;
  a.kb = (float)(8.0 * (d + 4.0) * u * (1.0 + 1.0 / 256) +
                 (metric == TPQ_METRIC_NEG_SQ_L2 ? 1.0 / 2048 : 1.0 / 4096) * (1.0 + 1.0 / 64) +
                 sqrt((double)d) / 274877906944.0);  // 2^-38 sqrt(d)
  a.qe = reinterpret_cast<int*>(fcells::fc_carve(a, workspace));
  // stage 1: the exact top-k of the first P0 probes, one workgroup per query (no list workspace)
  if (int rc = ivf_flat16_scan_topk_capped(vectors, query, is_empty, cell_start, cell_size, n_probe_list, out_vals,
                                           out_addr, n_slots, d, nq, max_nprobe, k, metric, 1, first_probe, nullptr, 0,
                                           stream))
    return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? fcells::fc16_launch<TPQ_METRIC_NEG_SQ_L2>(a, st)
                                        : fcells::fc16_launch<TPQ_METRIC_INNER>(a, st);
}
