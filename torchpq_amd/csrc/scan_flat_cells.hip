// IVFFlatIndex, large batches: the probed cells scanned CELL BY CELL on the fp32 matrix cores (tpq_ivf_flat_cells_topk).
//
// scan_flat_kernel reads the 4 d bytes of a slot once per query that probes its cell.  Here a cell's vectors are read
// once per block of 128 of the queries that list it, and the block's values come from the fp32-MFMA similarity chunk of
// sims_chunk.h (sims_rows_mfma, sims_rows.h): 256 slots x 128 queries per chunk, the 16-dimension slabs of the cell
// double-buffered in LDS.  The MFMA value cannot be the value include/torchpq_amd.h specifies (one fp32 operation per
// step, no fma), so it SELECTS only: every slot that may belong to a query's top-k is appended to the query's candidate
// list, and the finish kernel evaluates the candidates with the specified chain -- the returned bits are the scan's.
//
// Five stages on the caller's stream, no host read, no allocation:
//   1  threshold   today's scan_flat_kernel over each query's first P0 = first_probe probes (ivfflat_scan_topk_capped,
//                  scan_flat.hip): their exact top-k lands in the outputs.  tau_q = the k-th value (-inf: fewer than k).
//   2  fc_seed_kernel     a thread per query: |q|^2 (the ascending fmaf chain of sims_query_sq_norm), tau_q, a zero
//                  candidate counter, the flag of a query that must not take part (below).  Over its grid it also zeroes
//                  the histogram of the inversion and the control words.
//   3  fc_count_kernel, fc_scan_kernel, fc_scatter_kernel     the pairs (q, p), P0 <= p < n_probe_list[q], grouped by
//                  probed cell.  One workgroup per slice of kFcSlice consecutive queries counts its pairs per cell with
//                  LDS atomics and spends ONE global atomic per (slice, non-empty cell) -- one per pair puts hundreds of
//                  same-address atomics on every cell of a cell-dense batch (DESIGN 3.1 stage 3) --; one block forms the
//                  exclusive prefixes of pairs and of blocks of kFcBlock pairs; the scatter counts again, reserves the
//                  slice's positions in every cell with one RETURNING atomic and places the pairs from LDS cursors.  The
//                  LDS histogram covers kFcWindow cells at a time: an index with more cells takes several passes over
//                  the slice's pairs.  A probe whose start equals the previous probe's start writes no pair (the scan
//                  skips it); a cell listed twice, not in a row, writes two (the scan reads it twice).  The order
//                  inside a cell varies from run to run; nothing downstream depends on it.
//   4  fc_cand_kernel     the hot kernel, below.
//   5  fc_finish_kernel   a wave per unflagged query: the k seeds of stage 1 enter a WaveSelector with the values they
//                  have, every candidate address is valued with the specified chain -- a lane per candidate, dimensions
//                  ascending, kFcUnroll row loads in flight, the loop of scan_flat_kernel -- and enters unless its
//                  value is NaN or below the selector's threshold; [k] values and addresses, (-inf, -1) pads.
//
// The candidate kernel.  Work item: (cell, block of <= 128 of its pairs) -- four waves x 32 MFMA columns, a lane owns one
// query column (tau_q and |q|^2 in registers through the epilogue; the two half-waves share a column and split a tile's 32 rows).  Persistent
// workgroups, two per CU, draw items from a counter; items are numbered cell by cell, not longest first (not measured).
// Per item the workgroup walks the cell in chunks of 256 slots: thread i stages slot cell_start + c0 + i of the
// dimension-major storage (a wave reads 256 contiguous bytes per dimension) unless it lies past the cell's end or the
// storage, accumulates its |x|^2, and reads its mask byte alongside the first slab; the live rows reach the epilogue as
// one ballot word per tile.  LDS (33 KiB) and registers do not depend on d.
// Epilogue, per lane and row:   fast = 2 dot - |x|^2 - |q|^2   (euclidean)   or   dot   (inner product);
//   the row is appended when it is live and   !(fast < tau_q - delta),   delta = kb (|q|^2 + |x|^2).
// The negated compare admits on an unordered compare; tau_q = -inf admits every live row.  A lane counts its admitted
// rows of the whole chunk, reserves their positions in the query's list with ONE returning atomic per column and chunk
// (the lower half-wave's lane adds both halves' counts), and stores the slot addresses.  Beyond cand_cap nothing is
// stored and the query is flagged.
//
// The band.  u = 2^-24 (fp32, round to nearest), gamma_n = n u / (1 - n u), S = |q|^2 + |x|^2 in real numbers.
// dot and both norms are ascending fmaf chains of d steps (the MFMA accumulates as fmaf does: sims_chunk.h), so
//   |fl(dot) - q.x| <= gamma_d sum |q_i x_i| <= gamma_d S / 2,    |fl(|x|^2) - |x|^2| <= gamma_d |x|^2, likewise |q|^2.
//   euclidean   2 dot is exact; the two subtractions round numbers below 2 S (1 + gamma_d) each:
//               |fast - g| <= (2 gamma_d + 4 u (1 + gamma_d)) S          g = -|q - x|^2
//               the specified chain: t = fl(q_i - x_i), fl(t t), d subtractions -- every term carries at most d + 3
//               roundings:  |chain - g| <= gamma_{d+3} sum (q_i - x_i)^2 <= 2 gamma_{d+3} S
//               together  <= (4 d + 10) u S (1 + o(1))
//   inner       |fast - q.x| <= gamma_d S / 2,  |chain - q.x| <= gamma_{d+1} S / 2:  together <= (d + 1) u S
//   the test    fl(|q|^2) + fl(|x|^2), the product with kb and tau_q - delta each round once: delta is formed from
//               S (1 - gamma_d - 2 u) at worst, and the last subtraction moves the threshold by u (|tau_q| + delta);
//               a tau_q below -3 S admits every row whatever its rounding, so this is <= 4 u S where it matters.
// (4 d + 14) u S covers all of it; kb = 6 (d + 4) u (1 + 2^-8) -- c = 6 where 4 would do, WIDENED on purpose: the second
// order terms (gamma against n u: a factor 1.004 at d = 65 536) and the rounding of kb itself are inside it with room to
// spare, and the band is still 5e-5 of S at d = 128: it costs candidates only where values tie to that precision.
// So every live row whose specified value is >= tau_q has fast >= tau_q - delta and is appended; tau_q is the k-th
// best of a subset of the query's candidates, hence <= the final k-th value: the top-k, ties at the k-th place
// included, is among seeds and candidates.  The finish kernel orders them by (value descending, address ascending).
// Where S kb overflows, delta is +inf or NaN and the row is admitted; a tau_q of +inf flags the query.
//
// Flags.  flags[q] != 0: the query's row of the outputs is NOT the result (it holds stage 1's).  Set by the seed kernel
// for a query that has probes beyond P0 and a NaN or +-Inf component (|q|^2 is then not finite), a non-finite |q|^2, a
// tau_q of +inf, or a listed cell outside [0, n_cells); by the candidate kernel for a list that overflowed.  The finish
// kernel counts them into the workspace's first word; the caller redoes those queries with tpq_ivfflat_scan_topk.
//
// Stages 2, 3 and 5, the workspace and the launch sequence are in scan_flat_cells_stages.h, which the fp16 lists' route
// (scan_flat_f16_cells.hip) shares; this unit holds the fp32 candidate kernel and the fp32 value of a candidate.
#include <atomic>

#include "scan_flat_cells.h"
#include "scan_flat_cells_stages.h"
#include "sims_rows.h"

namespace tpq {
namespace fcells {

using FcArgs = FcArgsT<float>;

// ---- stage 4 ---------------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256, 2) void fc_cand_kernel(FcArgs a) {
  __shared__ __attribute__((aligned(16))) float cs[2 * kCsSlab];  // [2][kCsKC][kCsRows]
  __shared__ float c2s[kCsRows];
  __shared__ unsigned lmask[8];  // live rows of tile t
  __shared__ int item_s;
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int n_items = a.blk_off[a.n_cells];
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
    const float* __restrict__ xq = a.query + q;
    for (int c0 = 0; c0 < sz; c0 += kCsRows) {
      const int off = c0 + tid;
      const int64_t s64 = (int64_t)st + off;
      const int row = (off < sz && s64 >= 0 && s64 < (int64_t)a.n_slots) ? (int)s64 : -1;  // (a cell that leaves the storage is cut)
      // (the strides, formed per chunk as scalars: see flat_range_walk, flat_range.hip)
      int row_stride = a.n_slots, col_stride = a.nq;
      asm volatile("" : "+s"(row_stride), "+s"(col_stride));
      f32x16 acc[8];
      sims_rows_mfma(xq, qvalid, a.vectors, row, a.d, col_stride, row_stride, cs, c2s, acc, [&](bool cv) {
        // the mask byte, while the first slab's loads are in flight; a wave's ballot is tiles 2 wave and 2 wave + 1
        bool live = cv;
        if (cv && a.is_empty) live = a.is_empty[row] == 0;
        const unsigned long long m = __ballot(live);
        if (lane == 0) {
          lmask[2 * wave] = (unsigned)m;
          lmask[2 * wave + 1] = (unsigned)(m >> 32);
        }
      });
      // acc[t][r] = (slot st + c0 + 32 t + sims_tile_row(r, half), query column l31).  tau_q and |q|^2 are read per
      // chunk, behind the MFMA loop: held across it they cost the two registers that made the kernel spill
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
          const float dot = acc[t][r];
          const float fast = METRIC == TPQ_METRIC_INNER ? dot : (2.f * dot - x2) - q2;
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

// ---- stage 5 ---------------------------------------------------------------------------------------------------------
// the specified value of slot s for query q: the loop of scan_flat_kernel, the query read from global memory (the same
// address in every lane)
template <int METRIC>
__device__ __forceinline__ float fc_slot_value(const float* __restrict__ col, const float* __restrict__ xq, int d,
                                               int64_t stride, int64_t qstride) {
  float v = 0.f;
  int i = 0;
  for (; i + kFcUnroll <= d; i += kFcUnroll) {
    float x[kFcUnroll], y[kFcUnroll];
#pragma unroll
    for (int u = 0; u < kFcUnroll; ++u) {
      x[u] = col[(int64_t)u * stride];
      y[u] = xq[(int64_t)u * qstride];
    }
    col += (int64_t)kFcUnroll * stride;
    xq += (int64_t)kFcUnroll * qstride;
#pragma unroll
    for (int u = 0; u < kFcUnroll; ++u) v = metric_step<METRIC>(v, y[u], x[u]);
  }
  for (; i < d; ++i) {
    v = metric_step<METRIC>(v, *xq, *col);
    col += stride;
    xq += qstride;
  }
  return v;
}

struct FcValue32 {
  template <int METRIC>
  static __device__ __forceinline__ float value(const FcArgs& a, int s, int q) {
    return fc_slot_value<METRIC>(a.vectors + s, a.query + q, a.d, a.n_slots, a.nq);
  }
};

// ---- host ------------------------------------------------------------------------------------------------------------
static std::atomic<int> g_stop_after{0};

template <int METRIC>
static int fc_launch32(const FcArgs& a, int stop, hipStream_t st) {
  return fc_launch<METRIC, FcValue32>(a, FcNoPrep{}, stop, st, [&](dim3 grid) -> int {
    hipLaunchKernelGGL(fc_cand_kernel<METRIC>, grid, dim3(256), 0, st, a);
    TPQ_LAUNCH_CHECK("fc_cand_kernel");
    return TPQ_OK;
  });
}

}  // namespace fcells
}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivf_flat_cells_workspace_bytes(int nq, int max_nprobe, int n_cells, int k, int cand_cap,
                                                    int first_probe) {
  if (nq <= 0 || max_nprobe < 1 || n_cells < 1 || k < 1 || k > 256 || cand_cap < 64 || cand_cap % 64 != 0 ||
      first_probe < 1)
    return 0;
  return fcells::fc_workspace_bytes(nq, max_nprobe, n_cells, cand_cap, first_probe);
}

extern "C" int tpq_ivf_flat_cells_stop_after(int stage) {
  return fcells::g_stop_after.exchange(stage >= 1 && stage <= 4 ? stage : 0);
}

extern "C" int tpq_ivf_flat_cells_topk(const float* vectors, const float* query, const uint8_t* is_empty,
                                      const int64_t* cells, const int64_t* cell_start, const int64_t* cell_size,
                                      const int64_t* n_probe_list, float* out_vals, int64_t* out_addr, int64_t n_slots,
                                      int n_cells, int d, int nq, int max_nprobe, int k, int metric, int first_probe,
                                      int cand_cap, void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  const char* what = "ivfflat_cells";
  bool go = false;
  const int checked = fcells::fc_check(
      what, vectors && query && cells && cell_start && cell_size && n_probe_list && out_vals && out_addr, n_slots, n_cells,
      d, nq, max_nprobe, k, metric, first_probe, cand_cap, &go);
  if (!go) return checked;
  if (int rc = need_ws(workspace, workspace_bytes, fcells::fc_workspace_bytes(nq, max_nprobe, n_cells, cand_cap, first_probe),
                       what))
    return rc;
  fcells::FcArgs a{};
  a.vectors = vectors; a.query = query; a.is_empty = is_empty; a.cells = cells;
  a.cell_start = cell_start; a.cell_size = cell_size; a.n_probe_list = n_probe_list;
  a.out_vals = out_vals; a.out_addr = out_addr;
  a.n_slots = (int)n_slots; a.n_cells = n_cells; a.d = d; a.nq = nq; a.max_nprobe = max_nprobe; a.k = k;
  a.p0 = first_probe; a.cand_cap = cand_cap;
  a.kb = (float)(6.0 * (d + 4.0) / 16777216.0 * (1.0 + 1.0 / 256));
  fcells::fc_carve(a, workspace);
  const int stop = fcells::g_stop_after.load();
  // stage 1: the exact top-k of the first P0 probes, one workgroup per query (no list workspace)
  if (int rc = ivfflat_scan_topk_capped(vectors, query, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                                        n_slots, d, nq, max_nprobe, k, metric, 1, first_probe, nullptr, 0, stream))
    return rc;
  if (stop == 1) return TPQ_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return metric == TPQ_METRIC_NEG_SQ_L2 ? fcells::fc_launch32<TPQ_METRIC_NEG_SQ_L2>(a, stop, st)
                                        : fcells::fc_launch32<TPQ_METRIC_INNER>(a, stop, st);
}
