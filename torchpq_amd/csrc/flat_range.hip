// Range search over the whole database (tpq_flat_range_count / tpq_flat_range_fill): the fp32-MFMA similarity tile of
// flat_tile_kernel (sims_chunk.h) with a count epilogue and a fill epilogue; the caller's prefix sum stands between them.
// Nothing of size nq x n_slots exists: the state is one counter per (query, part) and the hits themselves.  Values,
// hits and order are defined in include/torchpq_amd.h.
#include "sims_chunk.h"
#include "row_select.h"

namespace tpq {

constexpr size_t kFrLds = (2 * kCsSlab + kCsRows) * sizeof(float) + 8 * sizeof(unsigned);   // 32 + 1 KiB and 8 mask words

// What both passes share.  grid (ceil(nq / 128), n_parts); part p walks the 256-slot chunks [p cpp, (p + 1) cpp) below
// n_chunks -- the cut of flat_tile_kernel.  A lane's query is the MFMA column l31 of its wave; its two half-waves hold the
// 2 x 16 rows of a 32-slot tile.  Per tile, tile(s0, pm, vv): s0 the tile's first slot, bit r of pm set where
// accumulator register r -- slot s0 + sims_tile_row(r, half) -- is a hit of this lane's query, vv[r] its value (the
// arithmetic of flat_tile_kernel, by the same calls).  The slots past n_slots are kept out by the live mask alone: they
// score -inf for -squared-L2 but 0 for the inner product.
template <class Tile>
__device__ __forceinline__ void flat_range_walk(const float* __restrict__ x, const float* __restrict__ Y,
                                                const int64_t* __restrict__ address2id, float thr, int d, int nq,
                                                int n_slots, int inner, int n_chunks, int chunks_per_part, Tile&& tile) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* cs = reinterpret_cast<float*>(smem);                       // [2][kCsKC][kCsRows]
  float* c2s = cs + 2 * kCsSlab;                                    // [kCsRows]
  unsigned* lmask = reinterpret_cast<unsigned*>(c2s + kCsRows);     // [8]: live slots of tile t
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int q = blockIdx.x * 128 + wave * 32 + l31;
  const bool qvalid = q < nq;
  const float* __restrict__ xq = x + (qvalid ? q : 0);
  const float q2 = sims_query_sq_norm(xq, d, nq);
  const int chunk0 = blockIdx.y * chunks_per_part;
  const int chunk1 = chunk0 + chunks_per_part < n_chunks ? chunk0 + chunks_per_part : n_chunks;
  for (int ch = chunk0; ch < chunk1; ++ch) {
    const int c0 = ch * kCsRows;
    // (the strides of the staging loads are the same in every chunk: left alone, the compiler forms two dozen 64-bit
    // row offsets ahead of this loop and spills them around the MFMA loop; formed per chunk they cost a few scalar
    // multiplies and no register across it)
    int row_stride = n_slots, col_stride = nq;
    asm volatile("" : "+s"(row_stride), "+s"(col_stride));
    f32x16 acc[8];
    sims_chunk_mfma(xq, qvalid, Y, c0, d, col_stride, row_stride, cs, c2s, acc, [&](bool cv) {
      // the chunk's live mask: thread i stages slot c0 + i, a wave's ballot is tiles 2 wave and 2 wave + 1
      bool live = cv;
      if (cv && address2id) live = address2id[c0 + (int)threadIdx.x] >= 0;
      const unsigned long long m = __ballot(live);
      if (lane == 0) {
        lmask[2 * wave] = (unsigned)m;
        lmask[2 * wave + 1] = (unsigned)(m >> 32);
      }
    });
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      asm volatile("" ::: "memory");   // one tile's |y|^2 and values at a time: no LDS load moves ahead of its tile
      // the live bits of this half-wave's rows, in register order: row sims_tile_row(r, half) -> bit r
      const unsigned lh = (qvalid ? lmask[t] : 0u) >> (4 * half);
      const unsigned live16 = (lh & 0xfu) | ((lh >> 4) & 0xf0u) | ((lh >> 8) & 0xf00u) | ((lh >> 12) & 0xf000u);
      unsigned pm = 0;
      float vv[16];
#pragma unroll
      for (int r = 15; r >= 0; --r) {
        const int cl = sims_tile_row(r, half);
        float v = inner ? acc[t][r] : neg_sq_l2(acc[t][r], q2, c2s[t * 32 + cl]);
        v = v + 0.0f;  // -0.0 -> +0.0, as the top-k's keys have it
        vv[r] = v;
        // not below the threshold: false for a NaN on either side.  (Shifted in from the right, last register first:
        // sixteen masks 1 << r, and sixteen 1 << row for the live test, would each sit in a register.)
        pm = (pm << 1) | (unsigned)(v >= thr);
      }
      pm &= live16;
      tile(c0 + t * 32, pm, vv);
    }
  }
}

// Pass 1: counts[q * n_parts + part] = the hits of query q in the part's chunks.  Every segment of the call is
// written: a part beyond the last chunk, or n_slots == 0, writes 0.
__global__ __launch_bounds__(256, 2) void flat_range_count_kernel(const float* __restrict__ x, const float* __restrict__ Y,
                                                                  const int64_t* __restrict__ address2id,
                                                                  const float* __restrict__ threshold,
                                                                  int32_t* __restrict__ counts, int d, int nq, int n_slots,
                                                                  int inner, int n_chunks, int chunks_per_part) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 128 + (threadIdx.x >> 6) * 32 + (lane & 31);
  const bool qvalid = q < nq;
  int cnt = 0;   // of this half-wave's 16 rows of every tile
  flat_range_walk(x, Y, address2id, qvalid ? threshold[q] : 0.f, d, nq, n_slots, inner, n_chunks, chunks_per_part,
                  [&](int, unsigned pm, const float (&)[16]) { cnt += __popc(pm); });
  cnt += __shfl_xor(cnt, 32, 64);
  if (qvalid && lane < 32) counts[(int64_t)q * gridDim.y + blockIdx.y] = cnt;
}

// Pass 2: the hits of segment q * n_parts + part go to offsets[seg] onwards, address ascending.  A tile's 32 rows
// alternate between the half-waves in groups of four (sims_tile_row): rows 8 g ... 8 g + 3 are registers 4 g ... 4 g + 3
// of half 0, rows 8 g + 4 ... 8 g + 7 the same registers of half 1.  So a lane needs the other half's four group counts
// (0 ... 4 each: 4 x 3 bits, one exchange per tile) to place its own four groups.  Nothing is stored at or beyond
// offsets[seg + 1]: inputs that changed since the count pass lose hits, they do not leave the segment.
__global__ __launch_bounds__(256, 2) void flat_range_fill_kernel(const float* __restrict__ x, const float* __restrict__ Y,
                                                                 const int64_t* __restrict__ address2id,
                                                                 const float* __restrict__ threshold,
                                                                 const int64_t* __restrict__ offsets,
                                                                 float* __restrict__ out_vals, int64_t* __restrict__ out_addr,
                                                                 int64_t* __restrict__ out_ids, int d, int nq, int n_slots,
                                                                 int inner, int n_chunks, int chunks_per_part) {
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5;
  const int q = blockIdx.x * 128 + (threadIdx.x >> 6) * 32 + (lane & 31);
  const bool qvalid = q < nq;
  int64_t o = 0, end = 0;   // the cursor (the same in both half-waves) and the segment's end
  if (qvalid) {
    const int64_t seg = (int64_t)q * gridDim.y + blockIdx.y;
    o = offsets[seg];
    end = offsets[seg + 1];
  }
  if (!__syncthreads_or(end > o)) return;   // none of the block's 128 segments holds a hit
  flat_range_walk(x, Y, address2id, qvalid ? threshold[q] : 0.f, d, nq, n_slots, inner, n_chunks, chunks_per_part,
                  [&](int s0, unsigned pm, const float (&vv)[16]) {
                    if (__ballot(pm != 0u) == 0ull) return;
                    unsigned mine = 0;
#pragma unroll
                    for (int g = 0; g < 4; ++g) mine |= (unsigned)__popc((pm >> (4 * g)) & 15u) << (3 * g);
                    const unsigned other = (unsigned)__shfl_xor((int)mine, 32, 64);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                      const int n_mine = (mine >> (3 * g)) & 7u, n_other = (other >> (3 * g)) & 7u;
                      int64_t at = o + (half ? n_other : 0);
#pragma unroll
                      for (int r = 4 * g; r < 4 * g + 4; ++r) {
                        if ((pm >> r) & 1u) {
                          if (at < end) {
                            const int s = s0 + sims_tile_row(r, half);
                            out_vals[at] = vv[r];
                            out_addr[at] = (int64_t)s;
                            if (out_ids) out_ids[at] = address2id[s];
                          }
                          ++at;
                        }
                      }
                      o += n_mine + n_other;
                    }
                  });
}

// the argument checks both entry points share (those of tpq_flat_topk); TPQ_OK: go on
static int flat_range_check(const char* what, bool pointers, const int64_t* address2id, const int64_t* out_ids,
                            int64_t n_slots, int d, int nq, int metric, int n_parts) {
  TPQ_REQUIRE(pointers, "%s: null pointer argument", what);
  TPQ_REQUIRE(address2id || !out_ids, "%s: out_ids needs address2id", what);
  TPQ_REQUIRE(d >= 1 && nq >= 0 && n_slots >= 0, "%s: bad shape d=%d nq=%d n_slots=%lld", what, d, nq,
              (long long)n_slots);
  TPQ_REQUIRE(n_parts >= 1 && n_parts <= 1024, "%s: n_parts=%d out of range (1 ... 1024)", what, n_parts);
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "%s: bad metric %d", what, metric);
  if (n_slots >= 2147483647LL) {
    set_error("%s: n_slots=%lld: addresses are 31-bit (n_slots < 2^31 - 1)", what, (long long)n_slots);
    return TPQ_ERR_UNSUPPORTED;
  }
  return TPQ_OK;
}

}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_flat_range_segments(int nq, int n_parts) {
  if (nq <= 0 || n_parts < 1 || n_parts > 1024) return 0;
  return (size_t)nq * (size_t)n_parts;
}

extern "C" int tpq_flat_range_count(const float* vectors, const float* query, const int64_t* address2id,
                                    const float* threshold, int32_t* counts, int64_t n_slots, int d, int nq, int metric,
                                    int n_parts, tpq_stream_t stream) {
  const int rc = flat_range_check("flat_range_count", vectors && query && threshold && counts, address2id, nullptr,
                                  n_slots, d, nq, metric, n_parts);
  if (rc) return rc;
  if (nq == 0) return TPQ_OK;
  const int n_chunks = (int)((n_slots + kCsRows - 1) / kCsRows);
  return launch_with_lds(flat_range_count_kernel, "flat_range_count_kernel", dim3((nq + 127) / 128, n_parts), dim3(256),
                         kFrLds, reinterpret_cast<hipStream_t>(stream), query, vectors, address2id, threshold, counts, d,
                         nq, (int)n_slots, (int)(metric == TPQ_METRIC_INNER), n_chunks,
                         (n_chunks + n_parts - 1) / n_parts);
}

extern "C" int tpq_flat_range_fill(const float* vectors, const float* query, const int64_t* address2id,
                                   const float* threshold, const int64_t* offsets, float* out_vals, int64_t* out_addr,
                                   int64_t* out_ids, int64_t n_slots, int d, int nq, int metric, int n_parts,
                                   tpq_stream_t stream) {
  const int rc = flat_range_check("flat_range_fill", vectors && query && threshold && offsets && out_vals && out_addr,
                                  address2id, out_ids, n_slots, d, nq, metric, n_parts);
  if (rc) return rc;
  if (nq == 0 || n_slots == 0) return TPQ_OK;   // (no slots: no hits)
  const int n_chunks = (int)((n_slots + kCsRows - 1) / kCsRows);
  return launch_with_lds(flat_range_fill_kernel, "flat_range_fill_kernel", dim3((nq + 127) / 128, n_parts), dim3(256),
                         kFrLds, reinterpret_cast<hipStream_t>(stream), query, vectors, address2id, threshold, offsets,
                         out_vals, out_addr, out_ids, d, nq, (int)n_slots, (int)(metric == TPQ_METRIC_INNER), n_chunks,
                         (n_chunks + n_parts - 1) / n_parts);
}
