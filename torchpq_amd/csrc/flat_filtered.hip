// Exact search among allowed ids (tpq_flat_topk_filtered, tpq_flat_range_filtered_count / _fill): the work scales with
// the number of ALLOWED slots, not with the capacity.  A workgroup owns a group -- at most 128 queries that use one
// row of filter bits -- and a slot range; it compacts the set bits of its part of the row into an LDS list of ascending
// addresses, and whenever 256 are pending runs the fp32-MFMA similarity chunk of sims_chunk.h on those GATHERED rows:
// thread i stages row list[i] instead of c0 + i.  A row's dot product and norm do not depend on where in a chunk the row
// sits, so the values are those of tpq_flat_topk, bit for bit, and the epilogues are those of flat_tile_kernel and
// flat_range_walk with a tile row's slot number read from the address list.  Liveness (address2id >= 0) is tested after
// the compaction, for allowed slots only, and becomes the chunk's live mask.  The semantics are in include/torchpq_amd.h.
#include "flat_merge.h"
#include "sims_rows.h"

namespace tpq {

constexpr int kFfWords = 256;                       // filter words per gather step: one per thread, 8192 slots
constexpr int kFfList = kCsRows + 32 * kFfWords;    // the list: fewer than 256 pending + every bit of one step
// the gather's LDS: the list, the slot numbers of the chunk in flight, the waves' totals of two steps
constexpr size_t kFfGatherLds = (size_t)(kFfList + kCsRows + 8) * sizeof(int);
constexpr size_t kFfTopkLds = kFtLds + kFfGatherLds;                                          // 98 + 34 KiB: one block per CU
constexpr size_t kFfRangeLds = (2 * kCsSlab + kCsRows) * sizeof(float) + 8 * sizeof(unsigned) + kFfGatherLds;   // 33 + 34 KiB

// the group tables of a call (built by the caller, see the header)
struct FfGroups {
  const int32_t* __restrict__ query_order;   // [nq]
  const int32_t* __restrict__ group_begin;   // [n_groups + 1] into query_order
  const int32_t* __restrict__ group_row;     // [n_groups]; < 0: the row allows nothing
  const unsigned* __restrict__ bits;         // [n_filters][stride]
  int64_t stride;
  int n_filters;
};

// this lane's query of group blockIdx.x (the ORIGINAL query number; MFMA column l31 of its wave), or -1
__device__ __forceinline__ int ff_lane_query(const FfGroups& g, int nq) {
  const int b = g.group_begin[blockIdx.x], e = g.group_begin[blockIdx.x + 1];
  const int i = b + (int)(threadIdx.x >> 6) * 32 + (int)(threadIdx.x & 31);
  if (i >= e || i >= b + 128 || i < 0 || i >= nq) return -1;
  const int q = g.query_order[i];
  return (q >= 0 && q < nq) ? q : -1;
}

// the group's row of bits, or nullptr where it allows nothing
__device__ __forceinline__ const unsigned* ff_group_bits(const FfGroups& g) {
  const int row = g.group_row[blockIdx.x];
  return (row >= 0 && row < g.n_filters) ? g.bits + (int64_t)row * g.stride : nullptr;
}

// The gather.  Part blockIdx.y of the row `bits`: the slots of the 256-slot chunks [p cpp, (p + 1) cpp) below n_chunks
// -- the cut of flat_tile_kernel -- and below n_slots.  A step reads one word per thread (a zero word costs its load
// and the test of the store loop), places the wave's set bits by a prefix sum of popcounts (skipped by a wave whose
// 64 words are all zero) and the waves by their totals through LDS: the list ascends, and nothing is atomic.
// chunk(row) runs on every thread of the block once 256 addresses are pending -- row = this thread's address -- and
// once more for what is left when the part ends (row = -1 beyond the last).  list [kFfList] and wtot [8] are LDS.
template <class Chunk>
__device__ __forceinline__ void ff_gather_walk(const unsigned* __restrict__ bits, int n_slots, int n_chunks,
                                               int chunks_per_part, int* list, int* wtot, Chunk&& chunk) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int chunk0 = blockIdx.y * chunks_per_part;
  const int chunk1 = chunk0 + chunks_per_part < n_chunks ? chunk0 + chunks_per_part : n_chunks;
  if (bits == nullptr || chunk0 >= chunk1) return;
  const int64_t end64 = (int64_t)chunk1 * kCsRows;
  const int s1 = end64 < n_slots ? (int)end64 : n_slots;   // the part's slots end here
  const int w0 = chunk0 * (kCsRows / 32), w1 = (int)(((int64_t)s1 + 31) >> 5);
  int pending = 0, par = 0;   // (both the same in every thread)
  for (int wb = w0; wb < w1; wb += kFfWords) {
    const int wi = wb + (int)threadIdx.x;
    unsigned w = wi < w1 ? bits[wi] : 0u;
    if (wi == w1 - 1 && (s1 & 31)) w &= (1u << (s1 & 31)) - 1u;   // a stale bit at or beyond n_slots
    const int c = __popc(w);
    int upto = c;   // ... and the words of the lanes below
    if (__ballot(w != 0u) != 0ull) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(upto, o, 64);
        if (lane >= o) upto += v;
      }
    }
    if (lane == 63) wtot[par * 4 + wave] = upto;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tj = wtot[par * 4 + j];
      total += tj;
      before += j < wave ? tj : 0;
    }
    par ^= 1;   // (the next step's totals go to the other four words: a wave may still be reading these)
    int at = pending + before + upto - c;
    const int base = wi << 5;
    while (w != 0u) {
      list[at++] = base + __builtin_ctz(w);
      w &= w - 1u;
    }
    pending += total;
    if (pending >= kCsRows) {
      __syncthreads();
      int head = 0;
      for (; pending - head >= kCsRows; head += kCsRows) chunk(list[head + (int)threadIdx.x]);
      const int rem = pending - head;
      const int keep = (int)threadIdx.x < rem ? list[head + (int)threadIdx.x] : 0;
      __syncthreads();
      if ((int)threadIdx.x < rem) list[threadIdx.x] = keep;
      pending = rem;
    }
  }
  if (pending > 0) {
    __syncthreads();
    chunk((int)threadIdx.x < pending ? list[threadIdx.x] : -1);
  }
}

// what a chunk's staged() does in all three kernels: the slot numbers of the chunk's rows for the epilogue, and the live
// mask from address2id -- read for gathered (allowed) slots only; a wave's ballot is tiles 2 wave and 2 wave + 1
__device__ __forceinline__ void ff_stage_rows(bool cv, int row, const int64_t* __restrict__ address2id, int* rows,
                                              unsigned* lmask) {
  rows[threadIdx.x] = row;
  bool live = cv;
  if (cv && address2id) live = address2id[row] >= 0;
  const unsigned long long m = __ballot(live);
  if ((threadIdx.x & 63) == 0) {
    lmask[2 * (threadIdx.x >> 6)] = (unsigned)m;
    lmask[2 * (threadIdx.x >> 6) + 1] = (unsigned)(m >> 32);
  }
}

// Top-k, pass 1.  grid (n_groups, n_parts).  flat_tile_kernel's queues, threshold and fold, per lane for its query of
// the group; the lists in the workspace are indexed by the original query number, so flat_merge_kernel reads them as
// it reads flat_tile_kernel's.  A group whose row allows nothing, and a part without an allowed slot, still write
// their lists (pads): the merge reads n_parts lists of every query.
template <int R>
__global__ __launch_bounds__(256, 1) void flat_filtered_tile_kernel(const float* __restrict__ x, const float* __restrict__ Y,
                                                                    const int64_t* __restrict__ address2id, FfGroups groups,
                                                                    unsigned long long* __restrict__ lists, int d, int nq,
                                                                    int n_slots, int k, int inner, int n_chunks,
                                                                    int chunks_per_part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* qs = reinterpret_cast<unsigned long long*>(smem);            // [128][kFtStride]
  float* cs = reinterpret_cast<float*>(qs + 128 * kFtStride);                       // [2][kCsKC][kCsRows]
  float* c2s = cs + 2 * kCsSlab;                                                   // [kCsRows]
  unsigned* lmask = reinterpret_cast<unsigned*>(c2s + kCsRows);                    // [8]: live rows of tile t
  int* rows = reinterpret_cast<int*>(lmask + 8);                                   // [kCsRows]: slot of chunk row i
  int* wtot = rows + kCsRows;                                                      // [2][4]
  int* list = wtot + 8;                                                            // [kFfList]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int q = ff_lane_query(groups, nq);       // this lane's query
  const bool qvalid = q >= 0;
  const float* __restrict__ xq = x + (qvalid ? q : 0);
  unsigned long long* qsl = qs + (wave * 32 + l31) * kFtStride;   // this lane's queue
  const int part = blockIdx.y, n_parts = gridDim.y;
  const int kr = (k - 1) >> 6, kl = (k - 1) & 63;

  const float q2 = sims_query_sq_norm(xq, d, nq);
  int cnt = 0, written = 0;
  float tv = -INFINITY;   // the threshold key: its value and its address
  int ts = kPadIdx;

  // folds the queues of the wave's queries in `mask` (bit j: the query of lane j); wave-uniform.  flat_tile_kernel's.
  auto fold = [&](unsigned mask) {
    while (mask != 0u) {
      const int j = __builtin_ctz(mask);
      mask &= mask - 1u;
      const int n = readlane_i(cnt, j);
      const int had = readlane_i(written, j);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      Key b = pad_key();
      if (lane < n) b = key_of_u64(qs[(wave * 32 + j) * kFtStride + lane]);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      unsigned long long* __restrict__ out = lists + ((int64_t)readlane_i(q, j) * n_parts + part) * (64 * R);
      WaveTopK<R> top;
      if (had) {
#pragma unroll
        for (int r = 0; r < R; ++r) top.k[r] = key_of_u64(out[r * 64 + lane]);
      } else {
        top.init();
      }
      top.insert_unsorted(b);
#pragma unroll
      for (int r = 0; r < R; ++r) out[r * 64 + lane] = key_u64(top.k[r]);
      Key th = pad_key();
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (r == kr) th = readlane_key(top.k[r], kl);
      if (l31 == j) {
        cnt = 0;
        written = 1;
        tv = key_value(th);
        ts = key_index(th);
      }
    }
  };

  ff_gather_walk(ff_group_bits(groups), n_slots, n_chunks, chunks_per_part, list, wtot, [&](int row) {
    f32x16 acc[8];
    sims_rows_mfma(xq, qvalid, Y, row, d, nq, n_slots, cs, c2s, acc,
                   [&](bool cv) { ff_stage_rows(cv, row, address2id, rows, lmask); });
    // epilogue: acc[t][r] = (slot rows[32 t + sims_tile_row(r, half)], query column l31); flat_tile_kernel's, one tile
    // per trip of a rolled loop (see there for the two empty asm statements)
    auto push_tile = [&](const f32x16& a, int t) {
      asm volatile("" : "+s"(t));
      const unsigned lm = qvalid ? lmask[t] : 0u;
      const int* trow = rows + t * 32;
      unsigned pm = 0;
      float vv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cl = sims_tile_row(r, half);
        float dot = a[r];
        asm volatile("" : "+v"(dot));
        float v = inner ? dot : neg_sq_l2(dot, q2, c2s[t * 32 + cl]);
        v = v + 0.0f;  // -0.0 -> +0.0 (key order)
        vv[r] = v;
        // live, not NaN (v >= tv fails), and ahead of the threshold key in (value desc, address asc)
        const bool p = (bool)((lm >> cl) & 1u) & (v >= tv) & ((v > tv) | (trow[cl] < ts));
        pm |= p ? (1u << r) : 0u;
      }
      if (__ballot(pm != 0u) == 0ull) return;
      const int n_mine = __popc(pm);
      const int n_other = __shfl_xor(n_mine, 32, 64);
      int at = cnt + (half ? n_other : 0);   // (cnt <= 32 here: at + n_mine <= 64)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if ((pm >> r) & 1u) {
          qsl[at] = key_u64(make_key(vv[r], trow[sims_tile_row(r, half)]));
          ++at;
        }
      }
      cnt += n_mine + n_other;
    };
#pragma nounroll
    for (int t = 0; t < 8; ++t) {
      static_for<0, 8>([&](auto T) {
        if (t == T.value) push_tile(acc[T.value], T.value);
      });
      fold((unsigned)__ballot(cnt > kFtQueue - 32));   // (the low word: one bit per query)
    }
  });
  // what is left in the queues; a list that was never written is written now (pads), so the merge reads n_parts lists
  fold((unsigned)__ballot(qvalid && (cnt > 0 || !written)));
}

// What both range passes share: flat_range_walk of flat_range.hip over the gathered chunks.  Per tile,
// tile(trow, pm, vv): trow the tile's 32 slot numbers (LDS), bit r of pm set where accumulator register r -- slot
// trow[sims_tile_row(r, half)] -- is a hit of this lane's query, vv[r] its value.
template <class Tile>
__device__ __forceinline__ void ff_range_walk(const float* __restrict__ x, const float* __restrict__ Y,
                                              const int64_t* __restrict__ address2id, const FfGroups& groups, int q,
                                              float thr, int d, int nq, int n_slots, int inner, int n_chunks,
                                              int chunks_per_part, Tile&& tile) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* cs = reinterpret_cast<float*>(smem);                       // [2][kCsKC][kCsRows]
  float* c2s = cs + 2 * kCsSlab;                                    // [kCsRows]
  unsigned* lmask = reinterpret_cast<unsigned*>(c2s + kCsRows);     // [8]: live rows of tile t
  int* rows = reinterpret_cast<int*>(lmask + 8);                    // [kCsRows]: slot of chunk row i
  int* wtot = rows + kCsRows;                                       // [2][4]
  int* list = wtot + 8;                                             // [kFfList]
  const int half = (threadIdx.x & 63) >> 5;
  const bool qvalid = q >= 0;
  const float* __restrict__ xq = x + (qvalid ? q : 0);
  const float q2 = sims_query_sq_norm(xq, d, nq);
  ff_gather_walk(ff_group_bits(groups), n_slots, n_chunks, chunks_per_part, list, wtot, [&](int row) {
    // (the strides, formed per chunk: see flat_range_walk)
    int row_stride = n_slots, col_stride = nq;
    asm volatile("" : "+s"(row_stride), "+s"(col_stride));
    f32x16 acc[8];
    sims_rows_mfma(xq, qvalid, Y, row, d, col_stride, row_stride, cs, c2s, acc,
                   [&](bool cv) { ff_stage_rows(cv, row, address2id, rows, lmask); });
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
        pm = (pm << 1) | (unsigned)(v >= thr);   // false for a NaN on either side
      }
      pm &= live16;
      tile(rows + t * 32, pm, vv);
    }
  });
}

// Range, pass 1: counts[q * n_parts + part] = the hits of query q among the part's allowed slots.  Every segment of
// the call is written: a group whose row allows nothing, a part beyond the last chunk, n_slots == 0 write 0.
__global__ __launch_bounds__(256, 2) void flat_filtered_count_kernel(const float* __restrict__ x, const float* __restrict__ Y,
                                                                     const int64_t* __restrict__ address2id, FfGroups groups,
                                                                     const float* __restrict__ threshold,
                                                                     int32_t* __restrict__ counts, int d, int nq, int n_slots,
                                                                     int inner, int n_chunks, int chunks_per_part) {
  const int lane = threadIdx.x & 63;
  const int q = ff_lane_query(groups, nq);
  int cnt = 0;   // of this half-wave's 16 rows of every tile
  ff_range_walk(x, Y, address2id, groups, q, q >= 0 ? threshold[q] : 0.f, d, nq, n_slots, inner, n_chunks,
                chunks_per_part, [&](const int*, unsigned pm, const float (&)[16]) { cnt += __popc(pm); });
  cnt += __shfl_xor(cnt, 32, 64);
  if (q >= 0 && lane < 32) counts[(int64_t)q * gridDim.y + blockIdx.y] = cnt;
}

// Range, pass 2: the hits of segment q * n_parts + part go to offsets[seg] onwards.  The gathered addresses ascend, so
// the placement of flat_range_fill_kernel (see there: a tile's rows alternate between the half-waves in groups of four)
// keeps address order.  Nothing is stored at or beyond offsets[seg + 1].
__global__ __launch_bounds__(256, 2) void flat_filtered_fill_kernel(const float* __restrict__ x, const float* __restrict__ Y,
                                                                    const int64_t* __restrict__ address2id, FfGroups groups,
                                                                    const float* __restrict__ threshold,
                                                                    const int64_t* __restrict__ offsets,
                                                                    float* __restrict__ out_vals, int64_t* __restrict__ out_addr,
                                                                    int64_t* __restrict__ out_ids, int d, int nq, int n_slots,
                                                                    int inner, int n_chunks, int chunks_per_part) {
  const int half = (threadIdx.x & 63) >> 5;
  const int q = ff_lane_query(groups, nq);
  int64_t o = 0, end = 0;   // the cursor (the same in both half-waves) and the segment's end
  if (q >= 0) {
    const int64_t seg = (int64_t)q * gridDim.y + blockIdx.y;
    o = offsets[seg];
    end = offsets[seg + 1];
  }
  if (!__syncthreads_or(end > o)) return;   // none of the group's segments holds a hit
  ff_range_walk(x, Y, address2id, groups, q, q >= 0 ? threshold[q] : 0.f, d, nq, n_slots, inner, n_chunks,
                chunks_per_part, [&](const int* trow, unsigned pm, const float (&vv)[16]) {
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
                          const int s = trow[sims_tile_row(r, half)];
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

// the argument checks the three entry points share (those of tpq_flat_topk, and the filter's); TPQ_OK: go on
static int flat_filtered_check(const char* what, bool pointers, const int64_t* address2id, const int64_t* out_ids,
                               int64_t filter_stride_words, int n_filters, int n_groups, int64_t n_slots, int d, int nq,
                               int metric, int n_parts) {
  TPQ_REQUIRE(pointers, "%s: null pointer argument", what);
  TPQ_REQUIRE(address2id || !out_ids, "%s: out_ids needs address2id", what);
  TPQ_REQUIRE(d >= 1 && nq >= 0 && n_slots >= 0, "%s: bad shape d=%d nq=%d n_slots=%lld", what, d, nq,
              (long long)n_slots);
  TPQ_REQUIRE(n_parts >= 1 && n_parts <= 1024, "%s: n_parts=%d out of range (1 ... 1024)", what, n_parts);
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "%s: bad metric %d", what, metric);
  TPQ_REQUIRE(n_filters >= 1, "%s: n_filters=%d: at least one row", what, n_filters);
  TPQ_REQUIRE(filter_stride_words >= (n_slots + 31) / 32, "%s: filter stride %lld words is below ceil(n_slots / 32) = %lld",
              what, (long long)filter_stride_words, (long long)((n_slots + 31) / 32));
  TPQ_REQUIRE(nq == 0 || (n_groups >= (nq + 127) / 128 && n_groups <= nq),
              "%s: n_groups=%d outside [ceil(nq / 128), nq] for nq=%d", what, n_groups, nq);
  if (n_slots >= 2147483647LL) {
    set_error("%s: n_slots=%lld: addresses are 31-bit (n_slots < 2^31 - 1)", what, (long long)n_slots);
    return TPQ_ERR_UNSUPPORTED;
  }
  return TPQ_OK;
}

}  // namespace tpq

using namespace tpq;

extern "C" int tpq_flat_topk_filtered(const float* vectors, const float* query, const int64_t* address2id,
                                      const uint32_t* filter_bits, int64_t filter_stride_words, int n_filters,
                                      const int32_t* query_order, const int32_t* group_begin, const int32_t* group_row,
                                      int n_groups, float* out_vals, int64_t* out_addr, int64_t* out_ids, int64_t n_slots,
                                      int d, int nq, int k, int metric, int n_parts, void* workspace,
                                      size_t workspace_bytes, tpq_stream_t stream) {
  const int rc = flat_filtered_check("flat_topk_filtered", vectors && query && filter_bits && query_order && group_begin &&
                                     group_row && out_vals && out_addr, address2id, out_ids, filter_stride_words,
                                     n_filters, n_groups, n_slots, d, nq, metric, n_parts);
  if (rc) return rc;
  TPQ_REQUIRE(k >= 1 && k <= 1024, "flat_topk_filtered: k=%d out of range (1 ... 1024)", k);
  if (nq == 0) return TPQ_OK;
  const size_t need = tpq_flat_topk_workspace_bytes(nq, k, n_parts);
  if (!workspace || workspace_bytes < need) {
    set_error("flat_topk_filtered: workspace too small (%zu < %zu)", workspace_bytes, need);
    return TPQ_ERR_WORKSPACE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(workspace);
  const FfGroups groups{query_order, group_begin, group_row, filter_bits, filter_stride_words, n_filters};
  const int n_chunks = (int)((n_slots + kCsRows - 1) / kCsRows);
  return with_list_regs(list_regs(k), [&](auto r_c) -> int {
    constexpr int R = decltype(r_c)::value;
    if (n_slots > 0) {
      const int rc = launch_with_lds(flat_filtered_tile_kernel<R>, "flat_filtered_tile_kernel", dim3(n_groups, n_parts),
                                     dim3(256), kFfTopkLds, st, query, vectors, address2id, groups, lists, d, nq,
                                     (int)n_slots, k, (int)(metric == TPQ_METRIC_INNER), n_chunks,
                                     (n_chunks + n_parts - 1) / n_parts);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(flat_merge_kernel<R>, dim3((nq + 3) / 4), dim3(256), 0, st, lists, address2id, out_vals, out_addr,
                       out_ids, nq, k, n_slots > 0 ? n_parts : 0);
    TPQ_LAUNCH_CHECK("flat_merge_kernel");
    return TPQ_OK;
  });
}

extern "C" int tpq_flat_range_filtered_count(const float* vectors, const float* query, const int64_t* address2id,
                                             const uint32_t* filter_bits, int64_t filter_stride_words, int n_filters,
                                             const int32_t* query_order, const int32_t* group_begin,
                                             const int32_t* group_row, int n_groups, const float* threshold,
                                             int32_t* counts, int64_t n_slots, int d, int nq, int metric, int n_parts,
                                             tpq_stream_t stream) {
  const int rc = flat_filtered_check("flat_range_filtered_count", vectors && query && filter_bits && query_order &&
                                     group_begin && group_row && threshold && counts, address2id, nullptr,
                                     filter_stride_words, n_filters, n_groups, n_slots, d, nq, metric, n_parts);
  if (rc) return rc;
  if (nq == 0) return TPQ_OK;
  const FfGroups groups{query_order, group_begin, group_row, filter_bits, filter_stride_words, n_filters};
  const int n_chunks = (int)((n_slots + kCsRows - 1) / kCsRows);
  return launch_with_lds(flat_filtered_count_kernel, "flat_filtered_count_kernel", dim3(n_groups, n_parts), dim3(256),
                         kFfRangeLds, reinterpret_cast<hipStream_t>(stream), query, vectors, address2id, groups, threshold,
                         counts, d, nq, (int)n_slots, (int)(metric == TPQ_METRIC_INNER), n_chunks,
                         (n_chunks + n_parts - 1) / n_parts);
}

extern "C" int tpq_flat_range_filtered_fill(const float* vectors, const float* query, const int64_t* address2id,
                                            const uint32_t* filter_bits, int64_t filter_stride_words, int n_filters,
                                            const int32_t* query_order, const int32_t* group_begin,
                                            const int32_t* group_row, int n_groups, const float* threshold,
                                            const int64_t* offsets, float* out_vals, int64_t* out_addr, int64_t* out_ids,
                                            int64_t n_slots, int d, int nq, int metric, int n_parts, tpq_stream_t stream) {
  const int rc = flat_filtered_check("flat_range_filtered_fill", vectors && query && filter_bits && query_order &&
                                     group_begin && group_row && threshold && offsets && out_vals && out_addr, address2id,
                                     out_ids, filter_stride_words, n_filters, n_groups, n_slots, d, nq, metric, n_parts);
  if (rc) return rc;
  if (nq == 0 || n_slots == 0) return TPQ_OK;   // (no slots: no hits)
  const FfGroups groups{query_order, group_begin, group_row, filter_bits, filter_stride_words, n_filters};
  const int n_chunks = (int)((n_slots + kCsRows - 1) / kCsRows);
  return launch_with_lds(flat_filtered_fill_kernel, "flat_filtered_fill_kernel", dim3(n_groups, n_parts), dim3(256),
                         kFfRangeLds, reinterpret_cast<hipStream_t>(stream), query, vectors, address2id, groups, threshold,
                         offsets, out_vals, out_addr, out_ids, d, nq, (int)n_slots, (int)(metric == TPQ_METRIC_INNER),
                         n_chunks, (n_chunks + n_parts - 1) / n_parts);
}
