// Exact search without its similarity matrix (tpq_flat_topk): the fp32-MFMA similarity tile of coarse_sims_kernel
// (sims_chunk.h) with a selection epilogue in place of the store of the tile, and a merge of the parts' lists.
// Nothing of size nq x n_slots exists: the state is one sorted list of 64 R keys per (query, part) in the caller's
// workspace and one 64-entry queue per query in LDS.  Values and order are defined in include/torchpq_amd.h.
#include "sims_chunk.h"
#include "row_select.h"

namespace tpq {

// Pass 1.  grid (ceil(nq / 128), n_parts); part p walks the 256-slot chunks [p cpp, (p + 1) cpp) below n_chunks (formed
// by the host in 64 bits: n_slots + 255 does not fit an int near 2^31).
// A lane's query is the MFMA column l31 of its wave; its two half-waves hold the 2 x 16 rows of a 32-slot tile, so
// a tile pushes at most 32 keys for one query.  Per query, in registers of both half-waves: the queue's fill, the
// admission threshold (the k-th key of the part's list; the pad key while fewer than k are held) and whether the
// list in the workspace has been written.  A queue that could not take another tile (fill > 32) is folded by the
// whole wave, one query per trip: list (L2-resident) -> registers, bitonic sort of the queue, merge, list back.
// A query belongs to one wave for the block's whole range: no atomics, no barrier beyond the slab pipeline's.
constexpr int kFtQueue = 64;        // keys per query queue
constexpr int kFtStride = 65;       // ... and its stride in LDS: the queues of a wave's lanes start on different banks
constexpr size_t kFtLds = (2 * kCsSlab + kCsRows) * sizeof(float) + 8 * sizeof(unsigned) +
                          (size_t)128 * kFtStride * sizeof(unsigned long long);   // 32 + 1 + 65 KiB: one block per CU

template <int R>
__global__ __launch_bounds__(256, 1) void flat_tile_kernel(const float* __restrict__ x, const float* __restrict__ Y,
                                                           const int64_t* __restrict__ address2id,
                                                           unsigned long long* __restrict__ lists, int d, int nq,
                                                           int n_slots, int k, int inner, int n_chunks,
                                                           int chunks_per_part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* qs = reinterpret_cast<unsigned long long*>(smem);            // [128][kFtStride]
  float* cs = reinterpret_cast<float*>(qs + 128 * kFtStride);                       // [2][kCsKC][kCsRows]
  float* c2s = cs + 2 * kCsSlab;                                                   // [kCsRows]
  unsigned* lmask = reinterpret_cast<unsigned*>(c2s + kCsRows);                    // [8]: live slots of tile t
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int qw = blockIdx.x * 128 + wave * 32;   // first query of this wave
  const int q = qw + l31;                        // this lane's query
  const bool qvalid = q < nq;
  const float* __restrict__ xq = x + (qvalid ? q : 0);
  unsigned long long* qsl = qs + (wave * 32 + l31) * kFtStride;   // this lane's queue
  const int part = blockIdx.y, n_parts = gridDim.y;
  const int kr = (k - 1) >> 6, kl = (k - 1) & 63;

  const float q2 = sims_query_sq_norm(xq, d, nq);
  int cnt = 0, written = 0;
  float tv = -INFINITY;   // the threshold key: its value and its address
  int ts = kPadIdx;

  // folds the queues of the wave's queries in `mask` (bit j: query qw + j); wave-uniform
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
      unsigned long long* __restrict__ list = lists + ((int64_t)(qw + j) * n_parts + part) * (64 * R);
      WaveTopK<R> top;
      if (had) {
#pragma unroll
        for (int r = 0; r < R; ++r) top.k[r] = key_of_u64(list[r * 64 + lane]);
      } else {
        top.init();
      }
      top.insert_unsorted(b);
#pragma unroll
      for (int r = 0; r < R; ++r) list[r * 64 + lane] = key_u64(top.k[r]);
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

  const int chunk0 = part * chunks_per_part;
  const int chunk1 = chunk0 + chunks_per_part < n_chunks ? chunk0 + chunks_per_part : n_chunks;
  for (int ch = chunk0; ch < chunk1; ++ch) {
    const int c0 = ch * kCsRows;
    f32x16 acc[8];
    sims_chunk_mfma(xq, qvalid, Y, c0, d, nq, n_slots, cs, c2s, acc, [&](bool cv) {
      // the chunk's live mask: thread i stages slot c0 + i, a wave's ballot is tiles 2 wave and 2 wave + 1
      bool live = cv;
      if (cv && address2id) live = address2id[c0 + (int)threadIdx.x] >= 0;
      const unsigned long long m = __ballot(live);
      if (lane == 0) {
        lmask[2 * wave] = (unsigned)m;
        lmask[2 * wave + 1] = (unsigned)(m >> 32);
      }
    });
    // epilogue: acc[t][r] = (slot c0 + 32 t + sims_tile_row(r, half), query column l31).  One tile per trip of a
    // rolled loop whose body branches (wave-uniformly) to the tile's registers, so that the fold is instantiated once.
    auto push_tile = [&](const f32x16& a, int t) {
      // (neither the tile's slot numbers nor its values depend on the trip of the rolled loop below: left alone, the
      // compiler forms all 8 x 16 of them, and their keys, ahead of the loop and spills -- seen with the clang 22 of
      // ROCm 7.2; build() fails if this kernel spills a register, so a compiler that sees through the two empty asm
      // statements here is noticed)
      asm volatile("" : "+s"(t));
      const unsigned lm = qvalid ? lmask[t] : 0u;
      const int s0 = c0 + t * 32;
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
        const bool p = (bool)((lm >> cl) & 1u) & (v >= tv) & ((v > tv) | (s0 + cl < ts));
        pm |= p ? (1u << r) : 0u;
      }
      if (__ballot(pm != 0u) == 0ull) return;
      const int n_mine = __popc(pm);
      const int n_other = __shfl_xor(n_mine, 32, 64);
      int at = cnt + (half ? n_other : 0);   // (cnt <= 32 here: at + n_mine <= 64)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if ((pm >> r) & 1u) {
          qsl[at] = key_u64(make_key(vv[r], s0 + sims_tile_row(r, half)));
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
  }
  // what is left in the queues; a list that was never written is written now (pads), so the merge reads n_parts lists
  fold((unsigned)__ballot(qvalid && (cnt > 0 || !written)));
}

// Pass 2: one wave per query folds its n_parts lists and writes the row -- values, addresses, ids, pads.
// n_parts == 0 (no slots): all pads.
template <int R>
__global__ __launch_bounds__(256) void flat_merge_kernel(const unsigned long long* __restrict__ lists,
                                                         const int64_t* __restrict__ address2id,
                                                         float* __restrict__ out_vals, int64_t* __restrict__ out_addr,
                                                         int64_t* __restrict__ out_ids, int nq, int k, int n_parts) {
  const int lane = lane_id();
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  WaveTopK<R> top;
  top.init();
  for (int p = 0; p < n_parts; ++p) {
    const unsigned long long* __restrict__ list = lists + ((int64_t)q * n_parts + p) * (64 * R);
    Key b[R];
#pragma unroll
    for (int r = 0; r < R; ++r) b[r] = key_of_u64(list[r * 64 + lane]);
    bool more = true;   // (a list is sorted: once a register's best is a pad, or cannot enter, neither can the rest)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      more = more && key_better(readlane_key(b[r], 0), readlane_key(top.k[R - 1], 63));
      if (more) top.insert_sorted(b[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = r * 64 + lane;
    if (e < k) {
      const int s = key_index(top.k[r]);
      const bool pad = s == kPadIdx;
      out_vals[(int64_t)q * k + e] = pad ? -INFINITY : key_value(top.k[r]);
      out_addr[(int64_t)q * k + e] = pad ? -1 : (int64_t)s;
      if (out_ids) out_ids[(int64_t)q * k + e] = pad ? -1 : address2id[s];
    }
  }
}

}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_flat_topk_workspace_bytes(int nq, int k, int n_parts) {
  if (nq <= 0 || k < 1 || k > 1024 || n_parts < 1 || n_parts > 1024) return 0;
  return (size_t)nq * (size_t)n_parts * (size_t)(64 * list_regs(k)) * sizeof(unsigned long long);
}

extern "C" int tpq_flat_topk(const float* vectors, const float* query, const int64_t* address2id, float* out_vals,
                             int64_t* out_addr, int64_t* out_ids, int64_t n_slots, int d, int nq, int k, int metric,
                             int n_parts, void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(vectors && query && out_vals && out_addr, "flat_topk: null pointer argument");
  TPQ_REQUIRE(address2id || !out_ids, "flat_topk: out_ids needs address2id");
  TPQ_REQUIRE(d >= 1 && nq >= 0 && n_slots >= 0, "flat_topk: bad shape d=%d nq=%d n_slots=%lld", d, nq,
              (long long)n_slots);
  TPQ_REQUIRE(k >= 1 && k <= 1024, "flat_topk: k=%d out of range (1 ... 1024)", k);
  TPQ_REQUIRE(n_parts >= 1 && n_parts <= 1024, "flat_topk: n_parts=%d out of range (1 ... 1024)", n_parts);
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "flat_topk: bad metric %d", metric);
  if (n_slots >= 2147483647LL) {
    set_error("flat_topk: n_slots=%lld: addresses are 31-bit (n_slots < 2^31 - 1)", (long long)n_slots);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (nq == 0) return TPQ_OK;
  const size_t need = tpq_flat_topk_workspace_bytes(nq, k, n_parts);
  if (!workspace || workspace_bytes < need) {
    set_error("flat_topk: workspace too small (%zu < %zu)", workspace_bytes, need);
    return TPQ_ERR_WORKSPACE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(workspace);
  const int n_chunks = (int)((n_slots + kCsRows - 1) / kCsRows);
  return with_list_regs(list_regs(k), [&](auto r_c) -> int {
    constexpr int R = decltype(r_c)::value;
    if (n_slots > 0) {
      const int rc = launch_with_lds(flat_tile_kernel<R>, "flat_tile_kernel", dim3((nq + 127) / 128, n_parts), dim3(256),
                                     kFtLds, st, query, vectors, address2id, lists, d, nq, (int)n_slots, k,
                                     (int)(metric == TPQ_METRIC_INNER), n_chunks, (n_chunks + n_parts - 1) / n_parts);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(flat_merge_kernel<R>, dim3((nq + 3) / 4), dim3(256), 0, st, lists, address2id, out_vals, out_addr,
                       out_ids, nq, k, n_slots > 0 ? n_parts : 0);
    TPQ_LAUNCH_CHECK("flat_merge_kernel");
    return TPQ_OK;
  });
}
