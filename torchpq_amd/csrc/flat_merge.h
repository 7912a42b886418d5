// What the exact top-k kernels share (flat_tile_kernel of flat_topk.hip, flat_filtered_tile_kernel of flat_filtered.hip):
// the size of a query's queue in LDS, and the merge of the parts' lists into the output rows.
#pragma once
#include "sims_chunk.h"
#include "row_select.h"

namespace tpq {

constexpr int kFtQueue = 64;        // keys per query queue
constexpr int kFtStride = 65;       // ... and its stride in LDS: the queues of a wave's lanes start on different banks
constexpr size_t kFtLds = (2 * kCsSlab + kCsRows) * sizeof(float) + 8 * sizeof(unsigned) +
                          (size_t)128 * kFtStride * sizeof(unsigned long long);   // 32 + 1 + 65 KiB: one block per CU

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
