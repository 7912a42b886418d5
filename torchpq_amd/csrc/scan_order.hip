// IVF list scan: the dispatch order of a large batch -- the queries by the tiles they scan, longest first.
//
// The large-batch routes (scan_packed_kernel's dump modes, scan.hip) run one workgroup per query and the hardware
// starts workgroups in blockIdx order.  In query order the work of consecutive workgroups is random: the last ones to
// start are as likely long as short, and a long one that starts last runs alone while the chip's other slots idle.
// Started longest first, the batch ends on its shortest queries.
//
// Two launches on the caller's stream, no host read, no allocation (a captured graph replays them):
//   scan_work_kernel        work[q] = sum over the probes of ceil(size / 2^tile_shift), one wave per query, with the
//                           clamps of the scan's own probe table (fetch_probes / build_probe_table, scan_shared.h);
//   scan_order_rank_kernel  rank[q] = number of queries that go before q -- more work, or the same work and a smaller
//                           index -- counted pair by pair: 64 queries per workgroup, one per lane, against the work of
//                           every other query, read wave-uniformly (scalar loads), sixteen waves sharing the batch.
//                           Exact (a strict total order: rank is a permutation, equal work keeps query order), any nq;
//                           nq^2 pairs of one compare and one add each, which is why scan.hip orders batches of up to
//                           kOrderMaxQueries only.
#include "common.h"
#include "scan_order.h"

namespace tpq {

constexpr int kOrderWaves = 16;  // waves of a rank workgroup: each takes a sixteenth of the batch

__global__ __launch_bounds__(256) void scan_work_kernel(const int64_t* __restrict__ cell_start,
                                                        const int64_t* __restrict__ cell_size,
                                                        const int64_t* __restrict__ n_probe_list,
                                                        int* __restrict__ work, int nq, int max_nprobe,
                                                        int tile_shift, int probe_cap) {
  const int lane = (int)(threadIdx.x & 63);
  const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (q >= nq) return;  // (wave-uniform)
  int n_probe = (int)n_probe_list[q];
  n_probe = n_probe < 0 ? 0 : (n_probe > max_nprobe ? max_nprobe : n_probe);
  if (probe_cap > 0 && n_probe > probe_cap) n_probe = probe_cap;  // (the scan's own cap: clamped_n_probe)
  const int64_t* __restrict__ cs = cell_start + (int64_t)q * max_nprobe;
  const int64_t* __restrict__ cz = cell_size + (int64_t)q * max_nprobe;
  unsigned long long tiles = 0ull;
  for (int p = lane; p < n_probe; p += 64) {
    const int st = (int)cs[p];
    int sz = (int)cz[p];
    if (p > 0 && cs[p - 1] == (int64_t)st) sz = 0;  // a cell listed twice in a row is scanned once
    if (sz < 0) sz = 0;
    tiles += (unsigned long long)(((int64_t)sz + ((int64_t)1 << tile_shift) - 1) >> tile_shift);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) tiles += __shfl_xor(tiles, d, 64);
  if (lane == 0) work[q] = tiles > 0x7fffffffull ? 0x7fffffff : (int)tiles;
}

__global__ __launch_bounds__(kOrderWaves * 64) void scan_order_rank_kernel(const int* __restrict__ work,
                                                                           int* __restrict__ order,
                                                                           int* __restrict__ rank, int nq) {
  __shared__ int cnt_s[kOrderWaves][64];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lo = (int)blockIdx.x * 64, hi = lo + 64;  // this workgroup's queries
  const int q = lo + lane;
  const int wq = q < nq ? work[q] : 0x7fffffff;
  // the wave's share [a, b) of the batch, in three runs by where the other query q' = i lies: below every query of this
  // workgroup (q' goes first on equal work), among them (lane by lane), above them (q goes first).  The index is
  // wave-uniform: the other query's work arrives through the scalar cache and is compared from an SGPR.
  const int per = (nq + kOrderWaves - 1) / kOrderWaves;
  const int a = wave * per < nq ? wave * per : nq, b = a + per < nq ? a + per : nq;
  const int m1 = lo < a ? a : (lo > b ? b : lo);
  const int m2 = hi < a ? a : (hi > b ? b : hi);
  int cnt = 0;
#pragma unroll 16
  for (int i = a; i < m1; ++i) cnt += work[i] >= wq ? 1 : 0;
  for (int i = m1; i < m2; ++i) {
    const int wp = work[i];
    cnt += (wp > wq || (wp == wq && i < q)) ? 1 : 0;
  }
#pragma unroll 16
  for (int i = m2; i < b; ++i) cnt += work[i] > wq ? 1 : 0;
  cnt_s[wave][lane] = cnt;
  __syncthreads();
  if (wave == 0 && q < nq) {
    int r = 0;
#pragma unroll
    for (int w = 0; w < kOrderWaves; ++w) r += cnt_s[w][lane];
    rank[q] = r;   // (r < nq: at most the nq - 1 other queries go before q)
    order[r] = q;
  }
}

int launch_scan_order(const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list, int nq,
                      int max_nprobe, int tile_shift, int* order, int* rank, int* work, hipStream_t st,
                      int probe_cap) {
  if (nq <= 0) return TPQ_OK;
  hipLaunchKernelGGL(scan_work_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, cell_start, cell_size,
                     n_probe_list, work, nq, max_nprobe, tile_shift, probe_cap);
  TPQ_LAUNCH_CHECK("scan_work_kernel");
  hipLaunchKernelGGL(scan_order_rank_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(kOrderWaves * 64), 0, st, work,
                     order, rank, nq);
  TPQ_LAUNCH_CHECK("scan_order_rank_kernel");
  return TPQ_OK;
}

}  // namespace tpq

extern "C" int tpq_ivfpq_scan_order(const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                    int nq, int max_nprobe, int tile_shift, int32_t* order, int32_t* rank,
                                    int32_t* work, tpq_stream_t stream) {
  TPQ_REQUIRE(cell_start && cell_size && n_probe_list && order && rank && work,
              "ivfpq_scan_order: null pointer argument");
  TPQ_REQUIRE(nq >= 0 && max_nprobe >= 1, "ivfpq_scan_order: bad nq/max_nprobe (%d, %d)", nq, max_nprobe);
  TPQ_REQUIRE(tile_shift >= 0 && tile_shift <= 16, "ivfpq_scan_order: tile_shift=%d out of range [0, 16]", tile_shift);
  return tpq::launch_scan_order(cell_start, cell_size, n_probe_list, nq, max_nprobe, tile_shift, order, rank, work,
                                reinterpret_cast<hipStream_t>(stream), 0);
}
