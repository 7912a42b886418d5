// IVF list scan: the kernels that finish what scan_packed_kernel leaves (lists, dumps, pools).
#pragma once
#include "scan_shared.h"
#include "scan_exact.h"
#include "scan_fk.h"
#include "scan_packed_kernel.h"

namespace tpq {

// phase 2, wave-level: the merged list already carries EXACT values; write the best k and raise
// the overflow flag when the list is so full of near-ties that a member of the exact top-k may
// have been evicted from a wave's list (see the header comment of this section)
template <int R, bool RES = false>
__device__ __forceinline__ void finalize_and_write(const ScanArgs& a, int q, const WaveTopK<R>& top,
                                                   float delta2) {
  const float ek = top.kth_value(a.k);
  const Key klast = readlane_key(top.k[R - 1], 63);
  const bool overflow = (key_index(klast) != kPadIdx) && !(key_value(klast) < ek - delta2);
  write_final<R>(a, q, top);
  if (RES || a.small_lists) {  // the scan kernel may already have raised this one
    if (lane_id() == 0 && overflow) a.flags[q] = a.epoch;
  } else {
    if (lane_id() == 0) a.flags[q] = overflow ? a.epoch : 0;
  }
}

// packed path, phase 2: merge the per-wave lists of a query (exact values) and write the result.
// W = blockDim.x / 64 waves per query (host: min(8, n_lists / 2)): wave w folds lists w, w+W, ...
// rank-major (every list's best 64 first: once those are in, most later chunks fail the
// wave-uniform early-exit test of insert_sorted) with the loads issued a group ahead of the
// merges, then the W partial lists are tree-merged through LDS.  Small batches run with many
// splits per query (512 lists at nq = 1): one wave folding them serially took 0.2 ms.
// RL = registers per dumped list (64 RL entries each), R = registers of the merged result.
template <int RL, int R, int M, bool RES>
__global__ __launch_bounds__(512) void scan_merge_refine_kernel(ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int q = blockIdx.x;
  const int lane = lane_id();
  const int W = (int)(blockDim.x >> 6), wave = (int)(threadIdx.x >> 6);
  const int n_lists = a.n_split * packed_waves(M);  // a multiple of 8
  const int n_mine = n_lists / W;
  WaveTopK<R> top;
  top.init();
  const unsigned* __restrict__ bv =
      reinterpret_cast<const unsigned*>(a.ws_vals) + (int64_t)q * n_lists * (RL * 64);
  const unsigned* __restrict__ bi =
      reinterpret_cast<const unsigned*>(a.ws_idx) + (int64_t)q * n_lists * (RL * 64);
  const int T = n_mine * RL;  // item t: rank chunk t / n_mine of my (t % n_mine)-th list
  auto load_item = [&](int t) -> Key {
    if (t >= T) return pad_key();
    const int r = t / n_mine, l = (t - r * n_mine) * W + wave;
    const int64_t o = (int64_t)l * (RL * 64) + r * 64 + lane;
    return Key{bv[o], bi[o]};
  };
  constexpr int G = 4;
  Key k0[G], k1[G];
#pragma unroll
  for (int u = 0; u < G; ++u) k0[u] = load_item(u);
  for (int t = 0; t < T; t += 2 * G) {
#pragma unroll
    for (int u = 0; u < G; ++u) k1[u] = load_item(t + G + u);
#pragma unroll
    for (int u = 0; u < G; ++u) top.insert_sorted(k0[u]);
#pragma unroll
    for (int u = 0; u < G; ++u) k0[u] = load_item(t + 2 * G + u);
#pragma unroll
    for (int u = 0; u < G; ++u) top.insert_sorted(k1[u]);
  }
  float* lv = reinterpret_cast<float*>(smem);
  int* li = reinterpret_cast<int*>(smem + (size_t)W * R * 64 * 4);
  for (int stride = 1; stride < W; stride <<= 1) {
    if ((wave & (2 * stride - 1)) == stride) store_list<R>(top, lv + wave * R * 64, li + wave * R * 64);
    __syncthreads();
    if ((wave & (2 * stride - 1)) == 0)
      merge_list<R>(top, lv + (wave + stride) * R * 64, li + (wave + stride) * R * 64);
    __syncthreads();
  }
  if (wave == 0) finalize_and_write<R, RES>(a, q, top, a.ws_delta[q]);
}

// dump modes, phase 2: ONE WAVE per query.  The query's lists of FAST values arrive as NCH chunks of 64 keys (n_split x
// nw_scan lists of RL chunks, best first).  With F_k the k-th best fast value over all of them and `band` the scan's
// 2 delta, every member of the exact top-k has F >= F_k - band.  F_k comes from a bit-wise binary search on the key
// images (a ballot and a scalar popcount per chunk and step: the chunks never leave their registers, and most of the
// work rides on the scalar unit); nothing at or above the cut may have been lost on the way -- a wave's list that evicted
// (list_evict) and still ends at or above the cut, or more survivors than 64 RM, flags the query for the exact kernel.
// The survivors are compacted through a small LDS queue, 64 per pass, and evaluated EXACTLY, one per lane: the
// candidate's 64 packed bytes are brought into sub-quantizer order IN REGISTERS (a byte permute per dword for the low
// two bits of its XOR mask, four rounds of conditional dword swaps for the others), then sub-quantizer by sub-quantizer,
// the same j in every lane: entry = tpq_adc_lut's arithmetic on the codebook row (in LDS) and the query component
// (v_readlane from a register: wave-uniform), added in ascending j -- the reference's order, hence its bits.  Sorted by
// (value desc, address asc) and written.
// The codebook lives in LDS: one persistent workgroup per CU copies it (m * ds KiB, query-independent) once and its
// waves walk the queries.  (Entries fetched from global memory -- a different cache line per lane and look-up -- ran into
// the address coalescer: 396 us per 10 000 queries at k = 100; from LDS with lane-varying sub-quantizers and a value
// butterfly: 160 us, instruction-bound at ~6 000 VALU per query; this form: ~2 500.)  Nothing of a scan workgroup's
// table slot is held while this runs, which is the point of the split: the end of a query idled that slot for 17 of
// its 43 us.
// (waves per workgroup: 16 at every RM the kernel is built for -- RM = 8, k in (248, 504], ds = 2: 128 KiB of codebook + 32
// KiB of survivor queues, all of the CU's LDS; a longer exact list would halve them)
//
// Round 6: every packed block structure (the 64-block of m = 64 and the 32 / 16 / 8 / 4-blocks of the shorter codes:
// the un-permute below walks scan_layout's blocks), any sub-vector length with m * ds <= 128 (DS = 0: read from the
// arguments), and a second SOURCE of the exact entries -- FROM_LUT: the caller's materialised table [m][nq][256]
// (tpq_adc_lut's output, the reference boundary: IVFPQTopkCuda.topk(precomputed=...), kernels/IVFPQTopkCuda.py:81-142),
// gathered per survivor (m independent loads per lane, ascending-j adds); nothing is staged in LDS then.
//
// The deal.  Workgroup b of G takes the CONTIGUOUS queries [b nq / G, (b + 1) nq / G): every workgroup's share is within
// one query of nq / G (queries strided over the grid's waves left the first nq mod 16 G waves a whole query more than the
// others: at 10 000 queries on 256 CUs, 48 queries on each of 113 CUs against 32 on the rest), and the 16 queries a
// workgroup holds at one time share the cache lines of query[d][nq].  Its waves draw the queries of that range from a
// counter in LDS, one atomic per query (kFinishDraw), so that a wave with a long query does not hold back its SIMD's
// share; where the codebook and the queues leave the CU no LDS for the counter -- RM = 8 beside a codebook -- wave w takes
// every kFinishWaves-th query of the range (10 000 queries at k = 300: 352 -> 322 us).  RM = 16 beside a codebook keeps
// the strided deal: its eight waves per workgroup take 4 or 5 queries each either way, so the ranges have nothing to
// give there.  (That instantiation runs 2 % slower than it did, under either deal -- 10 000 queries at k = 500: 757 ->
// 774 us strided, 774 -> 792 with the ranges on another machine; 83 -> 97 registers around sixteen-register exact rounds.
// The cause was not found.)
//
// The cell-major form's stage 5 (scan.hip) hands over two more numbers; both are 0 / null everywhere else.
//  * seed_chunks: the query's first seed_chunks chunks hold the exact top-k of its first probes, written by THIS kernel
//    in the form's stage 1 and copied there as make_key(value, address) (cell_seed_kernel).  Their survivors are not
//    queued and not evaluated again: they are inserted as Key{hi, ~address} straight from the registers.  The bits are
//    those the evaluation would return: stage 1 ran the same chain of this same kernel over the same codebook and query
//    (the codes, the un-permute, the ascending-j adds), `v + 0.0f` was applied before that value was written, key2f(f2key(v))
//    == v for every such v, and the exact list orders by (value desc, address asc) whatever the order of the inserts -- a
//    strict total order.  n_c, and with it the `lost` rule, counts seeds and candidates together as before: the same
//    queries are flagged.
//  * cnt[q]: the entries appended behind the seed chunks (the candidate kernel's counter; a count beyond the capacity
//    flags the query, which is then skipped here).  Only T_q = seed_chunks + ceil(min(cnt, capacity) / 64) chunks hold
//    anything; the loads, the ballots of the F_k search and the survivor walk stop there (finish_fk_upto: the search,
//    unrolled for 2, 4, 6, 8, 12 or 16 chunks -- steps of two up to the 8 chunks 99 % of the headline's queries stay
//    within, mean 4.6; a chunk of a step is a compare, a popcount and an add, and ONE 32-step loop whose chunk walk breaks
//    at T_q puts a scalar compare and a branch beside each: that form measured 101 us against 92).  The tail of the last chunk is pad: the seed kernel writes ~kPadIdx into
//    every idx chunk, and `hi` is zeroed under a pad index below.
// (Measured on the headline batch -- 10 000 queries, k = 100, stage 1 at 4 chunks / stage 5 at 16 --, us per launch,
// profiles/finish_deal_bench.json: strided deal 114.3 / 146.8; ranges 108.7 / 138.5, the same with and without the
// counter; seeds kept 119.6 and filled chunks only 114.0 on stage 5, both 92 -- and 103 with the ranges dealt statically:
// a query then costs one or two exact rounds over 3 to 13 chunks, and the counter evens that out.  48 % of a query's 105
// survivors are seeds; 23 % of the queries keep more than 64 among their candidates and run a second round.)
constexpr int finish_waves(int RM) { return RM <= 8 ? 16 : 8; }
// registers of the finish kernel's exact list.  Round 6: 16 (eight waves per workgroup: 128 KiB of codebook + 32 KiB of
// survivor queues) -- k in (440, 504] on long cells, whose band holds more than the 512 candidates of RM = 8
constexpr int kDumpMaxR = 16;
// the waves draw their queries from a counter in LDS (16 bytes behind the queues)
constexpr bool finish_draws(int RM, bool from_lut) { return from_lut || RM < 8; }
static size_t finish_lds_bytes(int m, int ds, int RM, bool from_lut) {
  return (from_lut ? 0 : (size_t)m * ds * 1024) + (size_t)finish_waves(RM) * RM * 64 * 4 +
         (finish_draws(RM, from_lut) ? 16 : 0);
}
// (F_k -- finish_fk, finish_fk_upto: scan_fk.h, shared with the cell-major form's cell_kth_kernel)
template <int RM, int M, int DS, int NCH, bool FROM_LUT = false>
__global__ __launch_bounds__(finish_waves(RM) * 64) void scan_finish_exact_kernel(ScanArgs a, int nw_scan, int RL,
                                                                                   int seed_chunks,
                                                                                   const int* __restrict__ cnt) {
  constexpr int kFinishWaves = finish_waves(RM);
  constexpr bool kFinishDraw = finish_draws(RM, FROM_LUT);
  constexpr bool kFinishRanges = kFinishDraw || RM <= 8;
  constexpr int kSeedMax = RM < NCH ? RM : NCH;  // (seeds are a top-k: k <= 64 RM)
  using L = scan_layout::Layout<M>;
  constexpr int G = M / 4;  // code dwords per slot
  static_assert(DS == 0 || M * DS <= 128, "the query rides in two registers per lane");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
  const int ds = DS ? DS : a.ds;  // (the host admits m * ds <= 128 only)
  float* cb = reinterpret_cast<float*>(smem);  // [m][ds][256]
  if constexpr (!FROM_LUT) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(a.codebook);
    float4* dst = reinterpret_cast<float4*>(cb);
    for (int i = threadIdx.x; i < M * ds * 64; i += kFinishWaves * 64) dst[i] = src[i];
  }
  int* queues = reinterpret_cast<int*>(cb + (FROM_LUT ? 0 : M * ds * 256));
  int* qi = queues + wave * (RM * 64);           // the wave's survivors (addresses)
  int* next = queues + kFinishWaves * (RM * 64);  // kFinishDraw: queries of the range handed out so far
  if (kFinishDraw && threadIdx.x == 0) *next = 0;
  __syncthreads();
  const int n_lists_all = a.n_split * nw_scan;
  const int T_all = n_lists_all * RL;  // chunks per query in the workspace (<= NCH)
  const bool euclid = a.euclid != 0;
  // (RM = 16: the queries strided over the grid's waves, as before -- see the header)
  const int q_lo = kFinishRanges ? (int)((int64_t)blockIdx.x * a.nq / (int64_t)gridDim.x) : (int)blockIdx.x * kFinishWaves;
  const int q_hi = kFinishRanges ? (int)(((int64_t)blockIdx.x + 1) * a.nq / (int64_t)gridDim.x) : a.nq;
  const int stride = kFinishRanges ? kFinishWaves : (int)gridDim.x * kFinishWaves;
  for (int turn = wave;; turn += stride) {
    int q = q_lo + turn;
    if constexpr (kFinishDraw) {
      int t = 0;
      if (lane == 0) t = atomicAdd(next, 1);
      q = q_lo + __builtin_amdgcn_readfirstlane(t);
    }
    if (q >= q_hi) break;
    if (a.flags[q] == a.epoch) continue;  // the scan left the query to the exact kernel
    // (tail split: an unsplit query filled the lists of its one part only; the stride is that of n_split parts)
    // (dispatch order, ScanArgs::rank: the unsplit queries are the first `unsplit` of the order)
    const int n_lists = (a.rank ? a.rank[q] : q) < a.unsplit ? nw_scan : n_lists_all;
    int T = n_lists * RL;  // chunks in use
    if (cnt) {             // (the cell-major form: one list of T_all chunks, filled from the front)
      const int room = (T_all - seed_chunks) * 64, n = cnt[q];
      T = seed_chunks + ((n < room ? n : room) + 63) / 64;
    }
    // the query: component i in lane i % 64 of register i / 64; |q_j|^2 (ascending-dimension fma chain) in lane j
    float xv[2] = {0.f, 0.f}, q2v = 0.f;
    if constexpr (!FROM_LUT) {
      if (lane < M * ds) xv[0] = a.query[(int64_t)lane * a.nq + q];
      if (64 + lane < M * ds) xv[1] = a.query[(int64_t)(64 + lane) * a.nq + q];
      if (lane < M) {
        for (int e = 0; e < ds; ++e) {
          const float x = a.query[(int64_t)(lane * ds + e) * a.nq + q];
          q2v = fmaf(x, x, q2v);
        }
      }
    }
    const unsigned* __restrict__ bv = reinterpret_cast<const unsigned*>(a.ws_vals) + (int64_t)q * T_all * 64;
    const unsigned* __restrict__ bi = reinterpret_cast<const unsigned*>(a.ws_idx) + (int64_t)q * T_all * 64;
    unsigned hi[NCH];
    int ix[NCH];
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      hi[t] = t < T ? bv[t * 64 + lane] : 0u;  // (0 < the image of -inf: never counted, never wanted)
      ix[t] = t < T ? (int)~bi[t * 64 + lane] : kPadIdx;
      if (ix[t] == kPadIdx) hi[t] = 0u;
    }
    int evict = 0;
    if (lane < n_lists) evict = a.list_evict[(int64_t)q * n_lists_all + lane];
    const float band = a.ws_delta[q];
    // F_k: the largest key image t with at least k entries >= t (0 while fewer than k entries exist)
    const unsigned fk = finish_fk_upto<2, NCH>(hi, T, a.k);
    const float cut = (fk ? key2f(fk) : -INFINITY) - band;
    const unsigned cutk = f2key(cut);
    // survivors -> queue (those of the seed chunks are only counted: they keep their values, see the header); a list
    // that evicted and still ends at or above the cut lost one that mattered
    int n_c = 0, n_q = 0;
    bool lost = false;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c >= T) break;  // (wave-uniform)
      const bool want = hi[c] != 0u && hi[c] >= cutk;
      const unsigned long long mask = __ballot(want);
      const int n = __popcll(mask);
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
      n_c += n;
      if (c >= seed_chunks) {  // (wave-uniform)
        if (want && n_q + rank < RM * 64) qi[n_q + rank] = ix[c];
        n_q += n;
      }
      // (chunk c is rank chunk c % RL of list c / RL: its lane 63 is the list's last entry when c % RL == RL - 1)
      const int l = c / (RL > 0 ? RL : 1);
      const bool last_chunk = (c % (RL > 0 ? RL : 1)) == RL - 1;
      const int ev = __builtin_amdgcn_readlane(evict, l < 64 ? l : 0);
      lost = lost || (last_chunk && ev && ((mask >> 63) & 1ull));
    }
    lost = lost || n_c > RM * 64;
    if (lost) {  // (wave-uniform)
      if (lane == 0) a.flags[q] = a.epoch;
      continue;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    WaveTopK<RM> ex;
    ex.init();
    // the seed chunks' survivors, as they are
#pragma unroll 1
    for (int s = 0; s < seed_chunks; ++s) {
      unsigned h = 0u;
      int x = kPadIdx;
#pragma unroll
      for (int c = 0; c < kSeedMax; ++c) {
        h = c == s ? hi[c] : h;  // (wave-uniform selects: the chunks stay in their registers)
        x = c == s ? ix[c] : x;
      }
      const bool want = h != 0u && h >= cutk;
      if (__ballot(want) == 0ull) continue;
      ex.insert_unsorted(want ? Key{h, ~(unsigned)x} : pad_key());
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      if (r * 64 >= n_q) break;  // wave-uniform
      const bool want = r * 64 + lane < n_q;
      const int idx = want ? qi[r * 64 + lane] : 0;  // (idle lanes walk slot 0's bytes: in range)
      typename L::chunk_t cw[L::kChunks];
      L::load(a.packed, a.n_slots, idx, cw);
      // sub-quantizer order, block by block (scan_layout::subq_at): inside a block of B positions from base b,
      // out dword D byte Y = in dword D ^ (x >> 2), byte Y ^ (x & 3), x = idx mod B -- a byte permute per dword for
      // the low two bits of x, log2(B / 4) rounds of conditional dword swaps for the others
      unsigned cd[G];
#pragma unroll
      for (int d = 0; d < G; ++d) {
        constexpr int dummy = 0;
        (void)dummy;
        const scan_layout::BlockAt<M> kb(4 * d);
        const unsigned x = (unsigned)idx & (unsigned)(kb.size - 1);
        const unsigned sel = 0x03020100u ^ ((x & 3u) * 0x01010101u);
        const unsigned wd = L::word(cw, d);
        cd[d] = __builtin_amdgcn_perm(wd, wd, sel);
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int d = 0; d < G; ++d) {
          const scan_layout::BlockAt<M> kb(4 * d);
          const int dr = d - (kb.base >> 2);            // dword inside the block
          if ((4 << b) < kb.size && (dr & (1 << b)) == 0) {  // the block has this XOR bit; d is the pair's lower dword
            const bool sw = (((unsigned)idx >> (2 + b)) & 1u) != 0u;  // (bit 2 + b of idx mod B: 4 << b < B)
            const unsigned lo = cd[d], up = cd[d | (1 << b)];         // (blocks are aligned to their size: | == +)
            cd[d] = sw ? up : lo;
            cd[d | (1 << b)] = sw ? lo : up;
          }
        }
      }
      float v = 0.f;
      if constexpr (FROM_LUT) {
        // the caller's table: entry (j, c) of query q at lut[(j * nq + q) * 256 + c]; all loads first, adds ascending j
        float ent[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const unsigned c = (cd[j >> 2] >> (8 * (j & 3))) & 255u;
          ent[j] = a.lut[((int64_t)j * a.nq + q) * 256 + (int)c];
        }
#pragma unroll
        for (int j = 0; j < M; ++j) v += ent[j];
      } else {
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const unsigned c = (cd[j >> 2] >> (8 * (j & 3))) & 255u;
          float dot = 0.f, c2 = 0.f;
          if constexpr (DS != 0) {
#pragma unroll
            for (int e = 0; e < DS; ++e) {
              const int i = j * DS + e;
              const float y = cb[i * 256 + (int)c];
              const float xx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xv[i >> 6]), i & 63));
              dot = fmaf(xx, y, dot);
              c2 = fmaf(y, y, c2);
            }
          } else {
            for (int e = 0; e < ds; ++e) {  // (wave-uniform trip count and lane index)
              const int i = j * ds + e;
              const float y = cb[i * 256 + (int)c];
              const int x0 = __builtin_amdgcn_readlane(__float_as_int(xv[0]), i & 63);
              const int x1 = __builtin_amdgcn_readlane(__float_as_int(xv[1]), i & 63);
              const float xx = __int_as_float(i < 64 ? x0 : x1);
              dot = fmaf(xx, y, dot);
              c2 = fmaf(y, y, c2);
            }
          }
          // (fused_lut4's arithmetic, operation for operation)
          float val = 2.f * dot;
          val = val - __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q2v), j));
          val = val - c2;
          v += euclid ? val : dot;
        }
      }
      ex.insert_unsorted(want ? make_key(v + 0.0f, idx) : pad_key());
    }
    write_final<RM>(a, q, ex);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the next query overwrites the queue
  }
}

// pool mode, phase 2: the query's n_lists sorted lists of exact candidates (64 RX entries each, pads last) are
// merged BY RANK in LDS (rank_merge: fixed-step binary searches, eight lists in flight per lane) and the best k
// written out.  A flagged query (a pool or a list overflowed) is left to the exact kernel.
constexpr int kPoolMergeThreads = 512;
template <int NW>
__global__ __launch_bounds__(kPoolMergeThreads) void scan_pool_merge_kernel(ScanArgs a) {
  constexpr int RX = NW == 4 ? 8 : 4, LEN = 64 * RX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int q = blockIdx.x;
  if (a.flags[q] == a.epoch) return;
  const int L = a.n_split * NW;
  unsigned* mhi = reinterpret_cast<unsigned*>(smem);
  unsigned* mlo = mhi + L * LEN;
  unsigned* ohi = mlo + L * LEN;
  const int kcap = (a.k + 63) / 64 * 64;
  unsigned* olo = ohi + kcap;
  for (int l = threadIdx.x >> 6; l < L; l += kPoolMergeThreads / 64) {
    const int64_t o = ((int64_t)q * L + l) * a.pool_cap;
    for (int e = threadIdx.x & 63; e < LEN; e += 64) {
      mhi[l * LEN + e] = a.pool_hi[o + e];
      mlo[l * LEN + e] = a.pool_lo[o + e];
    }
  }
  const Key pad = pad_key();
  for (int i = threadIdx.x; i < kcap; i += kPoolMergeThreads) {
    ohi[i] = pad.hi;
    olo[i] = pad.lo;
  }
  __syncthreads();
  rank_merge<LEN>(mhi, mlo, L, ohi, olo, kcap, (int)threadIdx.x, kPoolMergeThreads);
  __syncthreads();
  for (int e = threadIdx.x; e < a.k; e += kPoolMergeThreads) {
    const Key kk{ohi[e], olo[e]};
    const int idx = key_index(kk);
    const bool p = idx == kPadIdx;
    const int64_t o = (int64_t)q * a.k + e;
    a.out_vals[o] = p ? -INFINITY : key_value(kk);
    a.out_addr[o] = p ? -1 : (int64_t)idx;
    if (a.out_ids) a.out_ids[o] = p ? -1 : a.address2id[idx];
  }
}

}  // namespace tpq
