// tpq_coarse_assign through the fp16 cascade (fp16_cascade.h; called from assign_fast.hip): one problem, many
// centroids.  Wide vectors (128 < d <= 1024) take the GEMM-shaped path (run_wide), d <= 128 the level kernels of
// cascade_core.hip on points prepared per call (run_assign).  Both end in the same exact step on candidate
// (point, centroid) pairs (run_pair_tail).
#include <stdlib.h>

#include "fp16_cascade.h"
#include "wave_topk.h"

namespace tpq {
namespace lloyd {

// =========================================================================================================
// Wide vectors (128 < d <= 1024): GEMM-shaped, and the exact step works on CANDIDATES (the
// coarse assign of a GIST-dimension index -- 1 M x 16 384 x 960 -- is 270-320 ms on the fp32 MFMA)
// =========================================================================================================
// Beyond 128 dimensions a wave can no longer keep its points' pieces in registers, so both operands are
// streamed: a block owns 256 points x ALL centroids; per block of 256 centroids it runs the K loop over the
// k-steps with both operands' fragments coming through a double-buffered LDS ring by LDS-DMA (4 k-steps per
// stage: 32 KiB of centroid fragments + 32 KiB of point fragments), 8 waves as 4 point slabs x 2 centroid
// halves, each wave 64 points x 128 centroids = 8 accumulators; after the K loop the -N MFMAs and the
// epilogue over the 128 values per lane -- amortised over KS x 8 MFMAs.
//
// At d ~ 1000 every (d 2^-24)-sized term of the bound -- the fast path's accumulation AND the exact kernel's
// own rounding, which no fast path can remove -- is worth percents of the points: a third product pass
// (level 2 of the narrow path) would turn 18 % undecided into 11 %, and the exact kernel over 11 % of a
// million points is a third of the full problem.  So the wide path never runs the exact kernel over all
// centroids.  What the bound does give for an undecided point is a short list of CANDIDATES: the exact
// winner w satisfies f_w >= f_best - 2 delta.  Three passes:
//   1. gemm_kernel<false>: hi pieces, key top-2 of every point; gdecide_kernel decides 80 % and lists the rest
//      with its threshold f_best - 2 delta;
//   2. gemm_kernel<true> over the listed points (hi pieces gathered into a compact fragment array): every
//      (point, centroid) at or above the point's threshold goes to a pair list -- 2-3 per listed point;
//   3. pair_exact_kernel: the exact kernel's value of each pair -- the SAME instruction sequence as
//      max_sim_kernel (max_sim.hip): ascending-k fma chains for |x|^2 and |c|^2, v_mfma_f32_32x32x2f32 over
//      ascending k pairs, 2 acc - |x|^2 - |c|^2 -- 32 pairs per wave on the diagonal of a 32 x 32 tile,
//      folded per point with the 64-bit atomicMax key of the exact kernel's split mode (value, then the
//      smaller index).
// Pair lists that overflow (degenerate data: duplicates by the thousand, non-finite values) fall back to
// the exact kernel over the level-1 list: correctness never depends on the candidate counts.
// Operand layout: plain MFMA-fragment order [tile of 32 rows][k-step][lane] x 16 B for points and
// centroids alike (every access is a 1-KiB stream).
constexpr int kGK = 4;                       // k-steps per LDS stage
constexpr int kGStage = 2 * 8 * kGK * 1024;  // bytes of a stage: 8 centroid units + 8 point tiles, kGK k-steps each
constexpr int kPairList = 4096;              // LDS-staged (row, centroid) entries per block between flushes

struct PairList {
  int n;
  int base;
  unsigned item[kPairList];  // row in the block (8 bits) << 22 | centroid
};

struct GemmArgs {
  const u32x4* cfr;      // centroid operand [units][KA][64]
  const u32x4* pfr;      // point operand [tiles][KA][64]
  const u32x4* cnorm;    // [units][64]: -N as three bf16 pieces at k = 0, 1, 2 (-3e38 beyond n)
  float2* part_b;        // pass 1: [2 * ysplit][rows] (best, second) per centroid half
  int* part_i;           // pass 1: [2 * ysplit][rows] centroid index
  int KA;                // k-steps of the operands (multiple of kGK)
  int n_cblocks;         // blocks of 256 centroids
  int ysplit;            // 1, 2, 4 or 8 ranges of centroid blocks (see the block mapping in the kernel)
  int pblocks;           // blocks of 256 points the grid covers
  int64_t rows;          // points (pass 1) / capacity of the compact array (pass 2)
  const int* count_in;   // pass 2: number of listed points on the device (rows = min(this, capacity))
  const float* thr;      // pass 2: [capacity] threshold of the listed point
  uint2* pairs;          // pass 2: (list position, centroid)
  int* pair_count;
  int pair_cap;
  int* overflow;         // pass 2: set when a pair was dropped
  int n_centroids;       // pass 2: centroids beyond are padding (never a pair, whatever their value)
};

// the block's staged pairs -> the global list.  Called by all threads, at points where nobody appends.
__device__ __forceinline__ void flush_pairs(const GemmArgs& a, PairList* pl, unsigned row0) {
  if (threadIdx.x == 0) {
    const int n = pl->n < kPairList ? pl->n : kPairList;
    if (pl->n > kPairList) atomicOr(a.overflow, 1);
    pl->base = n ? atomicAdd(a.pair_count, n) : 0;
  }
  __syncthreads();
  const int n = pl->n < kPairList ? pl->n : kPairList, base = pl->base;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const unsigned e = pl->item[i];
    if (base + i < a.pair_cap)
      a.pairs[base + i] = make_uint2(row0 + (e >> 22), e & 0x3fffffu);
    else
      atomicOr(a.overflow, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) pl->n = 0;
}

// CT = point column tiles per wave: 2 -> 8 waves as 4 point slabs x 2 centroid halves (wave tile 128 x 64),
// 4 -> 4 waves as 2 x 2 (wave tile 128 x 128, one wave per SIMD, 16 accumulators)
template <bool CAND, int CT>
__global__ __launch_bounds__(CT == 2 ? 512 : 256) void gemm_kernel(GemmArgs a) {
  constexpr int NW = CT == 2 ? 8 : 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 stages, the block's -N fragments (8 KiB), PairList
  int64_t rows = a.rows;
  if (CAND) {
    const int c = *a.count_in;
    rows = c < a.rows ? c : a.rows;
  }
  // Block -> (point block pb, centroid range yi), XCD-aware.  A 256 x 256 tile streams 2 x 480 KiB at d = 960 and
  // every point block meets every centroid block: with one point block per CU walking all centroids, the 32
  // CUs of an XCD share the centroid stream but re-read 32 x 480 KiB = 15 MiB of point fragments per step --
  // four times their 4-MiB L2, i.e. from the Infinity Cache every time.  So the 32 blocks an XCD runs
  // side by side (the dispatcher deals block b to XCD b % 8, in order) are P = 32 / ysplit point blocks x
  // ysplit centroid ranges: per step they stream P + ysplit tiles instead of 33 (ysplit = 8: 12).
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, ys = a.ysplit, P = 32 / ys;
  const int pb = ((slot >> 5) * 8 + xcd) * P + (slot & 31) / ys, yi = (slot & 31) % ys;
  if (pb >= a.pblocks || (int64_t)pb * 256 >= rows) return;  // block-uniform
  // (the wave number as a SCALAR: everything derived from it -- the addresses of the LDS-DMA fills above all --
  // is then SALU work; as a vector it was 6 VALU instructions per MFMA in the issue slots the MFMAs need)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;  // point slab (64 points), centroid half (128 centroids)
  const int cb_per = (a.n_cblocks + ys - 1) / ys;
  const int cb0 = yi * cb_per, cb1 = (cb0 + cb_per) < a.n_cblocks ? (cb0 + cb_per) : a.n_cblocks;
  if (cb0 >= cb1) return;
  const int n_kst = a.KA / kGK;  // stages per centroid block (>= 3: d > 128)
  const int n_stage = (cb1 - cb0) * n_kst;
  char* nbuf = smem + 2 * kGStage;
  PairList* pl = reinterpret_cast<PairList*>(nbuf + 8 * 1024);
  if (CAND && threadIdx.x == 0) pl->n = 0;
  // stage (centroid block cb, k-steps [kGK kst, + kGK)) -> buffer buf: units 0..7 then point tiles 0..7, each
  // kGK consecutive 1-KiB fragments
  const unsigned lane16 = lane * 16;
  auto stage = [&](int cb, int kst, int buf) {
    char* dst = smem + buf * kGStage;
    const char* csrc = reinterpret_cast<const char*>(a.cfr) + ((size_t)cb * 8 * a.KA + kst * kGK) * 1024;
    const char* psrc = reinterpret_cast<const char*>(a.pfr) + ((size_t)pb * 8 * a.KA + kst * kGK) * 1024;
#pragma unroll
    for (int i = 0; i < 8 * kGK / NW; ++i) {  // this wave's share of the 8 kGK centroid fragments, then of the points'
      const int f = wave + i * NW, who = f / kGK, kk = f % kGK;
      const size_t off = ((size_t)who * a.KA + kk) * 1024;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(csrc + off + lane16),
                                       (__attribute__((address_space(3))) void*)(dst + f * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(psrc + off + lane16),
                                       (__attribute__((address_space(3))) void*)(dst + (8 * kGK + f) * 1024), 16, 0, 0);
    }
  };
  stage(cb0, 0, 0);
  f32x16 acc[4][CT];  // [centroid row tile of this wave's half][point column tile of its slab]
  float b1[CT], b2[CT], thr[CT];
  int bu[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    b1[ct] = -INFINITY;
    b2[ct] = -INFINITY;
    bu[ct] = 0;
    // (NaN: no value compares >= it.  With +inf a column of garbage fragments -- the rows of the last block beyond
    // the list are never gathered -- that happened to hold an inf passed the test: a pair of a list position
    // beyond the count, an address from an unwritten list entry, a memory fault: tools/selection_soak.py seed 11)
    thr[ct] = __builtin_nanf("");
    if (CAND) {
      const int64_t row = (int64_t)pb * 256 + wr * (CT * 32) + ct * 32 + l31;
      if (row < rows) thr[ct] = a.thr[row];
    }
  }
  const bf16x8 bones = ones3_bf16x8(half);  // B fragment of ones at k = 0, 1, 2
  const f32x16 zero = zero_f32x16();
  int cb = cb0, kst = 0;
#pragma unroll 1
  for (int g = 0; g < n_stage; ++g, ++kst) {
    if (kst == n_kst) {
      kst = 0;
      ++cb;
    }
    __syncthreads();  // stage g has landed; everyone is done with the other buffer (and with nbuf)
#ifndef TPQ_EXP_NODMA  // (experiment: the K loop without its LDS-DMA fills, garbage results: 22.6 instead of 28.7 ms.
                       // Two restructurings that were built and measured, neither kept: the points' fragments global ->
                       // registers instead (half the fills, a third fewer LDS reads): 30.4 ms -- fragment-shaped
                       // loads cost more on the vector memory path than they save in LDS; a ring of four 2-k-step
                       // stages with inline-asm fills and a barrier that leaves the newest stage in flight
                       // (`s_waitcnt vmcnt(4)`), next stage's first fragments read before the barrier: 31.0 ms --
                       // twice the barriers cost more than the refill bubble they remove)
    if (g + 1 < n_stage) {
      const bool wrap = kst + 1 == n_kst;
      stage(wrap ? cb + 1 : cb, wrap ? 0 : kst + 1, (g + 1) & 1);
    }
#endif
    if (kst == 0) {  // a new centroid block: its -N fragments (8 KiB; read after the K loop) and fresh accumulators
      for (int f = wave; f < 8; f += NW)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(reinterpret_cast<const char*>(a.cnorm) +
                                                           ((size_t)cb * 8 + f) * 1024 + lane * 16),
            (__attribute__((address_space(3))) void*)(nbuf + f * 1024), 16, 0, 0);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = zero;
      // (pairs are appended in the epilogue of the previous centroid block, before the barrier above:
      // pl->n is stable here, and the condition uniform)
      if (CAND && pl->n >= kPairList / 2) flush_pairs(a, pl, pb * 256u);
    }
    const u32x4* sb = reinterpret_cast<const u32x4*>(smem + (g & 1) * kGStage) + lane;
    // software pipeline inside the stage: the 4 + CT fragments of k-step kk + 1 are read before the MFMAs of
    // k-step kk issue (left to itself the compiler reads ONE A fragment, waits, issues its CT MFMAs, reads the next)
    f16x8 af[2][4], bf[2][CT];
    auto read_frags = [&](int kk, int set) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) af[set][rt] = __builtin_bit_cast(f16x8, sb[((wc * 4 + rt) * kGK + kk) * 64]);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        bf[set][ct] = __builtin_bit_cast(f16x8, sb[((8 + wr * CT + ct) * kGK + kk) * 64]);
    };
    read_frags(0, 0);
#pragma unroll
    for (int kk = 0; kk < kGK; ++kk) {
      if (kk + 1 < kGK) read_frags(kk + 1, (kk + 1) & 1);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[kk & 1][rt], bf[kk & 1][ct], acc[rt][ct], 0, 0, 0);
      if (kk + 1 < kGK) __builtin_amdgcn_sched_group_barrier(0x100, 4 + CT, 0);  // DS read
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * CT, 0);                      // MFMA
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kst == n_kst - 1) {  // the centroid block is complete: -N, then the epilogue over CT x 64 values per lane
      // (nbuf was requested n_kst stages ago and every barrier since waited for vmcnt(0))
      const u32x4* nb = reinterpret_cast<const u32x4*>(nbuf) + lane;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        const bf16x8 cf = __builtin_bit_cast(bf16x8, nb[(wc * 4 + rt) * 64]);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cf, bones, acc[rt][ct], 0, 0, 0);
      }
      if (!CAND) {
        float before[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) before[ct] = b1[ct];
        static_for<0, 4>([&](auto rt_c) {
          constexpr int rt = decltype(rt_c)::value;
          static_for<0, 8 * CT>([&](auto q_c) {  // 8 register pairs x CT column tiles
            constexpr int q = decltype(q_c)::value, ct = q % CT, pq = q / CT;
            top2_keys_pair(b1[ct], b2[ct], key6<16 * rt + 2 * pq>(acc[rt][ct][2 * pq]),
                           key6<16 * rt + 2 * pq + 1>(acc[rt][ct][2 * pq + 1]));
          });
        });
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) bu[ct] = b1[ct] > before[ct] ? cb : bu[ct];
      } else {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            float mx = acc[rt][ct][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[rt][ct][r]);
            if (__ballot(mx >= thr[ct]) == 0ull) continue;  // (nearly every tile)
            const unsigned rowbits = (unsigned)(wr * (CT * 32) + ct * 32 + l31) << 22;
            const int cbase = cb * 256 + wc * 128 + rt * 32 + 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const bool hit = acc[rt][ct][r] >= thr[ct] && cbase + (r & 3) + 8 * (r >> 2) < a.n_centroids;
              const unsigned long long mk = __ballot(hit);
              if (mk) {
                const int leader = __ffsll((long long)mk) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&pl->n, __popcll(mk));  // LDS
                base = __shfl(base, leader, 64);
                const int slot = base + __popcll(mk & ((1ull << lane) - 1ull));
                if (hit && slot < kPairList) pl->item[slot] = rowbits | (unsigned)(cbase + (r & 3) + 8 * (r >> 2));
              }
            }
          }
      }
    }
  }
  if (CAND) {
    __syncthreads();
    flush_pairs(a, pl, pb * 256u);
    return;
  }
  // this wave's (best, second, index) of its 2 x 32 points over its centroid half of every block
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int tag = __float_as_int(b1[ct]) & 63, r0 = tag & 15;
    int idx = bu[ct] * 256 + wc * 128 + (tag >> 4) * 32 + (r0 & 3) + 8 * (r0 >> 2) + 4 * half;
    const float m1 = b1[ct], m2 = b2[ct];
    const float o1 = __shfl_xor(m1, 32, 64), o2 = __shfl_xor(m2, 32, 64);
    const int oi = __shfl_xor(idx, 32, 64);
    const float B1 = fmaxf(m1, o1);
    const float B2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
    if (o1 > m1 || (o1 == m1 && oi < idx)) idx = oi;
    const int64_t row = (int64_t)pb * 256 + wr * (CT * 32) + ct * 32 + l31;
    if (half == 0 && row < rows) {
      const int64_t slot = (int64_t)(yi * 2 + wc) * a.rows + row;
      a.part_b[slot] = make_float2(B1, B2);
      a.part_i[slot] = idx;
    }
  }
}

// points -> fragment order: hi [T][KAp][64] x 16 B (k-steps beyond ceil(d / 16) zero), norms.  grid (ceil(T / 4))
__global__ __launch_bounds__(256) void gsplit_points_kernel(const float* __restrict__ A, const float* __restrict__ mu,
                                                           const float* __restrict__ scale, u32x4* __restrict__ hi,
                                                           float4* __restrict__ norms, int d, int64_t m, int64_t T,
                                                           int KAp) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  if (tile >= T) return;
  const int64_t i = tile * 32 + l31;
  const bool iv = i < m;
  const float* Ap = A + (iv ? i : 0);
  const float s = scale[0];
  float n2c = 0.f, n2r = 0.f, n2m = 0.f;
  for (int st = 0; st < KAp; ++st) {
    f16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * st + 8 * half + j;
      const float x = (iv && k < d) ? Ap[(int64_t)k * m] : 0.f;
      const float v = (iv && k < d) ? (x - mu[k]) * s : 0.f;
      const _Float16 hh = (_Float16)v;
      const float r = v - (float)hh;  // exact: what the fast path drops of this element
      h[j] = hh;
      n2c = fmaf(v, v, n2c);
      n2r = fmaf(x, x, n2r);
      n2m = fmaf(r, r, n2m);
    }
    hi[(tile * KAp + st) * 64 + lane] = __builtin_bit_cast(u32x4, h);
  }
  n2c += __shfl_xor(n2c, 32, 64);
  n2r += __shfl_xor(n2r, 32, 64);
  n2m += __shfl_xor(n2m, 32, 64);
  if (half == 0 && iv) norms[i] = make_float4(n2c, n2r, n2m, 0.f);
}

// centroids -> operand c1 [U][KAp][64] (hi piece of C = 2 c'; inner product: C = c'), -N fragments, max
// norms, range flag.  grid (U), U = 8 x blocks of 256
__global__ __launch_bounds__(64) void gprep_centroids_kernel(const float* __restrict__ B, const float* __restrict__ mu,
                                                            const float* __restrict__ scale, u32x4* __restrict__ c1,
                                                            u32x4* __restrict__ cnorm, unsigned* __restrict__ cmax2_bits,
                                                            int* __restrict__ cflag, int d, int n, int KAp, int euclid) {
  const int unit = blockIdx.x, lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  const int c = unit * 32 + l31;
  const float s = scale[0];
  float N = 0.f, sraw = 0.f;
  if (c < n) {  // |c'|^2 in double, rounded once: a chain of d fp32 roundings would be a term of the bound
    double Nd = 0.0;
    for (int k = 0; k < d; ++k) {
      const float y = B[(int64_t)k * n + c];
      const float cc = (y - mu[k]) * s;
      Nd += (double)cc * (double)cc;
      sraw = fmaf(y, y, sraw);
    }
    N = (float)Nd;
  }
  float c2m = 0.f;  // |C - Ch|^2: what the fast path drops of this centroid
  int bad = 0;
  {
    bf16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
    if (half == 0) {
      __bf16 p1, p2, p3;
      split3_bf16(c < n ? (euclid ? -N : 0.f) : -3.0e38f, p1, p2, p3);  // inner product: no norm
      f[0] = p1;
      f[1] = p2;
      f[2] = p3;
    }
    cnorm[(int64_t)unit * 64 + lane] = __builtin_bit_cast(u32x4, f);
  }
  if (c < n) {
    bad |= !(N <= 3.0e38f) | !(sraw <= 3.0e38f);
    if (half == 0 && !bad) {
      atomicMax(cmax2_bits, __float_as_uint(N));
      atomicMax(cmax2_bits + 1, __float_as_uint(sraw));
    }
  }
  for (int st = 0; st < KAp; ++st) {
    f16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * st + 8 * half + j;
      const float C = (k < d && c < n) ? (euclid ? 2.f : 1.f) * ((B[(int64_t)k * n + c] - mu[k]) * s) : 0.f;
      bad |= !(fabsf(C) <= 65000.f);
      const _Float16 hh = (_Float16)C;
      const float r = C - (float)hh;
      h[j] = hh;
      c2m = fmaf(r, r, c2m);
    }
    c1[((int64_t)unit * KAp + st) * 64 + lane] = __builtin_bit_cast(u32x4, h);
  }
  c2m += __shfl_xor(c2m, 32, 64);
  if (half == 0 && c < n && !bad) atomicMax(cmax2_bits + 2, __float_as_uint(c2m));
  if (bad) atomicOr(cflag, 1);
}

// pass 2's point operand: the listed points' hi fragments, compact: position pos of the list -> tile
// pos / 32, row pos % 32.  grid (ceil(cap / 32)), one wave per compact tile
__global__ __launch_bounds__(64) void ggather_kernel(const u32x4* __restrict__ hi, const int* __restrict__ list,
                                                    const int* __restrict__ count, u32x4* __restrict__ out, int KAp,
                                                    int cap) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  int cnt = *count;
  cnt = cnt < cap ? cnt : cap;
  const int64_t pos = (int64_t)blockIdx.x * 32 + l31;
  if ((int64_t)blockIdx.x * 32 >= cnt) return;
  const int p = pos < cnt ? list[pos] : -1;
  const int64_t src = p >= 0 ? ((int64_t)(p >> 5) * KAp) * 64 + half * 32 + (p & 31) : 0;
  const u32x4 z = {0u, 0u, 0u, 0u};
  u32x4* o = out + ((int64_t)blockIdx.x * KAp) * 64 + lane;
  for (int st = 0; st < KAp; ++st) o[(int64_t)st * 64] = p >= 0 ? hi[src + (int64_t)st * 64] : z;
}

// fold the partial results of a point and decide; an undecided point is listed with its candidate
// threshold.  grid (ceil(m / 256))
struct GDecideArgs {
  const float2* part_b;
  const int* part_i;
  int n_part;
  int64_t rows;                // stride of the partial tables
  const float4* norms;         // [m]: |a'|^2, |x|^2, |a' - ah|^2
  const unsigned* cmax2_bits;  // max N, max |c|^2, max |C - Ch|^2
  const float* scale;
  const int* flag;
  const int* cflag;
  int64_t* inds;
  float* vals;
  int* list;
  int* count;
  float* thr;  // [cap]
  int cap;
  int m;
  float eps, eps_exact, eta;  // eps: everything but the dropped pieces, relative to (|a'| + |c'|max)^2
  int euclid;                 // 0: inner product (no centring, C = c', no norms: the bounds hold a fortiori)
};
// The bound (the derivation of the header comment, with the refinements that matter at d ~ 1000):
//  * the dropped products are bounded by what was actually dropped -- |a' - ah| of the point (split kernel)
//    and max |C - Ch| over the centroids (prep kernel):
//        |sum (a C - ah Ch)| <= |a' - ah| (|Ch|max + |C - Ch|max) + |a'| |C - Ch|max,   |Ch| <= (1 + 2^-11) 2 |c'|
//    -- about a third of the worst case 2^-11 (|a'| + |c'|max)^2;
//  * accumulation: an MFMA adds 16 products and the accumulator, <= 17 roundings of <= 2^-23 (truncation
//    allowed for) of the running magnitude, which is <= sum |a_k C_k| + N <= |a'| 2 |c'| + |c'|^2: at most
//    (|a'| + |c'|)^2 / 2 for the products: (17 (KS + 1) + 8) 2^-24;
//  * N = fl(|c'|^2) is summed in double and rounded once (2^-24 N);
//  * pass 1 compares KEYS (2^-17 |v| off, |v| <= (.)^2), pass 2 the values themselves against the key of
//    the best minus 2 delta: the exact winner's value is within delta of its exact value, the best key within
//    delta of ITS exact value, so the winner is at or above the threshold (lowered by one more key error
//    and a denormal: delta = 0 -- all-zero data -- must still list the best itself).
__global__ __launch_bounds__(256) void gdecide_kernel(GDecideArgs a) {
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = pos < a.m;
  const int p = valid ? (int)pos : 0;
  float B1 = -INFINITY, B2 = -INFINITY;
  int idx = 0;
  if (valid)
    for (int c = 0; c < a.n_part; ++c) {
      const float2 v = a.part_b[(int64_t)c * a.rows + pos];
      const int i = a.part_i[(int64_t)c * a.rows + pos];
      const float n2 = fmaxf(fminf(B1, v.x), fmaxf(B2, v.y));
      idx = (v.x > B1 || (v.x == B1 && i < idx)) ? i : idx;
      B1 = fmaxf(B1, v.x);
      B2 = n2;
    }
  const float s = a.scale[0];
  const float cn = sqrtf(__uint_as_float(a.cmax2_bits[0])), cnr = sqrtf(__uint_as_float(a.cmax2_bits[1]));
  const float4 n2 = a.norms[p];
  const float an = sqrtf(n2.x), anr = sqrtf(n2.y) * s;
  const float t1 = an + cn, t2 = anr + cnr * s;
  const float a2 = sqrtf(n2.z), c2 = sqrtf(__uint_as_float(a.cmax2_bits[2]));
  const float cscale = a.euclid ? 2.002f : 1.001f;
  const float dropped = a2 * (cscale * cn + c2) + 1.001f * an * c2;
  float delta = 1.25f * (dropped + a.eps * t1 * t1 + a.eta * (2.f * cn + an) + a.eps_exact * t2 * t2);
  if ((a.flag[0] | a.cflag[0]) != 0) delta = INFINITY;
  if (valid) {
    a.inds[p] = idx;
    if (a.vals) a.vals[p] = (a.euclid ? B1 - n2.x : B1) * ((1.f / s) * (1.f / s));
  }
  const bool listed = valid && !(B1 - B2 > 2.f * delta);
  int slot;
  if (wave_append(listed, a.count, slot)) {
    a.list[slot] = p;
    // (a flagged problem -- delta = inf, keys possibly inf / NaN -- emits no candidates: gdecode_kernel sends
    // its whole list to the exact kernel)
    if (slot < a.cap)
      a.thr[slot] = (a.flag[0] | a.cflag[0]) != 0 ? __builtin_nanf("")  // (no value compares >= NaN, not even inf)
                                                  : B1 - 2.f * delta - (fabsf(B1) * (1.0f / 65536.0f) + 1.0e-30f);
  }
}

// pass 3 reads ROWS: a (point, centroid) pair needs one column of A [d][m] and one of B [d][n] -- 4 useful bytes
// per 64-byte sector as they lie (7 ms for 400 000 pairs at d = 960).  rows_kernel copies the columns it is given
// into rows out[j][dp] (dp = d rounded up to 16, zero padded): all centroids once per call (63 MB at 16 384 x
// 960), and the listed points (their columns are ascending and ~5 apart: a few sectors per dimension).
// grid (ceil(count / 32)), 64 lanes: lane (column i, half) gathers 16 consecutive dimensions, stores 64 B.
__global__ __launch_bounds__(64) void rows_kernel(const float* __restrict__ M, int64_t cols, const int* __restrict__ list,
                                                 const int* __restrict__ count, int cap, float* __restrict__ out, int d,
                                                 int dp) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  int cnt = cap;
  if (count) {
    cnt = *count;
    cnt = cnt < cap ? cnt : cap;
  }
  if ((int64_t)blockIdx.x * 32 >= cnt) return;
  const int j = blockIdx.x * 32 + l31;
  const bool valid = j < cnt;
  const int64_t col = valid ? (list ? list[j] : j) : 0;
  const float* src = M + col;
  float* dst = out + (int64_t)j * dp;
  for (int k0 = 16 * half; k0 < dp; k0 += 32) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = (k0 + u < d) ? src[(int64_t)(k0 + u) * cols] : 0.f;
    if (valid) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(dst + k0 + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
  }
}

// pass 3: the exact kernel's value of every (listed point, candidate centroid) pair, folded into keys[point].
// A wave takes 32 pairs: lane (pair i, half); half 0 streams the point's row, half 1 the centroid's row -- each
// the ascending-k fma chain of its squared norm as max_sim_kernel forms it -- and per pair of dimensions
// the halves swap what the other needs as MFMA operand (row i = centroid of pair i, column i = point of pair
// i: the diagonal of the 32 x 32 tile holds the 32 results).  The zero padding beyond d adds +0 to chains and
// products alike.
__global__ __launch_bounds__(256) void pair_exact_kernel(const float* __restrict__ Xt, const float* __restrict__ Bt,
                                                        const uint2* __restrict__ pairs, const int* __restrict__ pair_count,
                                                        int pair_cap, const int* __restrict__ list,
                                                        unsigned long long* __restrict__ keys, int dp, int euclid) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  int cnt = *pair_count;
  cnt = cnt < pair_cap ? cnt : pair_cap;
  const int tiles = (cnt + 31) >> 5;
  for (int tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
    const int q = tile * 32 + l31;
    const bool valid = q < cnt;
    const uint2 pr = valid ? pairs[q] : make_uint2(0u, 0u);
    const int p = valid ? list[pr.x] : 0;
    const int c = (int)pr.y;
    const float4* src = reinterpret_cast<const float4*>(half ? Bt + (int64_t)c * dp : Xt + (int64_t)pr.x * dp);
    f32x16 acc = zero_f32x16();
    float chain = 0.f;  // half 0: |x|^2, half 1: |c|^2
    for (int k0 = 0; k0 < dp; k0 += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 t = src[(k0 >> 2) + u];
        v[4 * u] = t.x;
        v[4 * u + 1] = t.y;
        v[4 * u + 2] = t.z;
        v[4 * u + 3] = t.w;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) chain = fmaf(v[u], v[u], chain);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // lane (i, half) multiplies dimension 2 j + half: half 0 keeps x[2j] and sends x[2j+1], half 1
        // keeps c[2j+1] and sends c[2j]
        const float own = half ? v[2 * j + 1] : v[2 * j];
        const float got = __shfl_xor(half ? v[2 * j] : v[2 * j + 1], 32, 64);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(half ? own : got, half ? got : own, acc, 0, 0, 0);
      }
    }
    const float other = __shfl_xor(chain, 32, 64);
    const float x2 = half ? other : chain, c2 = half ? chain : other;
    // D[row i][col i]: column = l31, row = (r & 3) + 8 (r >> 2) + 4 half
    const int rsel = (l31 & 3) | ((l31 >> 3) << 2);
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) dot = (r == rsel) ? acc[r] : dot;
    float v = dot;
    if (euclid) {
      v = 2.f * v;
      v = v - x2;
      v = v - c2;
    }
    v = v + 0.f;  // (-0 -> +0: the key orders by bits)
    if (valid && half == ((l31 >> 2) & 1)) {
      const unsigned long long key = key_u64(make_key(v, c));
      atomicMax(keys + p, key);
    }
  }
}

// labels / values of the listed points from their keys; then the fallback switch: the exact kernel runs
// over the level-1 list iff pairs were dropped or the list outgrew the compact array.  grid (ceil(m / 256))
__global__ __launch_bounds__(256) void gdecode_kernel(const int* __restrict__ list, const int* __restrict__ count,
                                                     const unsigned long long* __restrict__ keys,
                                                     float* __restrict__ vals, int64_t* __restrict__ inds, int m, int cap,
                                                     const int* __restrict__ overflow, const int* __restrict__ flag,
                                                     const int* __restrict__ cflag, int* __restrict__ count_fb) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int cnt = *count < m ? *count : m;
  if (p == 0) *count_fb = (*overflow != 0 || cnt > cap || (flag[0] | cflag[0]) != 0) ? cnt : 0;
  if (p >= cnt) return;
  const int i = list[p];
  const unsigned long long key = keys[i];
  if (key == 0ull) return;  // (beyond the compact array: the fallback's)
  store_keyed_best(key, i, vals, inds);
}

// the end of both candidate routes -- the centroids and the listed points as rows, the exact value of every pair,
// labels from the keys, then the exact kernel over what the pairs could not settle (normally zero points: pair
// lists that overflowed, more listed points than the row copies hold, or a flagged problem).  L: the route's
// workspace layout; cap_fb: points the fallback's compact copy holds.
template <class Layout>
static int run_pair_tail(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n, int euclid,
                         char* ws, const Layout& L, const int* flag, const int* cflag, int cap_fb, hipStream_t st) {
  const int* list1 = reinterpret_cast<const int*>(ws + L.list1_off);
  const int* count1 = reinterpret_cast<const int*>(ws + L.count1_off);
  const int* n_pairs = reinterpret_cast<const int*>(ws + L.npairs_off);
  const int* oflag = reinterpret_cast<const int*>(ws + L.oflag_off);
  int* count_fb = reinterpret_cast<int*>(ws + L.countfb_off);
  const uint2* pairs = reinterpret_cast<const uint2*>(ws + L.pairs_off);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + L.keys_off);
  float* Ac = reinterpret_cast<float*>(ws + L.ac_off);
  float* Bt = reinterpret_cast<float*>(ws + L.bt_off);
  float* Xt = reinterpret_cast<float*>(ws + L.xt_off);
  hipLaunchKernelGGL(rows_kernel, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, st, B, (int64_t)n,
                     static_cast<const int*>(nullptr), static_cast<const int*>(nullptr), n, Bt, d, L.dp);
  TPQ_LAUNCH_CHECK("lloyd rows_kernel");
  hipLaunchKernelGGL(rows_kernel, dim3((unsigned)(L.cap2 / 32)), dim3(64), 0, st, A, m, list1, count1, L.cap2, Xt, d, L.dp);
  TPQ_LAUNCH_CHECK("lloyd rows_kernel");
  hipLaunchKernelGGL(pair_exact_kernel, dim3(2048), dim3(256), 0, st, Xt, Bt, pairs, n_pairs, L.pair_cap, list1, keys,
                     L.dp, euclid);
  TPQ_LAUNCH_CHECK("lloyd pair_exact_kernel");
  hipLaunchKernelGGL(gdecode_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, list1, count1, keys, vals, inds,
                     (int)m, L.cap2, oflag, flag, cflag, count_fb);
  TPQ_LAUNCH_CHECK("lloyd gdecode_kernel");
  return launch_max_sim_list(A, B, vals, inds, 1, d, (int)m, n, euclid, list1, count_fb, keys, Ac, cap_fb, st);
}

struct WideLayout {
  int KS, KAp, U, ncb, ysplit, cap2, cap3, pair_cap;
  int64_t T;
  size_t mu_off, scale_off, flag_off, maxbits_off, cmax_off, cflag_off, count1_off, countfb_off, npairs_off, oflag_off,
      phi_off, norms_off, c1_off, cnorm_off, p2_off, thr_off, pairs_off, partb_off, parti_off, list1_off, keys_off, ac_off,
      bt_off, xt_off, total;
  int dp;
};
static WideLayout wide_layout(int d, int64_t m, int n) {
  WideLayout L;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  L.KS = (d + 15) / 16;
  L.KAp = (L.KS + kGK - 1) / kGK * kGK;
  L.ncb = (n + 255) / 256;
  L.U = L.ncb * 8;
  L.T = (m + 255) / 256 * 8;  // whole blocks of 256 points
  L.ysplit = L.ncb >= 8 ? 8 : (L.ncb >= 4 ? 4 : (L.ncb >= 2 ? 2 : 1));  // (gemm_kernel's block mapping)
  if (const char* e = TPQ_AB_ENV("TPQ_WIDE_YSPLIT")) L.ysplit = atoi(e);  // (A/B; 1, 2, 4, 8)
  L.cap2 = (int)(((m / 2 > 8192 ? m / 2 : 8192) + 255) / 256 * 256);     // pass 2's compact array, in points
  if (L.cap2 > L.T * 32) L.cap2 = (int)(L.T * 32);
  L.pair_cap = 4 * L.cap2 > 65536 ? 4 * L.cap2 : 65536;
  L.cap3 = (int)((m / 16 + 127) / 128 * 128);  // the fallback's compact copy
  if (L.cap3 < 128) L.cap3 = 128;
  L.mu_off = 0;
  L.scale_off = up((size_t)(d > 128 ? d : 128) * 4);
  L.flag_off = L.scale_off + 4;
  L.maxbits_off = L.flag_off + 4;
  L.cmax_off = L.maxbits_off + 4;
  L.cflag_off = L.cmax_off + 12;
  L.count1_off = L.cflag_off + 4;
  L.countfb_off = L.count1_off + 4;
  L.npairs_off = L.countfb_off + 4;
  L.oflag_off = L.npairs_off + 4;
  L.phi_off = up(L.oflag_off + 4);
  L.norms_off = up(L.phi_off + (size_t)L.T * L.KAp * 1024);
  L.c1_off = up(L.norms_off + (size_t)L.T * 32 * 16);
  L.cnorm_off = up(L.c1_off + (size_t)L.U * L.KAp * 1024);
  L.p2_off = up(L.cnorm_off + (size_t)L.U * 1024);
  L.thr_off = up(L.p2_off + (size_t)(L.cap2 / 32) * L.KAp * 1024);
  L.pairs_off = up(L.thr_off + (size_t)L.cap2 * 4);
  L.partb_off = up(L.pairs_off + (size_t)L.pair_cap * 8);
  L.parti_off = up(L.partb_off + (size_t)2 * L.ysplit * (size_t)(L.T * 32) * 8);
  L.list1_off = up(L.parti_off + (size_t)2 * L.ysplit * (size_t)(L.T * 32) * 4);
  L.keys_off = up(L.list1_off + (size_t)m * 4);
  L.ac_off = up(L.keys_off + (size_t)m * 8);
  L.dp = (d + 15) / 16 * 16;
  L.bt_off = up(L.ac_off + (size_t)d * L.cap3 * 4);            // [n][dp] f32: the centroids as rows
  L.xt_off = up(L.bt_off + (size_t)n * L.dp * 4);              // [cap2][dp] f32: the listed points as rows
  L.total = up(L.xt_off + (size_t)L.cap2 * L.dp * 4);
  return L;
}

// blocks of gemm_kernel: whole groups of 8 XCDs x 32 blocks (P point blocks x ysplit ranges each)
static unsigned gemm_grid(int pblocks, int ysplit) {
  const int per_group = 8 * (32 / ysplit);
  return (unsigned)((pblocks + per_group - 1) / per_group) * 256u;
}

static int run_wide(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n, int euclid,
                    char* ws, const WideLayout& L, hipStream_t st) {
  float* mu = reinterpret_cast<float*>(ws + L.mu_off);
  float* scale = reinterpret_cast<float*>(ws + L.scale_off);
  int* flag = reinterpret_cast<int*>(ws + L.flag_off);
  unsigned* maxbits = reinterpret_cast<unsigned*>(ws + L.maxbits_off);
  unsigned* cmax = reinterpret_cast<unsigned*>(ws + L.cmax_off);
  int* cflag = reinterpret_cast<int*>(ws + L.cflag_off);
  int* count1 = reinterpret_cast<int*>(ws + L.count1_off);
  int* n_pairs = reinterpret_cast<int*>(ws + L.npairs_off);
  int* oflag = reinterpret_cast<int*>(ws + L.oflag_off);
  u32x4* phi = reinterpret_cast<u32x4*>(ws + L.phi_off);
  float4* norms = reinterpret_cast<float4*>(ws + L.norms_off);
  u32x4* c1 = reinterpret_cast<u32x4*>(ws + L.c1_off);
  u32x4* cnorm = reinterpret_cast<u32x4*>(ws + L.cnorm_off);
  u32x4* p2 = reinterpret_cast<u32x4*>(ws + L.p2_off);
  float* thr = reinterpret_cast<float*>(ws + L.thr_off);
  uint2* pairs = reinterpret_cast<uint2*>(ws + L.pairs_off);
  float2* part_b = reinterpret_cast<float2*>(ws + L.partb_off);
  int* part_i = reinterpret_cast<int*>(ws + L.parti_off);
  int* list1 = reinterpret_cast<int*>(ws + L.list1_off);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + L.keys_off);
  int rc = check_hip(hipMemsetAsync(ws, 0, L.phi_off, st), "coarse_assign (wide) memset");
  if (rc) return rc;
  rc = check_hip(hipMemsetAsync(keys, 0, (size_t)m * 8, st), "coarse_assign (wide) keys memset");
  if (rc) return rc;
  // (rows beyond m / beyond the list in the last block of 256: an MFMA column depends on its own point only,
  // and those columns are never written out)
  // (inner products are not shift invariant: mu stays 0)
  rc = launch_scale({A, m, B, n, 1, d, 8192, 1, 0, euclid != 0, mu, maxbits, flag, scale}, st);
  if (rc) return rc;
  hipLaunchKernelGGL(gsplit_points_kernel, dim3((unsigned)((L.T + 3) / 4)), dim3(256), 0, st, A, mu, scale, phi, norms,
                     d, m, L.T, L.KAp);
  TPQ_LAUNCH_CHECK("lloyd gsplit_points_kernel");
  hipLaunchKernelGGL(gprep_centroids_kernel, dim3(L.U), dim3(64), 0, st, B, mu, scale, c1, cnorm, cmax, cflag, d, n,
                     L.KAp, euclid);
  TPQ_LAUNCH_CHECK("lloyd gprep_centroids_kernel");
  const size_t lds = (size_t)2 * kGStage + 8 * 1024 + sizeof(PairList);
  static const int tile_ct = TPQ_AB_ENV("TPQ_WIDE_CT") ? atoi(TPQ_AB_ENV("TPQ_WIDE_CT")) : 2;  // (A/B of the wave tile)
  const auto k_top2 = tile_ct == 4 ? gemm_kernel<false, 4> : gemm_kernel<false, 2>;
  const auto k_cand = tile_ct == 4 ? gemm_kernel<true, 4> : gemm_kernel<true, 2>;
  const int gemm_threads = tile_ct == 4 ? 256 : 512;
  const int64_t rows1 = L.T * 32;
  // (gdecide_kernel's comment) accumulation, N, shift rounding, 6-bit keys
  const float eps = 1.001f * (float)(17 * (L.KS + 1) + 8) / 16777216.0f + 1.0f / 8388608.0f + 1.0f / 4194304.0f +
                    1.0f / 131072.0f;
  {  // pass 1
    const int pblocks = (int)(L.T / 8);
    GemmArgs ga{c1, phi, cnorm, part_b, part_i, L.KAp, L.ncb, L.ysplit, pblocks, rows1, nullptr, nullptr, nullptr, nullptr,
                0, nullptr, n};
    rc = launch_with_lds(k_top2, "lloyd gemm_kernel", dim3(gemm_grid(pblocks, L.ysplit)), dim3(gemm_threads), lds, st, ga);
    if (rc) return rc;
    // (ranges of ceil(ncb / ysplit) centroid blocks: the last ones may be empty and write nothing)
    const int cb_per = (L.ncb + L.ysplit - 1) / L.ysplit, yused = (L.ncb + cb_per - 1) / cb_per;
    GDecideArgs da{part_b, part_i, 2 * yused, rows1, norms, cmax, scale, flag, cflag, inds, vals, list1, count1,
                   thr, L.cap2, (int)m, eps, (float)(d + 4) / 16777216.0f, sqrtf((float)d) / 8192.0f, euclid};
    hipLaunchKernelGGL(gdecide_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, da);
    TPQ_LAUNCH_CHECK("lloyd gdecide_kernel");
  }
  {  // pass 2: the candidates of the undecided points
    hipLaunchKernelGGL(ggather_kernel, dim3((unsigned)(L.cap2 / 32)), dim3(64), 0, st, phi, list1, count1, p2, L.KAp,
                       L.cap2);
    TPQ_LAUNCH_CHECK("lloyd ggather_kernel");
    GemmArgs ga{c1, p2, cnorm, nullptr, nullptr, L.KAp, L.ncb, L.ysplit, L.cap2 / 256, (int64_t)L.cap2, count1, thr, pairs,
                n_pairs, L.pair_cap, oflag, n};
    rc = launch_with_lds(k_cand, "lloyd gemm_kernel (candidates)", dim3(gemm_grid(L.cap2 / 256, L.ysplit)),
                         dim3(gemm_threads), lds, st, ga);
    if (rc) return rc;
  }
  // pass 3: exact values of the pairs
  return run_pair_tail(A, B, vals, inds, d, m, n, euclid, ws, L, flag, cflag, L.cap3, st);
}

// ---- many centroids: tpq_coarse_assign through the cascade (one problem, d <= 128) --------------------
// The centroids in chunks of 256 = blockIdx.y of ONE launch per level (a chunk's blocks alone fill half
// the chip); a chunk's (best, second, in-chunk index) of every point goes to part_*, decide_kernel folds
// the chunks and decides.  Level 1 = coarse_kernel over the points' hi pieces, level 2 = refine_kernel
// over the undecided points, level 3 = the exact kernel over what is left (compact copy + centroid
// splits, as in assign_fast.hip).  16 GB of piece streaming at 1 M x 16 384 x 128 instead of the
// three-product sweep of assign_fast_kernel.
struct AssignLayout {
  PrepLayout P;
  int KS, chunks, cap;
  size_t prep_off, frags_off, cmax_off, cflag_off, count1_off, count2_off, partb_off, parti_off, list1_off, list2_off,
      keys_off, ac_off, total;
  // candidate route (chunked problems): thresholds, pairs, row copies
  int cap2, pair_cap, dp;
  size_t npairs_off, oflag_off, countfb_off, thr_off, pairs_off, bt_off, xt_off;
};
static AssignLayout assign_layout(int d, int64_t m, int n) {
  AssignLayout L;
  L.P = prep_layout(1, d, m);
  L.KS = L.P.KS;
  L.chunks = (n + 255) / 256;
  L.cap = (int)((m / 4 + 127) / 128 * 128);
  if (L.cap < 128) L.cap = 128;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  L.prep_off = 0;
  L.frags_off = up(L.P.total);
  L.cmax_off = up(L.frags_off + (size_t)L.chunks * 8 * (2 * L.KS + 1) * 1024);
  L.cflag_off = L.cmax_off + 4 * kCm;
  L.count1_off = L.cflag_off + 4;
  L.count2_off = L.count1_off + 4;
  L.npairs_off = L.count2_off + 4;
  L.oflag_off = L.npairs_off + 4;
  L.countfb_off = L.oflag_off + 4;
  L.partb_off = up(L.countfb_off + 4);                              // [chunks][m] float2
  L.parti_off = up(L.partb_off + (size_t)L.chunks * m * 8);         // [chunks][m] u8
  L.list1_off = up(L.parti_off + (size_t)L.chunks * m);
  L.list2_off = up(L.list1_off + (size_t)m * 4);
  L.keys_off = up(L.list2_off + (size_t)m * 4);        // [m] u64 (level 3: zeroed)
  L.ac_off = up(L.keys_off + (size_t)m * 8);           // [d][cap] f32
  L.total = up(L.ac_off + (size_t)d * L.cap * 4);
  // candidate route: the listed points' thresholds and row copies (a quarter of the points), the pairs, the
  // centroids as rows
  L.cap2 = (int)(((m / 4 > 8192 ? m / 4 : 8192) + 511) / 512 * 512);
  if ((int64_t)L.cap2 > (m + 511) / 512 * 512) L.cap2 = (int)((m + 511) / 512 * 512);
  L.pair_cap = 4 * L.cap2 > 65536 ? 4 * L.cap2 : 65536;
  L.dp = (d + 15) / 16 * 16;
  L.thr_off = L.total;
  L.pairs_off = up(L.thr_off + (size_t)L.cap2 * 4);
  L.bt_off = up(L.pairs_off + (size_t)L.pair_cap * 8);
  L.xt_off = up(L.bt_off + (size_t)n * L.dp * 4);
  L.total = up(L.xt_off + (size_t)L.cap2 * L.dp * 4);
  return L;
}

// ---- the candidate route of the narrow path (d <= 128, many centroids) ---------------------------------------
// Level 1 of a chunked problem leaves 3-10 % of the points undecided.  Levels 2 and 3 (refine_stream_kernel:
// three products against every chunk; then the exact kernel over ALL centroids for what is left) cost 0.8 +
// 1.8 of the 7.4 ms at 1 M x 16 384 x 128.  Instead: the listed points' hi pieces stay in registers (64 points
// per wave: two column tiles share every centroid fragment), the hi fragments and -N of all chunks stream
// through a double-buffered LDS ring, and every value at or above the point's threshold (level 1's best key
// minus twice ITS bound, decide_kernel) is a candidate pair for pair_exact_kernel.  One product, no top-2.
struct CandStreamArgs {
  const u32x4* hi;       // [T][Q][32][64 B] (the points' hi pieces, prep layout)
  const u32x4* frags;    // [units][2 KS + 1][64]
  const int* list_in;
  const int* count_in;
  const float* thr;      // [cap]
  int cap;               // listed positions handled here: < min(count, cap)
  int n_half;            // half chunks (4 units each)
  int n;                 // centroids (units beyond are padding)
  int64_t T;
};
constexpr int kCandPoints = kWaves * 64;  // listed positions per block

template <int KS>
__global__ __launch_bounds__(kWaves * 64) void cand_stream_kernel(CandStreamArgs c, GemmArgs ga) {
  constexpr int FPU = 2 * KS + 1, FL = KS + 1, HB = 4 * FL * 1024, Q = (KS + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 half chunks (-N + hi fragments), PairList
  int cnt = *c.count_in;
  cnt = cnt < c.cap ? cnt : c.cap;
  if ((int64_t)blockIdx.x * kCandPoints >= cnt) return;  // block-uniform
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  PairList* pl = reinterpret_cast<PairList*>(smem + 2 * HB);
  if (threadIdx.x == 0) pl->n = 0;
  auto stage = [&](int h) {  // half chunk h -> buffer h & 1: per unit -N, then the hi piece of every k-step
    const char* src = reinterpret_cast<const char*>(c.frags) + (size_t)h * 4 * FPU * 1024;
    char* dst = smem + (h & 1) * HB;
    for (int f = wave; f < 4 * FL; f += kWaves) {
      const int unit = f / FL, j = f % FL;
      const int sf = unit * FPU + (j ? 2 * j - 1 : 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + sf * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(dst + f * 1024), 16, 0, 0);
    }
  };
  stage(0);
  const int64_t slice = c.T * Q * 2048;
  const __amdgpu_buffer_rsrc_t rs_hi = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(c.hi)), 0, (int)slice, 0x00020000);
  f16x8 xs[KS][2];
  float thr[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int64_t pos = (int64_t)blockIdx.x * kCandPoints + wave * 64 + ct * 32 + l31;
    const int p = pos < cnt ? c.list_in[pos] : -1;
    thr[ct] = p >= 0 ? c.thr[pos] : __builtin_nanf("");  // (NaN: no value compares >= it, not even an inf)
    const int voff = p >= 0 ? (p >> 5) * (Q * 2048) + (p & 31) * 64 + half * 16 : 0x7ffffff0;
    static_for<0, KS>([&](auto s_c) {
      constexpr int st = decltype(s_c)::value;
      xs[st][ct] = __builtin_bit_cast(
          f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_hi, voff, (st >> 1) * 2048 + (st & 1) * 32, 0));
    });
  }
  const bf16x8 bones = ones3_bf16x8(half);  // B fragment of ones at k = 0, 1, 2
  const f32x16 zero = zero_f32x16();
#pragma unroll 1
  for (int h = 0; h < c.n_half; ++h) {
    __syncthreads();  // half chunk h has landed (vmcnt(0) + barrier); everyone is done with the other buffer
    if (h + 1 < c.n_half) stage(h + 1);
    // (pairs are appended in every stage, so pl->n is not stable anywhere: the decision to flush is an OR over
    // the block, taken every eighth stage -- ~70 appends per block in between against 2 048 spare entries)
    if ((h & 7) == 7 && __syncthreads_or(pl->n >= kPairList / 2)) flush_pairs(ga, pl, blockIdx.x * (unsigned)kCandPoints);
    const u32x4* base = reinterpret_cast<const u32x4*>(smem + (h & 1) * HB) + lane;
#pragma unroll
    for (int U = 0; U < 4; ++U) {
      const u32x4* up = base + U * FL * 64;
      f32x16 acc[2] = {zero, zero};
      static_for<0, KS>([&](auto s_c) {
        constexpr int st = decltype(s_c)::value;
        const f16x8 cf = __builtin_bit_cast(f16x8, up[(1 + st) * 64]);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cf, xs[st][0], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cf, xs[st][1], acc[1], 0, 0, 0);
      });
      const bf16x8 nf = __builtin_bit_cast(bf16x8, up[0]);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(nf, bones, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(nf, bones, acc[1], 0, 0, 0);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        float mx = acc[ct][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[ct][r]);
        if (__ballot(mx >= thr[ct]) == 0ull) continue;  // (nearly every tile)
        const unsigned rowbits = (unsigned)(wave * 64 + ct * 32 + l31) << 22;
        const int cbase = (4 * h + U) * 32 + 4 * half;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cen = cbase + (r & 3) + 8 * (r >> 2);
          const bool hit = acc[ct][r] >= thr[ct] && cen < c.n;
          const unsigned long long mk = __ballot(hit);
          if (mk) {
            const int leader = __ffsll((long long)mk) - 1;
            int b0 = 0;
            if (lane == leader) b0 = atomicAdd(&pl->n, __popcll(mk));  // LDS
            b0 = __shfl(b0, leader, 64);
            const int slot = b0 + __popcll(mk & ((1ull << lane) - 1ull));
            if (hit && slot < kPairList) pl->item[slot] = rowbits | (unsigned)cen;
          }
        }
      }
    }
  }
  __syncthreads();
  flush_pairs(ga, pl, blockIdx.x * (unsigned)kCandPoints);
}

static int run_cand_tail(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n, char* ws,
                         const AssignLayout& L, hipStream_t st) {
  CandStreamArgs ca{reinterpret_cast<const u32x4*>(ws + L.prep_off + L.P.hi_off),
                    reinterpret_cast<const u32x4*>(ws + L.frags_off),
                    reinterpret_cast<const int*>(ws + L.list1_off), reinterpret_cast<const int*>(ws + L.count1_off),
                    reinterpret_cast<const float*>(ws + L.thr_off), L.cap2, 2 * L.chunks, n, L.P.T};
  GemmArgs ga{};
  ga.pairs = reinterpret_cast<uint2*>(ws + L.pairs_off);
  ga.pair_count = reinterpret_cast<int*>(ws + L.npairs_off);
  ga.pair_cap = L.pair_cap;
  ga.overflow = reinterpret_cast<int*>(ws + L.oflag_off);
  int rc = dispatch_ks<8>(L.KS, [&](auto ks) -> int {
    constexpr int K = decltype(ks)::value;
    return launch_with_lds(cand_stream_kernel<K>, "lloyd cand_stream_kernel", dim3((unsigned)(L.cap2 / kCandPoints)),
                           dim3(kWaves * 64), (size_t)2 * 4 * (K + 1) * 1024 + sizeof(PairList), st, ca, ga);
  });
  if (rc) return rc;
  return run_pair_tail(A, B, vals, inds, d, m, n, 1, ws, L, reinterpret_cast<const int*>(ws + L.prep_off + L.P.flag_off),
                       reinterpret_cast<const int*>(ws + L.cflag_off), L.cap, st);
}

// Chunked problems: the undecided points do not go through levels 2 and 3 -- their CANDIDATES (the centroids
// within twice level 1's bound of the best: ~2 per point) get the exact kernel's value (run_cand_tail), and the points
// with an exact step are counted in count1, not count2.  TPQ_COARSE_ASSIGN_CAND=0: levels 2 and 3 (A/B)
static bool assign_takes_cand_route(const AssignLayout& L, int n) {
  static const bool enabled = !(TPQ_AB_ENV("TPQ_COARSE_ASSIGN_CAND") && atoi(TPQ_AB_ENV("TPQ_COARSE_ASSIGN_CAND")) == 0);
  return enabled && L.chunks > 1 && n <= (1 << 22);  // (a pair entry carries the centroid in 22 bits)
}

static int run_assign(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n, char* ws,
                      const AssignLayout& L, hipStream_t st) {
  const PrepLayout& P = L.P;
  const int KS = L.KS;
  char* p = ws + L.prep_off;
  float* mu = reinterpret_cast<float*>(p + P.mu_off);
  float* scale = reinterpret_cast<float*>(p + P.scale_off);
  int* flag = reinterpret_cast<int*>(p + P.flag_off);
  unsigned* maxbits = reinterpret_cast<unsigned*>(p + P.maxbits_off);
  u32x4* frags = reinterpret_cast<u32x4*>(ws + L.frags_off);
  unsigned* cmax = reinterpret_cast<unsigned*>(ws + L.cmax_off);
  int* cflag = reinterpret_cast<int*>(ws + L.cflag_off);
  int* count1 = reinterpret_cast<int*>(ws + L.count1_off);
  int* count2 = reinterpret_cast<int*>(ws + L.count2_off);
  float2* part_b = reinterpret_cast<float2*>(ws + L.partb_off);
  uint8_t* part_i = reinterpret_cast<uint8_t*>(ws + L.parti_off);
  int* list1 = reinterpret_cast<int*>(ws + L.list1_off);
  int* list2 = reinterpret_cast<int*>(ws + L.list2_off);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + L.keys_off);
  float* Ac = reinterpret_cast<float*>(ws + L.ac_off);
  int rc = check_hip(hipMemsetAsync(p + P.mu_off, 0, P.total - P.mu_off, st), "coarse_assign memset");
  if (rc) return rc;
  rc = check_hip(hipMemsetAsync(ws + L.cmax_off, 0, L.partb_off - L.cmax_off, st), "coarse_assign memset");
  if (rc) return rc;
  rc = check_hip(hipMemsetAsync(keys, 0, (size_t)m * 8, st), "coarse_assign keys memset");
  if (rc) return rc;
  // prepare the points (per call: the points change from call to call, the centroids are the codebook)
  rc = launch_scale({A, m, B, n, 1, d, 4096, 1, 0, true, mu, maxbits, flag, scale}, st);
  if (rc) return rc;
  rc = launch_split(A, p, P, 1, d, m, st);
  if (rc) return rc;
  rc = launch_cprep(B, mu, scale, frags, cmax, cflag, 1, d, n, L.chunks, KS, st);
  if (rc) return rc;
  const bool chunked = L.chunks > 1;
  const int chunk_stride = 8 * (2 * KS + 1) * 64;  // 16-byte units
  StepArgs sa{reinterpret_cast<const u32x4*>(p + P.hi_off), reinterpret_cast<const u32x4*>(p + P.mid_off),
              reinterpret_cast<const float2*>(p + P.norms_off), frags, cmax, scale, flag, cflag, inds, vals,
              nullptr, nullptr, list1, count1, (int)m, P.T,
              level_eps(KS, d, 1), (float)(d + 4) / 16777216.0f, sqrtf((float)d) / 8192.0f, 1, nullptr, 0,
              chunked ? part_b : nullptr, chunked ? part_i : nullptr, chunk_stride};
  rc = launch_coarse(KS, sa, L.chunks, st);
  if (rc) return rc;
  if (chunked) {
    const bool cand = assign_takes_cand_route(L, n);
    if (cand) {
      sa.thr = reinterpret_cast<float*>(ws + L.thr_off);
      sa.thr_cap = L.cap2;
    }
    rc = launch_decide_level1(sa, L.chunks, st);
    if (rc) return rc;
    if (cand) return run_cand_tail(A, B, vals, inds, d, m, n, ws, L, st);
  }
  sa.eps = level_eps(KS, d, 2);
  sa.level = 2;
  sa.list_in = list1;
  sa.count_in = count1;
  sa.list = list2;
  sa.count = count2;
  if (chunked) {  // the points stay in registers, the chunks stream
    sa.part_b = nullptr;
    sa.part_i = nullptr;
    rc = launch_refine_stream(KS, sa, 2 * L.chunks, st);
  } else {
    rc = launch_refine(KS, sa, 1, st);
  }
  if (rc) return rc;
  return launch_max_sim_list(A, B, vals, inds, 1, d, (int)m, n, 1, list2, count2, keys, Ac, L.cap, st);
}

}  // namespace lloyd

int lloyd_assign_supported(int d, int64_t m, int n, int route) {
  if (!(d >= 1 && d <= 128 && n >= 1 && n <= (1 << 24) && m >= 1 && m < (1LL << 31))) return 0;
  if (TPQ_AB_ENV("TPQ_COARSE_ASSIGN_OLD")) return 0;  // (A/B: the two-piece bf16 selection of assign_fast.hip)
  // below ~4 096 centroids the per-call preparation (max-abs + split of the points, the fold of the
  // chunks) costs more than the lighter sweep saves: 128 x 2 048: 1.66 vs 1.48 ms, 128 x 4 096: 2.37 vs 2.76,
  // 128 x 16 384: 8.5 vs 11.0, 64 x 16 384: 4.7 vs 6.0, 128 x 65 536: 39.9 vs 47.4 (1 M points)
  // (route == TPQ_ASSIGN_ROUTE_CASCADE: the caller asks for the cascade whatever the size -- tests, tuning)
  if (route != TPQ_ASSIGN_ROUTE_CASCADE && n < 4096) return 0;
  const lloyd::PrepLayout P = lloyd::prep_layout(1, d, m);
  return (P.T * ((P.KS + 1) / 2) * 2048 <= 0x7fffffffLL && (int64_t)d * m * 4 <= 0x7fffffffLL) ? 1 : 0;
}
// 128 < d <= 1024: the GEMM-shaped cascade (euclidean)
int lloyd_wide_supported(int d, int64_t m, int n) {
  return (d > 128 && d <= 1024 && n >= 1 && n <= (1 << 22) && m >= 1 && m < (1LL << 28)) ? 1 : 0;
}
size_t lloyd_assign_workspace_bytes(int d, int64_t m, int n) {
  return d > 128 ? lloyd::wide_layout(d, m, n).total : lloyd::assign_layout(d, m, n).total;
}
size_t lloyd_assign_count_offset(int d, int64_t m, int n) {  // wide: the points with an exact step (candidates)
  if (d > 128) return lloyd::wide_layout(d, m, n).count1_off;
  const lloyd::AssignLayout L = lloyd::assign_layout(d, m, n);
  // (chunked problems on the candidate route: the points that got an exact step on their candidates)
  return lloyd::assign_takes_cand_route(L, n) ? L.count1_off : L.count2_off;
}
int lloyd_assign(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n, int euclid,
                 char* ws, hipStream_t st) {
  if (d > 128) return lloyd::run_wide(A, B, vals, inds, d, m, n, euclid, ws, lloyd::wide_layout(d, m, n), st);
  return lloyd::run_assign(A, B, vals, inds, d, m, n, ws, lloyd::assign_layout(d, m, n), st);
}
}  // namespace tpq
