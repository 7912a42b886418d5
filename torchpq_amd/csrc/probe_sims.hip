// The coarse step of search() on the fp16 matrix cores (probe_fast.h; called from coarse_probe.hip), at many cells
// (IVF4096 / IVF16384 of the reference's benchmark grid), where the fp32-MFMA similarity GEMM (75 TF/s) was 40-85 % of a
// search: fast similarities of every (query, cell) pair on data prepared as the fp16 cascade prepares it
// (fp16_cascade.h; the centroids' preparation runs the shared kernels of cascade_core.hip), then a row select on them
// that re-evaluates its candidates in fp32.
#include "fp16_cascade.h"
#include "probe_fast.h"

namespace tpq {

// What the fast pass leaves in the workspace (and the prepared block) for the select kernel.
struct ProbeFastBuffers {
  const _Float16* sims;  // [nq][n_cells] fast values f' = 2 a'.c' - |c'|^2 (centred, scaled: per query a monotone image of
                         // the similarity), stored as fp16 of f' x qscale[q]
  const float* gmax;     // [nq][n_groups] maxima of the unrounded f' over groups of 2^gshift cells (fp32, not scaled)
  const float* band;     // [nq] 2 delta' x qscale: the candidate band in STORED units before the rounding of the stored
                         // values (which the select kernel adds); +inf: the query is evaluated exactly
  const float* qscale;   // [nq] power of two
  const float* xt;       // [nq][xt_stride] the queries as rows (fp32, as given)
  const float* q2;       // [nq] |x|^2 as the exact kernels sum it (fma chain over ascending k)
  int xt_stride;         // multiple of 4
  const float* ct;    // [n_cells][d] the centroids as rows
  const float* c2;    // [n_cells] |C|^2, ascending-k fma chain
  int n_groups;
  int gshift;            // log2 of the cells per group (5 or 7)
};

namespace lloyd {

// ---- the coarse step of search(): fast similarities of every (query, cell) pair (probe_fast.h) ---------------
// coarse_kernel's loop -- hi pieces only, one product per k-step, the -N MFMA, two column tiles per A operand,
// the chunk's fragments staged once per block by LDS-DMA -- with another epilogue: instead of the top-2 update (2.5
// VALU instructions per value, what bounds level 1) the 16 values a lane holds of its query are stored as four
// 16-byte pieces of the query's row (rows 8 g + 4 half + j of a 32 x 32 tile are four consecutive cells), and the
// maximum over each 128-cell group is kept for the row select's group filter.  grid (query blocks, 256-cell chunks);
// a block walks n_wide wide tiles per wave (small query batches: one, so that 10 000 queries x 64 chunks are 1 280 blocks).
// (see the epilogue of probe_sims_kernel)
#define TPQ_STORE_PAD() asm volatile("s_nop 7" ::: "memory")

struct ProbeSimsArgs {
  const u32x4* hi;
  const u32x4* frags;
  _Float16* sims;        // [nq][n_cells] f' x qscale[q], fp16
  const float* qscale;   // [nq] the power of two that puts |f'| <= (|a'| + |c'|max)^2 of the query below 2^15
  float* gmax;           // [nq][n_groups] maxima of the UNROUNDED f' (fp32, unscaled)
  int nq, n_cells, n_groups, n_wide;
  int64_t T;
  int chunk_frag_stride;
};

template <int KS, int GSH>   // GSH: log2 of the cells per group of the maxima (5: one unit, 7: four)
__global__ __launch_bounds__(kWaves * 64, 2) void probe_sims_kernel(ProbeSimsArgs a) {
  constexpr int NG = 256 >> GSH;   // groups per 256-cell chunk
  constexpr int FPU = 2 * KS + 1;  // fragments per unit in global memory
  constexpr int FL = KS + 1;       // ... in LDS
  constexpr int Q = (KS + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int chunk = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  {
    const char* src = reinterpret_cast<const char*>(a.frags) + (size_t)chunk * a.chunk_frag_stride * 16;
    for (int f = wave; f < 8 * FL; f += kWaves) {
      const int unit = f / FL, j = f % FL;
      const int sf = unit * FPU + (j ? 2 * j - 1 : 0);  // -N, then the hi piece of k-step j - 1
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + sf * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(smem + f * 1024), 16, 0, 0);
    }
  }
  const int64_t slice = a.T * Q * 2048;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.hi)), 0, (int)slice, 0x00020000);
  const int n_wide = a.n_wide;
  auto wide_of = [&](int t) -> int64_t { return ((int64_t)blockIdx.x * n_wide + t) * kWaves + wave; };
  auto frag_voff = [&](int t) -> int {
    const int64_t wt = wide_of(t);
    return (t < n_wide && 2 * wt < a.T) ? (int)(2 * wt * Q * 2048) + l31 * 64 + half * 16 : 0x7ffffff0;
  };
  f16x8 xsb[2][2][KS];  // [buffer][column tile][k-step]
  auto load_frag = [&](int voff, auto e_c, f16x8 (&dst)[2][KS]) {
    constexpr int e = decltype(e_c)::value, ct = e / KS, st = e % KS;
    dst[ct][st] = __builtin_bit_cast(
        f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, ct * Q * 2048 + (st >> 1) * 2048 + (st & 1) * 32, 0));
  };
  {
    const int voff = frag_voff(0);
    static_for<0, 2 * KS>([&](auto e_c) { load_frag(voff, e_c, xsb[0]); });
  }
  __syncthreads();  // fragments (vmcnt(0) of the DMA) are in LDS
  const u32x4* fp = reinterpret_cast<const u32x4*>(smem) + lane;
  auto ldsf = [&](const u32x4* p) -> f16x8 { return __builtin_bit_cast(f16x8, *p); };
  f32x16 acc[2];
  f16x8 a0 = ldsf(fp + 1 * 64), a1 = a0, aring[3];
  if constexpr (KS > 1) a1 = ldsf(fp + 2 * 64);
  const bf16x8 bones = ones3_bf16x8(half);  // B fragment of ones at k = 0, 1, 2
  float gm[2][NG];  // [column tile][group of the chunk]
  // the sims rows of this block's queries as ONE buffer resource (base: the block's first query, the chunk's first
  // cell): a lane's stores are buffer_store_dwordx4 at a 32-bit offset -- its row, its half -- plus a compile-time
  // constant; rows beyond nq get an offset beyond the resource's range and are dropped by the hardware (64-bit
  // per-lane pointers and exec-mask predicates put this kernel 319 registers over its budget)
  const int64_t q_block0 = (int64_t)blockIdx.x * n_wide * kWaves * 64;
  const int64_t rows_here = (a.nq - q_block0) < (int64_t)n_wide * kWaves * 64 ? (a.nq - q_block0) : (int64_t)n_wide * kWaves * 64;
  const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(a.sims + q_block0 * a.n_cells + chunk * 256), 0,
      (int)(rows_here > 0 ? (rows_here - 1) * (int64_t)a.n_cells * 2 + (a.n_cells - chunk * 256) * 2 : 0), 0x00020000);
  float qs[2];     // the lane's query's scale, per column tile
  int svoff[2];    // byte offset of the lane's row (and half) of each column tile inside that resource
  const int units_here = (a.n_cells - chunk * 256 + 31) / 32;  // (n_cells % 32 == 0: whole units)

  auto unit = [&](auto u_c, int voff_next, const f16x8 (&xs)[2][KS], f16x8 (&xsn)[2][KS]) {
    constexpr int U = decltype(u_c)::value;
    const u32x4* up = fp + U * FL * 64;
    const u32x4* upn = fp + ((U + 1) & 7) * FL * 64;
    const f32x16 zero = zero_f32x16();
    const bf16x8 cfrag = __builtin_bit_cast(bf16x8, up[0]);
    if constexpr (U < 4) {
      constexpr int l0 = (U * 2 * KS) / 4, l1 = ((U + 1) * 2 * KS) / 4;
      static_for<l0, l1>([&](auto e_c) { load_frag(voff_next, e_c, xsn); });
    }
    static_for<0, KS>([&](auto s_c) {
      constexpr int st = decltype(s_c)::value;
      if constexpr (st + 2 < KS) aring[(st + 2) % 3] = ldsf(up + (1 + st + 2) * 64);
      if constexpr (st == 0) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, xs[0][0], zero, 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, xs[1][0], zero, 0, 0, 0);
        a0 = ldsf(upn + 1 * 64);
      } else if constexpr (st == 1) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, xs[0][1], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, xs[1][1], acc[1], 0, 0, 0);
        a1 = ldsf(upn + 2 * 64);
      } else {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aring[st % 3], xs[0][st], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aring[st % 3], xs[1][st], acc[1], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cfrag, bones, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cfrag, bones, acc[1], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (U < units_here) {  // wave-uniform (the last chunk of a cell count that is not a multiple of 256)
      typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
      u32x4 w[2][2];  // [column tile][pair of pieces]: eight consecutive cells of the lane's query, fp16
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        float mx = gm[ct][U >> (GSH - 5)];
        uint32_t pk[4][2];  // the lane's four pieces (cells 8 g + 4 half + 0..3) as fp16 pairs
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 v = {acc[ct][4 * g], acc[ct][4 * g + 1], acc[ct][4 * g + 2], acc[ct][4 * g + 3]};
          mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
          const f16x2 h0 = {(_Float16)(v[0] * qs[ct]), (_Float16)(v[1] * qs[ct])};
          const f16x2 h1 = {(_Float16)(v[2] * qs[ct]), (_Float16)(v[3] * qs[ct])};
          pk[g][0] = __builtin_bit_cast(uint32_t, h0);
          pk[g][1] = __builtin_bit_cast(uint32_t, h1);
        }
        gm[ct][U >> (GSH - 5)] = mx;
        // lanes l and l + 32 hold the two halves of the same eight cells of the same query: v_permlane32_swap gives the
        // lower lane both halves of piece 2 p and the upper lane both halves of piece 2 p + 1 -- 16-byte stores of eight
        // consecutive cells (as 8-byte stores the kernel is bound by the number of store instructions, not their bytes)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const auto s0 = __builtin_amdgcn_permlane32_swap(pk[2 * p][0], pk[2 * p + 1][0], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(pk[2 * p][1], pk[2 * p + 1][1], false, false);
          w[ct][p] = u32x4{s0[0], s1[0], s0[1], s1[1]};
        }
      }
      // The four stores last and back to back, then TPQ_STORE_PAD: on gfx950 a VALU instruction that overwrites a
      // register of a 16-byte store's data two instructions after the store (all the wait the compiler's hazard rule
      // asks for) reaches the register file before the store has read it -- measured here: with the stores in between
      // the conversions, 9 % of the rows held a later group maximum in the first dword of a piece
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          __builtin_amdgcn_raw_buffer_store_b128(w[ct][p], srsrc, svoff[ct], (U * 32 + 16 * p) * 2, 0);
      TPQ_STORE_PAD();
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  auto tile = [&](int t, auto cb_c) {
    constexpr int CB = decltype(cb_c)::value, NX = 1 - CB;
    const int voff_next = frag_voff(t + 1);
    const int64_t wt = wide_of(t);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int64_t qi = (2 * wt + ct) * 32 + l31;
      svoff[ct] = qi < a.nq ? (int)((qi - q_block0) * a.n_cells * 2) + half * 16 : 0x7ffffff0;
      qs[ct] = a.qscale[qi < a.nq ? qi : 0];
#pragma unroll
      for (int gg = 0; gg < NG; ++gg) gm[ct][gg] = -INFINITY;
    }
    static_for<0, 8>([&](auto u_c) { unit(u_c, voff_next, xsb[CB], xsb[NX]); });
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int64_t qi = (2 * wt + ct) * 32 + l31;
#pragma unroll
      for (int gg = 0; gg < NG; ++gg) {
        const float m2 = fmaxf(gm[ct][gg], __shfl_xor(gm[ct][gg], 32, 64));  // the two halves hold disjoint cells
        const int grp = chunk * NG + gg;
        if (half == 0 && qi < a.nq && grp < a.n_groups) a.gmax[qi * a.n_groups + grp] = m2;
      }
    }
  };
  using std::integral_constant;
#pragma unroll 1
  for (int t = 0; t < n_wide; t += 2) {
    if (2 * ((int64_t)blockIdx.x * n_wide + t) * kWaves >= a.T) break;
    tile(t, integral_constant<int, 0>{});
    if (t + 1 >= n_wide || 2 * ((int64_t)blockIdx.x * n_wide + t + 1) * kWaves >= a.T) break;
    tile(t + 1, integral_constant<int, 1>{});
  }
}

// What probe_split_kernel writes beside the pieces: the query as a ROW (the select kernel's exact step reads a
// query's d values; from the [d][nq] operand that is d cache lines per query), |x|^2 as the exact kernels sum it
// (fma chain over ascending k), and the query's candidate band and fp16 scale (probe_band).
struct ProbeSplitOut {
  float* xt;                   // [m][xt_stride] fp32 row copies
  float* q2;                   // [m] |x|^2
  float* band;                 // [m]
  float* qscale;               // [m]
  const unsigned* cmax2_bits;  // the prepared centroids' maxima (kCm words)
  const int* cflag;
  float eps, eps_exact, eta;
  int xt_stride;
};

// band[q] = 2 delta' of query q: emit()'s level-1 bound (the pieces this query and the worst centroid actually drop, the
// fp32 accumulation of the MFMA terms, the subnormal pieces, and the exact chain's own rounding), in f' units;
// +inf when the queries or the centroids do not fit the fp16 scale (the select then evaluates the query exactly)
__device__ __forceinline__ void probe_band(const ProbeSplitOut& po, float s, float n2c, float n2r, float n2m, float& band,
                                           float& qscale) {
  const float cn = sqrtf(__uint_as_float(po.cmax2_bits[0])), cnr = sqrtf(__uint_as_float(po.cmax2_bits[1]));
  const float c2 = sqrtf(__uint_as_float(po.cmax2_bits[2]));
  const float an = sqrtf(n2c), anr = sqrtf(n2r) * s;
  const float t1 = an + cn, t2 = anr + cnr * s;
  const float a2 = sqrtf(n2m);
  const float dropped = a2 * (2.002f * cn + c2) + 1.001f * an * c2;
  float delta = 1.26f * (dropped + po.eps * t1 * t1 + po.eta * (2.f * cn + an) + po.eps_exact * t2 * t2);
  if (po.cflag[0] != 0 || !(delta < 3.0e38f)) delta = INFINITY;  // (a query beyond the scale: n2c = inf -> delta = inf)
  // the fast values are STORED as fp16 of f' x 2^-e with |f'| <= (|a'| + |c'|max)^2 = t1^2 < 2^(e + 15): half the bytes
  // of the matrix the select reads (and the sims kernel's time is its write).  The rounding of the stored values is
  // the select kernel's to add to the band: it knows how large the values near the top of the row are
  float sc = 0.f;
  const float b = t1 * t1;
  if (delta < INFINITY && b > 0.f) {
    const int e = ilogbf(b) - 14;
    if (e > -100 && e < 100) sc = ldexpf(1.f, -e);
  }
  if (!(sc > 0.f)) {  // (all-zero or astronomically scaled data: evaluated exactly)
    sc = 1.f;
    if (b > 0.f) delta = INFINITY;
  }
  qscale = sc;
  band = 2.f * delta * sc;  // in STORED units
}

// split_kernel for a search batch.  There a lane walks all of its point's dimensions, 32 at a time: four dependent
// rounds of strided loads, and 10 000 queries are 40 blocks -- 16 us of latency on a mostly idle chip.  Here a block is
// 64 queries x 4 waves and WAVE w takes k-quarter w: one round of loads per wave, all in flight together.  The raw
// values also go to LDS, from which wave 0 sums |x|^2 as the exact kernels do (one fma chain over ascending k -- the
// one quantity here whose rounding is part of the result) and derives the band; |a'|^2 and |a' - ah|^2 only enter
// bounds and are summed per quarter.  No norms are written: nothing on the probe's path reads them.
__global__ __launch_bounds__(256) void probe_split_kernel(const float* __restrict__ A, const float* __restrict__ mu,
                                                         const float* __restrict__ scale, u32x4* __restrict__ hi,
                                                         u32x4* __restrict__ mid, int d, int64_t m, int64_t T, int KS,
                                                         ProbeSplitOut po) {
  __shared__ float xs[128 * 64];      // [k][query]
  __shared__ float part[4][2][64];    // per quarter: |a'|^2, |a' - ah|^2
  __shared__ int bad_s[4][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  const int64_t tile = i >> 5;
  const int l31 = (int)(i & 31);
  const bool iv = i < m;
  const int Q = (KS + 1) / 2;
  const float s = scale[0];
  if (w < Q) {
    const int q = w;
    const float* Ab = A + (iv ? i : 0);
    float x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int k = 32 * q + j;
      x[j] = (iv && k < d) ? Ab[(int64_t)k * m] : 0.f;
    }
    if (iv) {
      float4* xr = reinterpret_cast<float4*>(po.xt + i * po.xt_stride + 32 * q);
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (32 * q + 4 * c < po.xt_stride) xr[c] = make_float4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
    }
    float n2c = 0.f, n2m = 0.f;
    int bad = 0;
    const int64_t fo = ((tile * Q) + q) * 128 + l31 * 4;  // in 16-byte chunks
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f16x8 h, mm;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * q + 8 * c + j;
        const float xv = x[8 * c + j];
        xs[k * 64 + lane] = xv;
        const float a = (iv && k < d) ? (xv - mu[k]) * s : 0.f;
        bad |= !(fabsf(a) < 16384.f);
        const _Float16 hh = (_Float16)a;
        const float r = a - (float)hh;
        h[j] = hh;
        mm[j] = (_Float16)r;
        n2c = fmaf(a, a, n2c);
        n2m = fmaf(r, r, n2m);
      }
      if (tile < T) {
        hi[fo + c] = __builtin_bit_cast(u32x4, h);
        mid[fo + c] = __builtin_bit_cast(u32x4, mm);
      }
    }
    part[q][0][lane] = n2c;
    part[q][1][lane] = n2m;
    bad_s[q][lane] = bad;
  }
  __syncthreads();
  if (w == 0 && iv) {
    float n2r = 0.f, n2c = 0.f, n2m = 0.f;
    int bad = 0;
#pragma unroll 16
    for (int k = 0; k < 32 * Q; ++k) {
      const float xv = xs[k * 64 + lane];
      n2r = fmaf(xv, xv, n2r);
    }
    for (int q = 0; q < Q; ++q) {
      n2c += part[q][0][lane];
      n2m += part[q][1][lane];
      bad |= bad_s[q][lane];
    }
    // (the quarter sums round differently from one chain: a few ulps, under the bounds' own 1.001 factors)
    float band, qs;
    probe_band(po, s, bad ? INFINITY : n2c * 1.000001f, n2r, n2m * 1.000001f, band, qs);
    po.q2[i] = n2r;
    po.band[i] = band;
    po.qscale[i] = qs;
  }
}

// the centroids as rows, and |C|^2 as the exact kernels sum it (ascending k, fma)
__global__ __launch_bounds__(256) void probe_rows_kernel(const float* __restrict__ C, float* __restrict__ ct,
                                                        float* __restrict__ c2, int d, int n_cells) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8 threads
  float sq = 0.f;
  for (int k0 = 0; k0 < d; k0 += 32) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = k0 + ty + 8 * r, c = c0 + tx;
      tile[ty + 8 * r][tx] = (k < d && c < n_cells) ? C[(int64_t)k * n_cells + c] : 0.f;
    }
    __syncthreads();
    if (ty == 0) {  // (one thread per cell: the chain is sequential in k)
#pragma unroll
      for (int kk = 0; kk < 32; ++kk)
        if (k0 + kk < d) sq = fmaf(tile[kk][tx], tile[kk][tx], sq);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + ty + 8 * r, k = k0 + tx;
      if (c < n_cells && k < d) ct[(int64_t)c * d + k] = tile[tx][ty + 8 * r];
    }
    __syncthreads();
  }
  if (ty == 0 && c0 + tx < n_cells) c2[c0 + tx] = sq;
}

// Everything that depends on the centroids alone -- mean, scale (from the CENTROIDS' range, one bit of headroom: a
// query beyond it gets an infinite norm from split_kernel and is evaluated exactly), fp16 fragments, row copies, |C|^2
// -- is prepared once per codebook (tpq_ivfpq_coarse_probe_prepare) or, without a prepared block, per call.
struct ProbePrepared {
  int KS, chunks;
  size_t mu_off, scale_off, cflag_off, maxbits_off, cmax_off, frags_off, ct_off, c2_off, total;
};
static int probe_ks(int d) { return d <= 32 ? 2 : (d <= 64 ? 4 : 8); }
static ProbePrepared probe_prepared_layout(int d, int n_cells) {
  ProbePrepared L;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  L.KS = probe_ks(d);
  L.chunks = (n_cells + 255) / 256;
  L.mu_off = 0;
  L.scale_off = (size_t)kMu * 4;
  L.cflag_off = L.scale_off + 4;      // (also the "flag" of maxabs / scale: non-finite centroids)
  L.maxbits_off = L.cflag_off + 4;
  L.cmax_off = L.maxbits_off + 4;
  L.frags_off = up(L.cmax_off + 4 * kCm);
  L.ct_off = up(L.frags_off + (size_t)L.chunks * 8 * (2 * L.KS + 1) * 1024);
  L.c2_off = up(L.ct_off + (size_t)n_cells * d * 4);
  L.total = up(L.c2_off + (size_t)n_cells * 4);
  return L;
}
struct ProbeLayout {
  PrepLayout P;
  ProbePrepared C;
  int KS, n_groups, gshift;
  int xt_stride;
  size_t prep_off, flag_off, sims_off, gmax_off, band_off, qscale_off, q2_off, xt_off, prepared_off, total;
};
static int probe_gshift(int n_cells) { return n_cells <= 8192 ? 5 : (n_cells <= 16384 ? 6 : 7); }
static ProbeLayout probe_layout(int d, int nq, int n_cells) {
  ProbeLayout L;
  L.C = probe_prepared_layout(d, n_cells);
  L.KS = L.C.KS;
  L.P = prep_layout(1, 16 * L.KS, nq);
  // group maxima: of 32 cells up to 8 192 cells, of 64 up to 16 384 (<= 256 groups, which the select prefetches whole;
  // its direct list needs 2 n_probe <= groups), of 128 beyond
  L.gshift = probe_gshift(n_cells);
  L.n_groups = (n_cells + (1 << L.gshift) - 1) >> L.gshift;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  L.prep_off = 0;
  L.flag_off = up(L.P.total);
  L.sims_off = L.flag_off + 256;
  L.gmax_off = up(L.sims_off + (size_t)nq * n_cells * 2);
  L.band_off = up(L.gmax_off + (size_t)nq * L.n_groups * 4);
  L.qscale_off = up(L.band_off + (size_t)nq * 4);
  L.q2_off = up(L.qscale_off + (size_t)nq * 4);
  L.xt_stride = (d + 3) / 4 * 4;
  L.xt_off = up(L.q2_off + (size_t)nq * 4);
  L.prepared_off = up(L.xt_off + (size_t)nq * L.xt_stride * 4);   // (used when the caller passes no prepared block)
  L.total = L.prepared_off + L.C.total;
  return L;
}

static int run_probe_prepare(const float* centroids, int d, int n_cells, char* prepared, const ProbePrepared& C,
                             hipStream_t st) {
  float* mu = reinterpret_cast<float*>(prepared + C.mu_off);
  float* scale = reinterpret_cast<float*>(prepared + C.scale_off);
  int* cflag = reinterpret_cast<int*>(prepared + C.cflag_off);
  unsigned* maxbits = reinterpret_cast<unsigned*>(prepared + C.maxbits_off);
  unsigned* cmax = reinterpret_cast<unsigned*>(prepared + C.cmax_off);
  int rc = check_hip(hipMemsetAsync(prepared, 0, C.frags_off, st), "coarse_probe_prepare memset");
  if (rc) return rc;
  rc = launch_scale({centroids, n_cells, centroids, n_cells, 1, d, 4096, 1, 1, true, mu, maxbits, cflag, scale}, st);
  if (rc) return rc;
  rc = launch_cprep(centroids, mu, scale, reinterpret_cast<u32x4*>(prepared + C.frags_off), cmax, cflag, 1, d, n_cells,
                    C.chunks, C.KS, st);
  if (rc) return rc;
  hipLaunchKernelGGL(probe_rows_kernel, dim3((n_cells + 31) / 32), dim3(256), 0, st, centroids,
                     reinterpret_cast<float*>(prepared + C.ct_off), reinterpret_cast<float*>(prepared + C.c2_off), d,
                     n_cells);
  TPQ_LAUNCH_CHECK("probe_rows_kernel");
  return TPQ_OK;
}

template <int KS>
static int run_probe_sims(const float* query, const char* prepared, int d, int nq, int n_cells, char* ws,
                          const ProbeLayout& L, ProbeFastBuffers* out, hipStream_t st) {
  const PrepLayout& P = L.P;
  const ProbePrepared& C = L.C;
  char* p = ws + L.prep_off;
  int* flag = reinterpret_cast<int*>(ws + L.flag_off);   // (queries beyond the scale carry it in their norm)
  _Float16* sims = reinterpret_cast<_Float16*>(ws + L.sims_off);
  float* gmax = reinterpret_cast<float*>(ws + L.gmax_off);
  float* band = reinterpret_cast<float*>(ws + L.band_off);
  float* qscale = reinterpret_cast<float*>(ws + L.qscale_off);
  const float* mu = reinterpret_cast<const float*>(prepared + C.mu_off);
  const float* scale = reinterpret_cast<const float*>(prepared + C.scale_off);
  const int* cflag = reinterpret_cast<const int*>(prepared + C.cflag_off);
  const unsigned* cmax = reinterpret_cast<const unsigned*>(prepared + C.cmax_off);
  const u32x4* frags = reinterpret_cast<const u32x4*>(prepared + C.frags_off);
  float* q2 = reinterpret_cast<float*>(ws + L.q2_off);
  float* xt = reinterpret_cast<float*>(ws + L.xt_off);
  const ProbeSplitOut po{xt, q2, band, qscale, cmax, cflag, level_eps(KS, 16 * KS, 1), (float)(d + 4) / 16777216.0f,
                         sqrtf((float)(16 * KS)) / 8192.0f, L.xt_stride};
  hipLaunchKernelGGL(probe_split_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(256), 0, st, query, mu, scale,
                     reinterpret_cast<u32x4*>(p + P.hi_off), reinterpret_cast<u32x4*>(p + P.mid_off), d, (int64_t)nq, P.T, KS,
                     po);
  TPQ_LAUNCH_CHECK("probe_split_kernel");
  const size_t lds = (size_t)8 * (KS + 1) * 1024;
  auto kernel = L.gshift == 5 ? probe_sims_kernel<KS, 5> : (L.gshift == 6 ? probe_sims_kernel<KS, 6> : probe_sims_kernel<KS, 7>);
  // wide tiles (64 queries) per wave: as few as it takes to put >= ~1 000 blocks on the chip
  const int64_t wide = (P.T + 1) / 2;
  int n_wide = (int)((wide * C.chunks) / ((int64_t)kWaves * 1024));
  n_wide = n_wide < 1 ? 1 : (n_wide > kWide ? kWide : n_wide);
  // the block's sims rows are ONE buffer resource addressed with 32-bit offsets (probe_sims_kernel): its
  // rows x n_cells x 2 bytes must stay below the out-of-range sentinel 0x7ffffff0 (at 262 144 cells a block of
  // 8 192 rows was 4 GiB: num_records truncated to 0, row offsets wrapped).  lloyd_probe_supported() keeps one
  // wide tile per wave inside the range; here the tiles per wave are cut to what fits.
  const int64_t row_bytes = (int64_t)n_cells * 2, rows_per_wide = (int64_t)kWaves * 64;
  const int64_t fit = (int64_t)0x7ffffff0 / (row_bytes * rows_per_wide);
  if (fit < 1) {
    set_error("probe_sims: %d cells: one block's rows exceed the 2 GiB buffer resource", n_cells);
    return TPQ_ERR_UNSUPPORTED;
  }
  n_wide = n_wide > fit ? (int)fit : n_wide;
  const int64_t per_block = (int64_t)kWaves * n_wide;
  ProbeSimsArgs pa{reinterpret_cast<const u32x4*>(p + P.hi_off), frags, sims, qscale, gmax, nq, n_cells, L.n_groups, n_wide,
                   P.T, 8 * (2 * KS + 1) * 64};
  int rc = launch_with_lds(kernel, "probe_sims_kernel", dim3((unsigned)((wide + per_block - 1) / per_block), C.chunks),
                           dim3(kWaves * 64), lds, st, pa);
  if (rc) return rc;
  *out = ProbeFastBuffers{sims, gmax, band, qscale, xt, q2, L.xt_stride, reinterpret_cast<const float*>(prepared + C.ct_off),
                          reinterpret_cast<const float*>(prepared + C.c2_off), L.n_groups, L.gshift};
  return TPQ_OK;
}

}  // namespace lloyd

// ---- the coarse step's row select on FAST similarities: one wave per query ---------------------------------------
// The reference offers a reduced-precision coarse GEMM behind use_tensor_core / fp16_scale_mode (torchpq/metric.py:47-73,
// index/IVFPQIndex.py:98-125) and accepts its errors; here the fp16 pass only SELECTS: every cell that can still be among
// the query's n_probe best -- fast value within twice a rigorous error bound of the n_probe-th best fast value -- gets the
// fp32 kernel's own value (the same ascending-k fma chain), and the result (cells, order, similarities) is
// coarse_sims_kernel's (coarse_probe.hip), bit for bit.
//   1. the k best fast values of the row, kept with a margin: everything within `band` = 2 delta' of the running
//      k-th best is admitted and the list holds 64 R > k entries (the group filter works on fast values too: a group
//      is read when its maximum reaches the k-th largest group maximum minus the band);
//   2. every list entry within the band of the k-th best fast value is a CANDIDATE: the exact top-k is among them
//      (|f' - e'| <= delta' for every cell).  A lane evaluates its candidate with the fp32 kernels' own arithmetic --
//      acc = fma chain over ascending k of C[k][c] x[k], v = ((2 acc) - |x|^2) - |C|^2 -- from the centroid's row copy;
//   3. the candidates are re-ranked by (exact value desc, cell asc) and the best k written: coarse_sims_kernel +
//      topk_select_kernel's output, bit for bit.
// A list full of candidates (an entry may have been evicted), or band = +inf (queries / centroids beyond the fp16 scale):
// the wave evaluates ALL cells of its query exactly -- slow, and normally never taken.
constexpr int kCandCap = 256;  // candidate cells a wave keeps without selecting (direct path)
constexpr int kHotCap = 512;   // hot groups a wave lists

// Every lane of the wave calls it; the lanes with `take` set append x to the wave's own LDS list, in lane order, while
// it has room.  n -- wave-uniform, kept in a register -- counts every taker, so n > cap says that the list overflowed.
__device__ __forceinline__ void list_append(bool take, int x, int* list, int cap, int& n) {
  const unsigned long long b = __ballot(take);
  const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
  if (take && pos < cap) list[pos] = x;
  n += __popcll(b);
}

template <int R>
__global__ __launch_bounds__(kSelWaves * 64) void probe_select_fast_kernel(ProbeFastBuffers fb, const float* __restrict__ x,
                                                                          float* __restrict__ vals,
                                                                          int64_t* __restrict__ idx, int d, int nq,
                                                                          int n_cells, int k, ProbeEpilogue pe) {
  __shared__ float qv[kSelWaves * 64];
  __shared__ int qi[kSelWaves * 64];
  __shared__ float xq_all[kSelWaves * 128];
  __shared__ int cand[kSelWaves * kCandCap];
  __shared__ int hot[kSelWaves * kHotCap];
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int row = blockIdx.x * kSelWaves + wave;
  if (row >= nq) return;
  float* xq = xq_all + wave * 128;
  // everything the wave needs first, issued together: its query's row (d <= 128 floats), |x|^2, band, scale and the
  // first group maxima
  const float4 xrow = lane * 4 < d ? reinterpret_cast<const float4*>(fb.xt + (int64_t)row * fb.xt_stride)[lane]
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
  const float q2 = fb.q2[row];
  const float band0 = fb.band[row];
  const float qs = fb.qscale[row];
  const float* __restrict__ gm = fb.gmax + (int64_t)row * fb.n_groups;   // f' (fp32): scaled on the fly
  float gm0[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) gm0[u] = 64 * u + lane < fb.n_groups ? gm[64 * u + lane] : -INFINITY;
  if (lane * 4 < d) reinterpret_cast<float4*>(xq)[lane] = xrow;  // (d % 4 != 0: the row copy is zero-padded to xt_stride)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  auto exact = [&](int c) -> float {  // the fp32 kernels' value of (query, cell c)
    const float4* __restrict__ cr = reinterpret_cast<const float4*>(fb.ct + (int64_t)c * d);
    float acc = 0.f;
    int t = 0;
    auto block = [&](auto n_c) {
      load_then_use<decltype(n_c)::value>([&](int u) { return cr[(t >> 2) + u]; },
                                          [&](int u, const float4& y) {
                                            acc = fmaf(y.x, xq[t + 4 * u], acc);
                                            acc = fmaf(y.y, xq[t + 4 * u + 1], acc);
                                            acc = fmaf(y.z, xq[t + 4 * u + 2], acc);
                                            acc = fmaf(y.w, xq[t + 4 * u + 3], acc);
                                          });
    };
    // (each candidate's row is a lane's own: eight loads in flight, four round trips at d = 128)
    for (; t + 32 <= d; t += 32) block(std::integral_constant<int, 8>{});
    for (; t + 16 <= d; t += 16) block(std::integral_constant<int, 4>{});
    for (; t < d; ++t) acc = fmaf(fb.ct[(int64_t)c * d + t], xq[t], acc);
    const float v = neg_sq_l2(acc, q2, fb.c2[c]);
    return v + 0.0f;  // (a statement of its own: folded into the line above, the kernel's registers are allocated differently)
  };
#ifdef TPQ_SELECT_STOP
#define TPQ_STOP_AT(n, val) if (TPQ_SELECT_STOP == n) { if (lane == 0) vals[(int64_t)row * k] = (val); return; }
#else
#define TPQ_STOP_AT(n, val)
#endif
  TPQ_STOP_AT(1, q2)
  WaveTopK<R> ex;
  bool slow = !(band0 < INFINITY);
  if (!slow) {
    WaveSelector<R> sel;
    sel.init(qv + wave * 64, qi + wave * 64, k);
    sel.margin = band0;
    const _Float16* __restrict__ xr = fb.sims + (int64_t)row * n_cells;  // stored units: f' x qs, fp16
    const uint32_t* __restrict__ xr2 = reinterpret_cast<const uint32_t*>(xr);  // (rows are 64-byte aligned: n_cells % 32 == 0)
    // phase 1: the k-th largest group maximum (a lower bound of the k-th largest fast value)
    for (int base = 0; base < fb.n_groups; base += 64) {
      const int g = base + lane;
      const float gv = base < 256 ? gm0[(base >> 6) & 3] : (g < fb.n_groups ? gm[g] : -INFINITY);
      const float v = g < fb.n_groups ? gv * qs + 0.0f : -INFINITY;
      sel.push(g < fb.n_groups && (v >= sel.tau - band0), v, g);
    }
    sel.flush();
    // The stored values are fp16: u = f' x qs rounded to nearest, |stored - u| <= 2^-11 |u| (+ 2^-25 where the result is
    // subnormal).  A cell that belongs to the exact top k has u in [G_k - band0, M_1] (G_k the k-th largest group
    // maximum -- a lower bound of the k-th largest u --, M_1 the largest; both unrounded), so its stored value is within
    // eps = 2^-11 (max(|M_1|, |G_k|) + band0) of u; and the k-th largest stored value is within eps of the k-th largest u
    // (rounding is monotone, the k-th largest u lies in [G_k, M_1]).  Band in stored values: band0 + 2 eps.  |u| < 2^15
    // by the choice of qs: eps <= 16 whatever the row holds (fewer than k groups: G_k = -inf).
    const float gk = sel.top.kth_value(k);
    const float mag = fmaxf(fabsf(sel.top.kth_value(1)), fabsf(gk)) + band0;
    const float eps = fminf(16.f, mag * 4.8828125e-4f) * 1.001f + 5.9604645e-8f;
    const float band = band0 + 2.f * eps;
    const float tau0 = gk - band;  // -inf while there are fewer than k groups
    TPQ_STOP_AT(2, tau0)
    // the hot groups -- those whose maximum reaches tau0 -- as a list in LDS, then their cells two per lane (a dword of
    // the fp16 row; a 32-cell group is 16 lanes of a load, a 128-cell group all 64), eight loads a round: the walk is a
    // chain of memory round trips and there are as many of them as rounds
    int* hl = hot + wave * kHotCap;
    int n_hot = 0;  // wave-uniform
    for (int base = 0; base < fb.n_groups; base += 64) {
      const int g = base + lane;
      const float gv = base < 256 ? gm0[(base >> 6) & 3] : (g < fb.n_groups ? gm[g] : -INFINITY);
      const bool is_hot = g < fb.n_groups && (gv * qs >= tau0);
      list_append(is_hot, g, hl, kHotCap, n_hot);
    }
    const bool hot_listed = n_hot <= kHotCap;  // (more groups than the list holds: only beyond 65 536 cells; exact then)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (the wave's own LDS appends)
    const int lpg_shift = fb.gshift - 1;                    // lanes per group: a lane holds two cells
    const int sub = lane >> lpg_shift, lig = lane & ((1 << lpg_shift) - 1);
    const int gpl = 64 >> lpg_shift;                        // groups per load
    auto walk = [&](auto&& consume, auto&& go_on) {
      for (int h0 = 0; h0 < n_hot && go_on(); h0 += 8 * gpl) {
        uint32_t vw[8];
        int cb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int hi = h0 + u * gpl + sub;
          const int g = hi < n_hot ? hl[hi] : -1;
          const int c = (g << fb.gshift) + 2 * lig;   // (n_cells is even: a pair is inside the row or beyond it)
          const bool ok = g >= 0 && c < n_cells;
          vw[u] = ok ? xr2[c >> 1] : 0xfc00fc00u;      // (-inf, -inf)
          cb[u] = ok ? c : -1;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (h0 + u * gpl < n_hot) {  // wave-uniform
            typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
            const f16x2 hv = __builtin_bit_cast(f16x2, vw[u]);
            consume(cb[u] >= 0, cb[u], (float)hv[0]);
            consume(cb[u] >= 0, cb[u] + 1, (float)hv[1]);
          }
        }
      }
    };
    // phase 2, direct: EVERY cell of a hot group whose stored value reaches tau0 is kept -- a superset of the candidates
    // (cut >= tau0: the k-th largest stored value is not below G_k - eps) that costs a ballot and an LDS append per 64
    // cells instead of the selector's queue, sorts and merges; the exact top k is among them whatever else is, so the
    // exact values of all of them, sorted once, are the answer.  More than kCandCap of them (k close to or beyond the
    // number of groups: G_k is a poor bound or none) and the selector path below finds the cut itself.
    int* cl = cand + wave * kCandCap;
    int n_cand = 0;  // wave-uniform
    bool direct = hot_listed && gk > -INFINITY && 2 * k <= fb.n_groups;  // (k-th of fewer than 2 k maxima: too low a bound to try)
    if (direct) {
      walk(
          [&](bool valid, int c, float v) { list_append(valid && v >= tau0, c, cl, kCandCap, n_cand); },
          [&]() { return n_cand <= kCandCap; });
      direct = n_cand <= kCandCap;
    }
    TPQ_STOP_AT(3, (float)n_cand)
    if (direct) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (the wave's own LDS appends)
      ex.init();
      for (int base = 0; base < n_cand; base += 64) {
        const bool want = base + lane < n_cand;
        const int c = want ? cl[base + lane] : 0;
        const float e = want ? exact(c) : -INFINITY;
        ex.insert_unsorted(want ? make_key(e, c) : pad_key());
      }
      TPQ_STOP_AT(4, ex.kth_value(1))
    } else if (!hot_listed) {
      slow = true;
    } else {
    sel.init(qv + wave * 64, qi + wave * 64, k);
    sel.margin = band;
    // phase 2 through the selector: the k best stored values with their band
    walk([&](bool valid, int c, float v0) {
           const float v = v0 + 0.0f;
           sel.push(valid && (v >= sel.tau - band), v, c);
         },
         [&]() { return true; });
    sel.flush();
    const float cut = sel.top.kth_value(k) - band;
    const Key last = readlane_key(sel.top.k[R - 1], 63);
    if (key_index(last) != kPadIdx && key_value(last) >= cut) slow = true;  // a full list of candidates: wave-uniform
    if (!slow) {
      ex.init();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int c = key_index(sel.top.k[r]);
        const bool want = c != kPadIdx && key_value(sel.top.k[r]) >= cut;
        if (__ballot(want) == 0ull) break;  // sorted by fast value: nothing further down qualifies
        const float e = want ? exact(c) : -INFINITY;
        ex.insert_unsorted(want ? make_key(e, c) : pad_key());
      }
    }
    }
  }
  if (slow) {  // every cell, exactly
    WaveSelector<R> sel;
    sel.init(qv + wave * 64, qi + wave * 64, k);
    for (int base = 0; base < n_cells; base += 64) {
      const int c = base + lane;
      const float v = c < n_cells ? exact(c) : -INFINITY;
      sel.push(c < n_cells && (v >= sel.tau), v, c);
    }
    sel.flush();
    ex = sel.top;
  }
  write_row<R>(ex, vals, idx, row, k, pe);
}

// hooks for tpq_ivfpq_coarse_probe (coarse_probe.hip, probe_fast.h): euclidean, d <= 128, whole 16-byte pieces per row
int lloyd_probe_supported(int d, int nq, int n_cells) {
  // d % 4: probe_select_fast_kernel reads the centroid rows (stride d floats) as float4.
  // n_cells <= 2^20: the 512 rows of one wide tile per wave (kWaves x 64) x n_cells x 2 bytes must fit the 32-bit
  // buffer resource of probe_sims_kernel (run_probe_sims cuts the tiles per wave to what fits).
  if (!(d >= 4 && d <= 128 && (d & 3) == 0 && nq >= 1 && n_cells >= 256 && (n_cells & 31) == 0 && n_cells <= (1 << 20)))
    return 0;
  if ((int64_t)n_cells * 2 * lloyd::kWaves * 64 > (int64_t)0x7ffffff0) return 0;
  return (int64_t)nq * n_cells < (1LL << 36) ? 1 : 0;
}
int lloyd_probe_groups(int n_cells) {
  const int gs = lloyd::probe_gshift(n_cells);
  return (n_cells + (1 << gs) - 1) >> gs;
}
size_t lloyd_probe_workspace_bytes(int d, int nq, int n_cells) {
  return lloyd_probe_supported(d, nq, n_cells) ? lloyd::probe_layout(d, nq, n_cells).total : 0;
}
size_t lloyd_probe_prepared_bytes(int d, int n_cells) {
  return lloyd_probe_supported(d, 1, n_cells) ? lloyd::probe_prepared_layout(d, n_cells).total : 0;
}
int lloyd_probe_prepare(const float* centroids, int d, int n_cells, char* prepared, hipStream_t st) {
  const lloyd::ProbePrepared C = lloyd::probe_prepared_layout(d, n_cells);
  return lloyd::run_probe_prepare(centroids, d, n_cells, prepared, C, st);
}
int lloyd_probe_select(const float* query, const float* centroids, const void* prepared, int d, int nq, int n_cells,
                       int n_probe, float* topk_sims, int64_t* cells, const ProbeEpilogue& pe, char* ws, hipStream_t st) {
  const lloyd::ProbeLayout L = lloyd::probe_layout(d, nq, n_cells);
  const char* prep = reinterpret_cast<const char*>(prepared);
  if (!prep) {  // no prepared block: prepare into the workspace, for this call
    int rc = lloyd_probe_prepare(centroids, d, n_cells, ws + L.prepared_off, st);
    if (rc) return rc;
    prep = ws + L.prepared_off;
  }
  ProbeFastBuffers fb;
  int rc;
  switch (L.KS) {
    case 2: rc = lloyd::run_probe_sims<2>(query, prep, d, nq, n_cells, ws, L, &fb, st); break;
    case 4: rc = lloyd::run_probe_sims<4>(query, prep, d, nq, n_cells, ws, L, &fb, st); break;
    default: rc = lloyd::run_probe_sims<8>(query, prep, d, nq, n_cells, ws, L, &fb, st);
  }
  if (rc) return rc;
  // (the candidate list: 64 R >= n_probe + 16 entries)
  return with_list_regs(list_regs(n_probe + 16), [&](auto r_c) -> int {
    hipLaunchKernelGGL(probe_select_fast_kernel<decltype(r_c)::value>, dim3((nq + kSelWaves - 1) / kSelWaves),
                       dim3(kSelWaves * 64), 0, st, fb, query, topk_sims, cells, d, nq, n_cells, n_probe, pe);
    TPQ_LAUNCH_CHECK("probe_select_fast_kernel");
    return TPQ_OK;
  });
}
}  // namespace tpq
