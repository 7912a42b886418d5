// The kernels every unit of the fp16 cascade runs (fp16_cascade.h: the scheme and its error bound), each compiled once,
// here, behind a host launcher: the preparation -- mu, maxabs, scale, split (points -> fp16 pieces h + m in fragment
// order), cprep (centroids -> fragments) -- and the levels on prepared pieces: coarse, refine, refine_stream, decide.
#include "fp16_cascade.h"

namespace tpq {
namespace lloyd {

// mu[b][k] = mean over the n initial centroids of dimension k (zero beyond d)
__global__ __launch_bounds__(256) void mu_kernel(const float* __restrict__ B, float* __restrict__ mu, int d, int n) {
  __shared__ float red[256];
  const int k = blockIdx.x, b = blockIdx.y;
  const float* row = B + ((int64_t)b * d + k) * n;
  float s = 0.f;
  for (int c = threadIdx.x; c < n; c += 256) s += row[c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = red[0] / (float)n;
    mu[b * kMu + k] = (v == v && fabsf(v) <= 3.0e38f) ? v : 0.f;  // a non-finite mean: no centring (flagged below)
  }
}

// max |x - mu| per sub-problem (bits of a non-negative float: integer order == value order) and a
// flag for any non-finite element.  grid (chunks, d, l)
// `sample` > 1: only every sample-th 4-KiB run of a row is read (tpq_lloyd_prepare: the scale then leaves one bit
// of headroom and split_kernel, which sees every element, flags what exceeds it -- a full pass over 16 GB for
// a power of two was 2.8 ms of the 13.3 ms the preparation took)
__global__ __launch_bounds__(256) void maxabs_kernel(const float* __restrict__ A, const float* __restrict__ mu,
                                                    unsigned* __restrict__ maxbits, int* __restrict__ flag, int d,
                                                    int64_t m, int sample = 1) {
  const int k = blockIdx.y, b = blockIdx.z;
  const float* row = A + ((int64_t)b * d + k) * m;
  const float mk = mu[b * kMu + k];
  float mx = 0.f;
  int bad = 0;
  const int64_t per = (m + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = (i0 + per) < m ? (i0 + per) : m;
  if ((m & 3) == 0 && (per & 3) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0) {
    for (int64_t i = i0 + (int64_t)threadIdx.x * 4; i < i1; i += 1024 * (int64_t)sample) {
      const float4 x = *reinterpret_cast<const float4*>(row + i);
      const float v0 = fabsf(x.x - mk), v1 = fabsf(x.y - mk), v2 = fabsf(x.z - mk), v3 = fabsf(x.w - mk);
      bad |= !(v0 <= 3.0e38f) | !(v1 <= 3.0e38f) | !(v2 <= 3.0e38f) | !(v3 <= 3.0e38f);
      mx = fmaxf(fmaxf(mx, fmaxf(v0, v1)), fmaxf(v2, v3));
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256 * (int64_t)sample) {
      const float v = fabsf(row[i] - mk);
      bad |= !(v <= 3.0e38f);
      mx = fmaxf(mx, v);
    }
  }
  __shared__ float red[256];
  __shared__ int redb[256];
  red[threadIdx.x] = mx;
  redb[threadIdx.x] = bad;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
      redb[threadIdx.x] |= redb[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (red[0] > 0.f) atomicMax(maxbits + b, __float_as_uint(red[0]));
    if (redb[0]) atomicOr(flag + b, 1);
  }
}

// s[b] = 2^(13 - floor(log2 max)): max |x - mu| s in [2^13, 2^14)
// (headroom = 1: the maximum came from a sample; it lands in [2^12, 2^13) and the data may exceed it twofold)
__global__ void scale_kernel(const unsigned* __restrict__ maxbits, int* __restrict__ flag, float* __restrict__ scale,
                             int l, int headroom = 0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= l) return;
  const float mx = __uint_as_float(maxbits[b]);
  float s = 1.f;
  if (flag[b] || !(mx <= 3.0e38f)) {
    flag[b] = 1;
  } else if (mx > 0.f) {
    int e = ilogbf(mx);
    int se = 13 - headroom - e;
    se = se > 100 ? 100 : (se < -100 ? -100 : se);
    s = ldexpf(1.f, se);
    if (!(mx * s < 16384.f)) flag[b] = 1;  // (a clamped exponent on astronomically large data)
  }
  scale[b] = s;
}

// norms[point] = (|a'|^2, packed): the second word carries two quantities that only ever enter BOUNDS, each
// rounded UP to bf16: |x|^2 (the exact kernel's own rounding scales with it) in the high half, and
// |a' - ah|^2 -- what level 1 drops of this point -- in the low half.
__device__ __forceinline__ unsigned bf16_up(float x) {  // x >= 0 (an overflow to inf just lists the point)
  return (__float_as_uint(x) + 0xffffu) >> 16;
}
__device__ __forceinline__ float pack_bound_norms(float n2r, float n2m) {
  return __uint_as_float((bf16_up(n2r) << 16) | bf16_up(n2m));
}
__device__ __forceinline__ void unpack_bound_norms(float y, float& n2r, float& n2m) {
  const unsigned u = __float_as_uint(y);
  n2r = __uint_as_float(u & 0xffff0000u);
  n2m = __uint_as_float(u << 16);
}

// pieces + norms.  grid (ceil(m / 256), l), 4 waves; LANE = POINT (64 consecutive points per wave = two tiles):
// every load instruction reads 256 contiguous bytes of one dimension's row, and a lane owns the 64 contiguous
// bytes of its point in each (k-step pair, piece), written as four 16-byte chunks -- a wave's stores of one pair
// are two whole 2-KiB runs.  (Round 3's kernel gave a lane (point, half of a k-step): 128-byte reads, 32-byte
// interleaved writes, 2.9 TB/s over 16 GB in + 16 GB out.)  Every element is seen here, so this is also where a
// non-finite value, or one beyond the range the (sampled) scale leaves, flags its sub-problem.
// The coarse probe's queries get the same pieces from probe_split_kernel (probe_sims.hip).
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ A, const float* __restrict__ mu,
                                                   const float* __restrict__ scale, u32x4* __restrict__ hi,
                                                   u32x4* __restrict__ mid, float2* __restrict__ norms,
                                                   int* __restrict__ flag, int d, int64_t m, int64_t T, int KS) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t tile = i >> 5;
  if (tile >= T) return;
  const int l31 = (int)(i & 31);
  const bool iv = i < m;
  const float* Ab = A + (int64_t)b * d * m + (iv ? i : 0);
  const float* mub = mu + b * kMu;
  const float s = scale[b];
  const int Q = (KS + 1) / 2;
  float n2c = 0.f, n2r = 0.f, n2m = 0.f;
  int bad = 0;
  for (int q = 0; q < Q; ++q) {
    float x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int k = 32 * q + j;
      x[j] = (iv && k < d) ? Ab[(int64_t)k * m] : 0.f;
    }
    const int64_t fo = (((int64_t)b * T + tile) * Q + q) * 128 + l31 * 4;  // in 16-byte chunks
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f16x8 h, mm;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * q + 8 * c + j;
        const float xv = x[8 * c + j];
        const float a = (iv && k < d) ? (xv - mub[k]) * s : 0.f;
        bad |= !(fabsf(a) < 16384.f);
        const _Float16 hh = (_Float16)a;
        const float r = a - (float)hh;
        h[j] = hh;
        mm[j] = (_Float16)r;
        n2c = fmaf(a, a, n2c);
        n2r = fmaf(xv, xv, n2r);
        n2m = fmaf(r, r, n2m);
      }
      hi[fo + c] = __builtin_bit_cast(u32x4, h);
      mid[fo + c] = __builtin_bit_cast(u32x4, mm);
    }
  }
  // (a point the scale cannot hold carries an infinite norm: every bound derived from it is infinite, whoever reads it)
  norms[(int64_t)b * T * 32 + i] = make_float2(bad ? INFINITY : n2c, pack_bound_norms(n2r, n2m));
  if (__ballot(bad != 0) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag + b, 1);
}

// ---- per iteration: centroid fragments -----------------------------------------------------------
// grid (8 units, l), 64 lanes: lane (row = centroid l31 of the unit, k-group half).
// frags [l][8][2 KS + 1][64] x 16 B: fragment 0 = -N (N = fl |c'|^2) as three exact bf16 pieces at
// k = 0, 1, 2 (rows beyond n: -3e38, never first or second); fragments 1 + 2 st + q = piece q of
// C = 2 c' = 2 s (c - mu), k-step st, fp16.
__global__ __launch_bounds__(64) void cprep_kernel(const float* __restrict__ B, const float* __restrict__ mu,
                                                  const float* __restrict__ scale, u32x4* __restrict__ frags,
                                                  unsigned* __restrict__ cmax2_bits, int* __restrict__ cflag, int d,
                                                  int n, int KS) {
  const int unit = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  const int c = unit * 32 + l31;
  const int FPU = 2 * KS + 1;
  const float* Bb = B + (int64_t)b * d * n;
  const float s = scale[b];
  u32x4* out = frags + ((int64_t)b * gridDim.x + unit) * FPU * 64 + lane;  // (gridDim.x = 8 units per chunk of 256)
  float N = 0.f, sraw = 0.f;
  if (c < n)
    for (int k = 0; k < d; ++k) {
      const float y = Bb[(int64_t)k * n + c];
      const float cc = (y - mu[b * kMu + k]) * s;
      N = fmaf(cc, cc, N);
      sraw = fmaf(y, y, sraw);
    }
  int bad = 0;
  {
    bf16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
    if (half == 0) {
      __bf16 p1, p2, p3;
      split3_bf16(c < n ? -N : -3.0e38f, p1, p2, p3);
      f[0] = p1;
      f[1] = p2;
      f[2] = p3;
    }
    out[0] = __builtin_bit_cast(u32x4, f);
  }
  if (c < n) {
    bad |= !(N <= 3.0e38f) | !(sraw <= 3.0e38f);
    if (half == 0 && !bad) {
      atomicMax(cmax2_bits + b * kCm, __float_as_uint(N));
      atomicMax(cmax2_bits + b * kCm + 1, __float_as_uint(sraw));
    }
  }
  float c2m = 0.f;  // |C - Ch|^2: what level 1 drops of this centroid
  for (int st = 0; st < KS; ++st) {
    f16x8 h, mm;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * st + 8 * half + j;
      const float C = (k < d && c < n) ? 2.f * ((Bb[(int64_t)k * n + c] - mu[b * kMu + k]) * s) : 0.f;
      bad |= !(fabsf(C) <= 65000.f);  // beyond fp16's range (or NaN): the whole sub-problem goes exact
      const _Float16 hh = (_Float16)C;
      const float r = C - (float)hh;
      h[j] = hh;
      mm[j] = (_Float16)r;
      c2m = fmaf(r, r, c2m);
    }
    out[(1 + 2 * st) * 64] = __builtin_bit_cast(u32x4, h);
    out[(2 + 2 * st) * 64] = __builtin_bit_cast(u32x4, mm);
  }
  c2m += __shfl_xor(c2m, 32, 64);
  if (half == 0 && c < n && !bad) atomicMax(cmax2_bits + b * kCm + 2, __float_as_uint(c2m));
  if (bad) atomicOr(cflag + b, 1);
}

// label, value and -- unless the two best fast values are more than 2 delta apart -- a list entry.
// Called by all lanes of the wave.  The list is staged in LDS (one LDS atomic per wave) and flushed
// once per block (flush_list): a RETURNING global atomic per tile put a memory round trip -- and,
// vmcnt being in order, the wait for every load issued before it -- into each tile of level 1,
// where 92 % of the tiles hold an undecided point (19 ms instead of 2).
template <int CAP>
struct BlockListT {
  int n;
  int base;
  int item[CAP];
};
template <int CAP>
__device__ __forceinline__ void emit(const StepArgs& a, BlockListT<CAP>* bl, int b, int lane, bool valid, int64_t fi,
                                     int idx, float B1, float B2, float2 n2, float s, float cn, float cnr,
                                     float inv_s2, bool exact_all, float c2, int64_t part_slot = -1) {
  if (a.part_b != nullptr) {  // chunked: this chunk's result of the point; decide_kernel does the rest
    if (valid) {
      a.part_b[part_slot] = make_float2(B1, B2);
      a.part_i[part_slot] = (uint8_t)idx;
    }
    return;
  }
  // (v_sqrt_f32: 1 ulp; the norms only scale the bound, whose 1.25 covers it)
  float n2r, n2m;
  unpack_bound_norms(n2.y, n2r, n2m);
  const float an = __builtin_amdgcn_sqrtf(n2.x), anr = __builtin_amdgcn_sqrtf(n2r) * s;
  const float t1 = an + cn, t2 = anr + cnr * s;
  // Level 1 drops the products with the mid pieces: |sum (a C - ah Ch)| <= |a' - ah| (|Ch|max + |C - Ch|max) +
  // |a'| |C - Ch|max with what was ACTUALLY dropped of this point and of the worst centroid (|Ch| <= (1 + 2^-11)
  // 2 |c'|) -- about 0.4 of the worst case 2^-11 (|a'| + |c'|max)^2, and 7.5 % undecided points become 3 %.
  // (c2 = max |C - Ch|, read ONCE by the caller: a load here, in the tile loop, sits behind the prefetched pieces
  // on the in-order vmcnt and cost level 1 18 % -- or < 0 at level 2, which drops nothing)
  float dropped = 0.f;
  if (c2 >= 0.f) {
    const float a2 = __builtin_amdgcn_sqrtf(n2m);
    dropped = a2 * (2.002f * cn + c2) + 1.001f * an * c2;
  }
  float delta = 1.25f * (dropped + a.eps * t1 * t1 + a.eta * (2.f * cn + an) + a.eps_exact * t2 * t2);
  if (exact_all) delta = INFINITY;
  if (valid) {
    a.inds[(int64_t)b * a.m + fi] = idx;
    if (a.vals) a.vals[(int64_t)b * a.m + fi] = (B1 - n2.x) * inv_s2;
  }
  const bool listed = valid && !(B1 - B2 > 2.f * delta);
  const unsigned long long mk = __ballot(listed);
  if (mk) {
    const int leader = __ffsll((long long)mk) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&bl->n, __popcll(mk));  // LDS
    base = __shfl(base, leader, 64);
    if (listed) bl->item[base + __popcll(mk & ((1ull << lane) - 1ull))] = (int)fi;
  }
}
// end of the block: reserve [base, base + n) of the sub-problem's list with one global atomic, copy
template <int CAP>
__device__ __forceinline__ void flush_list(const StepArgs& a, BlockListT<CAP>* bl, int b) {
  __syncthreads();
  if (threadIdx.x == 0) bl->base = bl->n ? atomicAdd(a.count + b, bl->n) : 0;
  __syncthreads();
  const int n = bl->n, base = bl->base;
  for (int i = threadIdx.x; i < n; i += kWaves * 64) a.list[(int64_t)b * a.m + base + i] = bl->item[i];
}

// ---- level 1 -----------------------------------------------------------------------------------------
// A wave owns WIDE tiles of 64 points (two MFMA column tiles sharing every A operand: at one A
// operand per MFMA the centroid fragments alone would take the whole LDS bandwidth -- 1 KiB per
// 32-cycle MFMA per SIMD = 128 B/clk/CU); the two accumulators of a k-step are independent, so no
// MFMA waits for the one before it.  LDS holds -N and the hi pieces of the centroids only (40 KiB).
constexpr int kCoarseList = kWaves * kWide * 64;  // points a level-1 block decides = capacity of its staged list

template <int KS>
__global__ __launch_bounds__(kWaves * 64, 2) void coarse_kernel(StepArgs a) {
  constexpr int FPU = 2 * KS + 1;  // fragments per unit in global memory
  constexpr int FL = KS + 1;       // ... in LDS
  constexpr int Q = (KS + 1) / 2;
  typedef BlockListT<kCoarseList> BL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool chunked = a.part_b != nullptr;
  const int b = chunked ? 0 : blockIdx.y, chunk = chunked ? blockIdx.y : 0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  const int m = a.m;
  BL* bl = reinterpret_cast<BL*>(smem + 8 * FL * 1024);
  if (threadIdx.x == 0) bl->n = 0;
  {
    const char* src = reinterpret_cast<const char*>(a.frags) + (size_t)b * 8 * FPU * 1024 +
                      (size_t)chunk * a.chunk_frag_stride * 16;
    for (int f = wave; f < 8 * FL; f += kWaves) {
      const int unit = f / FL, j = f % FL;
      const int sf = unit * FPU + (j ? 2 * j - 1 : 0);  // -N, then the hi piece of k-step j - 1
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + sf * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(smem + f * 1024), 16, 0, 0);
    }
  }
  const int64_t slice = a.T * Q * 2048;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.hi) + (size_t)b * slice), 0, (int)slice, 0x00020000);
  const float2* __restrict__ nrm = a.norms + (int64_t)b * a.T * 32;
  auto wide_of = [&](int t) -> int64_t { return ((int64_t)blockIdx.x * kWide + t) * kWaves + wave; };
  auto frag_voff = [&](int t) -> int {
    const int64_t wt = wide_of(t);
    return (t < kWide && 2 * wt < a.T) ? (int)(2 * wt * Q * 2048) + l31 * 64 + half * 16 : 0x7ffffff0;
  };
  f16x8 xsb[2][2][KS];  // [buffer][column tile][k-step]
  float2 n2b[2][2];     // [buffer][column tile]
  // fragment e of the wide tile: column tile e / KS (the next tile), k-step e % KS
  auto load_frag = [&](int voff, auto e_c, f16x8 (&dst)[2][KS]) {
    constexpr int e = decltype(e_c)::value, ct = e / KS, st = e % KS;
    dst[ct][st] = __builtin_bit_cast(
        f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, ct * Q * 2048 + (st >> 1) * 2048 + (st & 1) * 32, 0));
  };
  auto load_norm = [&](int t, int ct) -> float2 {
    const int64_t tile = 2 * wide_of(t) + ct;  // (clamped: a tile beyond the range reads tile 0's norms; never used)
    return nrm[((t < kWide && tile < a.T) ? tile : 0) * 32 + l31];
  };
  {
    const int voff = frag_voff(0);
    static_for<0, 2 * KS>([&](auto e_c) { load_frag(voff, e_c, xsb[0]); });
    n2b[0][0] = load_norm(0, 0);
    n2b[0][1] = load_norm(0, 1);
  }
  __syncthreads();  // fragments (vmcnt(0) of the DMA) are in LDS
  const u32x4* fp = reinterpret_cast<const u32x4*>(smem) + lane;
  auto ldsf = [&](const u32x4* p) -> f16x8 { return __builtin_bit_cast(f16x8, *p); };

  // ONE accumulator per column tile.  A unit = its 2 (KS + 1) MFMAs -- the two tiles in turn on every A
  // operand, so no MFMA waits for the one before it and the centroid fragments cross the LDS port once
  // per TWO MFMAs -- then the top-2 update of its 2 x 16 values; the SIMD's other wave has its MFMAs
  // meanwhile.  The A operands run through a three-slot ring two k-steps ahead (all KS of a unit in
  // registers: 32 of them at d = 128).  Tried on the way (C5, all within 3 % of each other: the kernel is
  // bound by the VALU work of the update, not by its schedule): the two tiles half a unit out of phase
  // (updates of one between the MFMAs of the other); four waves per SIMD without register prefetch;
  // two accumulator SETS (updating unit U - 1 between the MFMAs of unit U): 256 VGPRs + 53 spilled
  // around the per-tile epilogue -- and a scratch reload waits, vmcnt being in order, for the piece
  // loads issued before it.
  f32x16 acc[2];
  float b1[2] = {-INFINITY, -INFINITY}, b2[2] = {-INFINITY, -INFINITY};
  float b1h[2] = {-INFINITY, -INFINITY};  // the best after units 0..3
  // A operands: k-steps 0 and 1 of a unit in a0 / a1 -- re-loaded for the NEXT unit as soon as this unit's
  // MFMAs have taken them --, k-steps >= 2 through a three-slot ring two k-steps ahead
  f16x8 a0 = ldsf(fp + 1 * 64), a1 = a0, aring[3];
  if constexpr (KS > 1) a1 = ldsf(fp + 2 * 64);
  const bf16x8 bones = ones3_bf16x8(half);  // B fragment of ones at k = 0, 1, 2
  const float s = a.scale[b];
  const float cn = sqrtf(__uint_as_float(a.cmax2_bits[b * kCm])), cnr = sqrtf(__uint_as_float(a.cmax2_bits[b * kCm + 1]));
  const float c2n = a.level == 1 ? sqrtf(__uint_as_float(a.cmax2_bits[b * kCm + 2])) : -1.f;
  const bool exact_all = (a.flag[b] | a.cflag[b]) != 0;
  const float inv_s2 = (1.f / s) * (1.f / s);

  auto finish = [&](int ct, int64_t tile, float2 n2) {
    const int tag = __float_as_int(b1[ct]) & 63, r0 = tag & 15;
    // a best key found in units 4..7 is greater than the best of units 0..3 (equal keys: b2 == b1, listed)
    const int unit = (tag >> 4) + (b1[ct] > b1h[ct] ? 4 : 0);
    int idx = unit * 32 + (r0 & 3) + 8 * (r0 >> 2) + 4 * half;
    const float m1 = b1[ct], m2 = b2[ct];
    const float o1 = __shfl_xor(m1, 32, 64), o2 = __shfl_xor(m2, 32, 64);
    const int oi = __shfl_xor(idx, 32, 64);
    const float B1 = fmaxf(m1, o1);
    const float B2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
    if (o1 > m1 || (o1 == m1 && oi < idx)) idx = oi;
    const int64_t fi = tile * 32 + l31;
    emit(a, bl, b, lane, half == 0 && fi < m, fi, idx, B1, B2, n2, s, cn, cnr, inv_s2, exact_all, c2n,
         (int64_t)chunk * m + fi);
  };
  using std::integral_constant;

  auto unit = [&](auto u_c, int voff_next, const f16x8 (&xs)[2][KS], f16x8 (&xsn)[2][KS]) {
    constexpr int U = decltype(u_c)::value;
    const u32x4* up = fp + U * FL * 64;
    const u32x4* upn = fp + ((U + 1) & 7) * FL * 64;  // the next unit (unit 0 of the next tile after 7)
    const f32x16 zero = zero_f32x16();
    const bf16x8 cfrag = __builtin_bit_cast(bf16x8, up[0]);
    if constexpr (U < 4) {  // the next wide tile's hi pieces: 2 KS 16-byte loads over units 0..3
      constexpr int l0 = (U * 2 * KS) / 4, l1 = ((U + 1) * 2 * KS) / 4;
      static_for<l0, l1>([&](auto e_c) { load_frag(voff_next, e_c, xsn); });
    }
    if constexpr (U == 4) {
      b1h[0] = b1[0];
      b1h[1] = b1[1];
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
    static_for<0, 16>([&](auto q_c) {  // 16 register pairs, the two column tiles in turn
      constexpr int q = decltype(q_c)::value, ct = q & 1, pq = q >> 1;
      top2_keys_pair(b1[ct], b2[ct], key6<2 * pq + 16 * (U & 3)>(acc[ct][2 * pq]),
                     key6<2 * pq + 1 + 16 * (U & 3)>(acc[ct][2 * pq + 1]));
    });
    __builtin_amdgcn_sched_barrier(0);
  };

  auto tile = [&](int t, auto cb_c) {
    constexpr int CB = decltype(cb_c)::value, NX = 1 - CB;
    const int voff_next = frag_voff(t + 1);
    n2b[NX][0] = load_norm(t + 1, 0);
    n2b[NX][1] = load_norm(t + 1, 1);
    b1[0] = b1[1] = b2[0] = b2[1] = -INFINITY;
    static_for<0, 8>([&](auto u_c) { unit(u_c, voff_next, xsb[CB], xsb[NX]); });
    const int64_t wt = wide_of(t);
    finish(0, 2 * wt, n2b[CB][0]);
    finish(1, 2 * wt + 1, n2b[CB][1]);
  };
#pragma unroll 1
  for (int t = 0; t < kWide; t += 2) {
    if (2 * ((int64_t)blockIdx.x * kWide + t) * kWaves >= a.T) break;
    tile(t, integral_constant<int, 0>{});
    if (t + 1 >= kWide || 2 * ((int64_t)blockIdx.x * kWide + t + 1) * kWaves >= a.T) break;
    tile(t + 1, integral_constant<int, 1>{});
  }
  if (!chunked) flush_list(a, bl, b);
}

// Key epilogue: the accumulator register number r (0..15: which of the lane's 16 centroid rows of
// the unit) replaces the value's low 4 mantissa bits, so the running best carries its own index
// and no compare / select is needed: per PAIR of values  t = med3(b1, k0, k1); b1 = max3(b1, k0, k1);
// b2 = max(b2, t)  (the second best of {b1 >= b2, k0, k1} is max(med3(b1, k0, k1), b2)).  5 VALU per
// two values against 8; the 2^-19 |v| the keys are off by is part of the bound (StepArgs::eps).
template <int R0>
__device__ __forceinline__ void take_keys_pair(float& p1, float& p2, float v0, float v1) {
  static_assert(R0 >= 0 && R0 + 1 <= 15, "inline constants");
  float k0, k1, t0;
  asm volatile(
      "v_and_or_b32 %2, %5, -16, %7\n\t"
      "v_and_or_b32 %3, %6, -16, %8\n\t"
      "v_med3_f32 %4, %0, %2, %3\n\t"
      "v_max3_f32 %0, %0, %2, %3\n\t"
      "v_max_f32 %1, %1, %4"
      : "+v"(p1), "+v"(p2), "=&v"(k0), "=&v"(k1), "=&v"(t0)
      : "v"(v0), "v"(v1), "n"(R0), "n"(R0 + 1));
}

// ---- level 2 -----------------------------------------------------------------------------------------
// The three-product selection (assign_fast.hip section 2b's loop order, fp16 pieces) over the points of
// the level-1 list: a tile is 32 LISTED points, their pieces gathered from the hi and mid arrays (64
// contiguous bytes per point, k-step pair and array).  The grid covers the worst case (every point listed); blocks beyond the
// list leave at once.
constexpr int kTilesR = 8;  // 32-point tiles per wave and block: 2048 listed points per block (many small blocks:
                            // the list is a few percent of the points and its length is only known on the device)
constexpr int kRefineList = kTilesR * kWaves * 32;  // points a level-2 block decides
template <int KS>
__global__ __launch_bounds__(kWaves * 64, 2) void refine_kernel(StepArgs a) {
  constexpr int FPU = 2 * KS + 1;
  constexpr int NM = 3 * KS + 1;  // MFMAs per unit
  constexpr bool PF = KS <= 4;    // the next tile's pieces prefetched into a second register set (d <= 64);
                                  // beyond, that set does not fit: the pieces are loaded when the tile is done
  typedef BlockListT<kRefineList> BL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool chunked = a.part_b != nullptr;
  const int b = chunked ? 0 : blockIdx.y, chunk = chunked ? blockIdx.y : 0;
  const int m = a.m;
  int cnt = a.count_in[b];
  cnt = cnt < m ? cnt : m;
  if ((int64_t)blockIdx.x * kTilesR * kWaves * 32 >= cnt) return;  // block-uniform
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  BL* bl = reinterpret_cast<BL*>(smem + 8 * FPU * 1024);
  if (threadIdx.x == 0) bl->n = 0;
  {
    const char* src = reinterpret_cast<const char*>(a.frags) + (size_t)b * 8 * FPU * 1024 +
                      (size_t)chunk * a.chunk_frag_stride * 16;
    for (int f = wave; f < 8 * FPU; f += kWaves)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + f * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(smem + f * 1024), 16, 0, 0);
  }
  constexpr int Q = (KS + 1) / 2;
  const int64_t slice = a.T * Q * 2048;
  const __amdgpu_buffer_rsrc_t rs_hi = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.hi) + (size_t)b * slice), 0, (int)slice, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_mid = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.mid) + (size_t)b * slice), 0, (int)slice, 0x00020000);
  const float2* __restrict__ nrm = a.norms + (int64_t)b * a.T * 32;
  const int* __restrict__ lst = a.list_in + (int64_t)b * m;
  // tile t of this wave = positions [32 tile, 32 tile + 32) of the list
  auto pos_of = [&](int t) -> int64_t { return (((int64_t)blockIdx.x * kTilesR + t) * kWaves + wave) * 32 + l31; };
  auto point_of = [&](int t) -> int {
    const int64_t pos = pos_of(t);
    return (t < kTilesR && pos < cnt) ? lst[pos] : -1;
  };
  auto voff_of = [&](int p) -> int {
    return p >= 0 ? (p >> 5) * (Q * 2048) + (p & 31) * 64 + half * 16 : 0x7ffffff0;
  };
  f16x8 xs[KS][2], xsn[PF ? KS : 1][2];
  auto load_frag = [&](int voff, auto e_c, f16x8 (&dst)[KS][2]) {
    constexpr int e = decltype(e_c)::value, st = e >> 1;
    dst[st][e & 1] = __builtin_bit_cast(
        f16x8, __builtin_amdgcn_raw_buffer_load_b128((e & 1) ? rs_mid : rs_hi, voff, (st >> 1) * 2048 + (st & 1) * 32, 0));
  };
  auto load_norm = [&](int p) -> float2 { return nrm[p >= 0 ? p : 0]; };  // (clamped, never used when p < 0)
  int p_cur = point_of(0), p_nxt = point_of(1), p_nx2 = -1, p_prev = -1;
  float2 n2cur = load_norm(p_cur), n2nxt = make_float2(0.f, 0.f), n2prev = make_float2(0.f, 0.f);
  {
    const int voff = voff_of(p_cur);
    static_for<0, 2 * KS>([&](auto e_c) { load_frag(voff, e_c, xs); });
  }
  __syncthreads();  // fragments (vmcnt(0) of the DMA) are in LDS
  const u32x4* fp = reinterpret_cast<const u32x4*>(smem) + lane;
  auto ldsf = [&](const u32x4* p) -> f16x8 { return __builtin_bit_cast(f16x8, *p); };

  f32x16 accA, accB;
#pragma unroll
  for (int r = 0; r < 16; ++r) accB[r] = -3.0e38f;
  float b1[2] = {-INFINITY, -INFINITY}, b2[2] = {-INFINITY, -INFINITY};
  int bu[2] = {0, 0};
  f16x8 c1k[KS], c2r[3];
  c1k[0] = ldsf(fp + 1 * 64);
  c2r[0] = ldsf(fp + 2 * 64);
  if constexpr (KS > 1) {
    c1k[1] = ldsf(fp + 3 * 64);
    c2r[1] = ldsf(fp + 4 * 64);
  }
  const bf16x8 bones = ones3_bf16x8(half);  // B fragment of ones at k = 0, 1, 2
  const float s = a.scale[b];
  const float cn = sqrtf(__uint_as_float(a.cmax2_bits[b * kCm])), cnr = sqrtf(__uint_as_float(a.cmax2_bits[b * kCm + 1]));
  const float c2n = a.level == 1 ? sqrtf(__uint_as_float(a.cmax2_bits[b * kCm + 2])) : -1.f;
  const bool exact_all = (a.flag[b] | a.cflag[b]) != 0;
  const float inv_s2 = (1.f / s) * (1.f / s);

  auto finish_tile = [&](int p, float2 n2, int64_t pos) {
    const int r0 = __float_as_int(b1[0]) & 15, r1 = __float_as_int(b1[1]) & 15;
    const int ia = bu[0] * 32 + (r0 & 3) + 8 * (r0 >> 2) + 4 * half;
    const int ib = bu[1] * 32 + (r1 & 3) + 8 * (r1 >> 2) + 4 * half;
    const bool tb = b1[1] > b1[0] || (b1[1] == b1[0] && ib < ia);
    int idx = tb ? ib : ia;
    const float m1 = fmaxf(b1[0], b1[1]);
    const float m2 = fmaxf(fminf(b1[0], b1[1]), fmaxf(b2[0], b2[1]));
    const float o1 = __shfl_xor(m1, 32, 64), o2 = __shfl_xor(m2, 32, 64);
    const int oi = __shfl_xor(idx, 32, 64);
    const float B1 = fmaxf(m1, o1);
    const float B2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
    if (o1 > m1 || (o1 == m1 && oi < idx)) idx = oi;
    emit(a, bl, b, lane, half == 0 && p >= 0, p, idx, B1, B2, n2, s, cn, cnr, inv_s2, exact_all, c2n,
         (int64_t)chunk * m + pos);
  };

  auto unit = [&](auto u_c, f32x16& acc, const f32x16& fin, int voff_next, const f16x8 (&xs)[KS][2],
                  f16x8 (&xsn)[PF ? KS : 1][2]) {
    constexpr int U = decltype(u_c)::value, FU = (U + 7) & 7;
    const u32x4* up = fp + U * FPU * 64;
    const u32x4* upn = fp + ((U + 1) & 7) * FPU * 64;  // the next unit (unit 0 of the next tile after 7)
    const float before0 = b1[0], before1 = b1[1];
    const f32x16 zero = zero_f32x16();
    const bf16x8 cfrag = __builtin_bit_cast(bf16x8, up[0]);
    auto fill = [&](auto mi_c) {
      constexpr int mi = decltype(mi_c)::value;
      if constexpr (mi >= 2) {  // 8 register pairs of the previous unit's values over gaps 2 .. NM - 1
        constexpr int lo = ((mi - 2) * 16) / (NM - 2), hi = ((mi - 1) * 16) / (NM - 2);
        static_for<0, 8>([&](auto q_c) {
          constexpr int q = decltype(q_c)::value;
          if constexpr (2 * q + 1 >= lo && 2 * q + 1 < hi)
            take_keys_pair<2 * q>(b1[q & 1], b2[q & 1], fin[2 * q], fin[2 * q + 1]);
        });
      }
      if constexpr (U < 4 && mi == 0 && PF) {  // the next tile's pieces: 2 KS gathered 16-byte loads over units 0..3
        constexpr int l0 = (U * 2 * KS) / 4, l1 = ((U + 1) * 2 * KS) / 4;
        static_for<l0, l1>([&](auto e_c) {
          constexpr int e = decltype(e_c)::value, st = e >> 1;
          xsn[st][e & 1] = __builtin_bit_cast(
              f16x8, __builtin_amdgcn_raw_buffer_load_b128((e & 1) ? rs_mid : rs_hi, voff_next,
                                                           (st >> 1) * 2048 + (st & 1) * 32, 0));
        });
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    // small products first: corrections (C2 a1, C1 a2), main (C1 a1), then -N
    static_for<0, KS>([&](auto s_c) {
      constexpr int st = decltype(s_c)::value;
      if constexpr (st + 2 < KS) {
        c1k[st + 2] = ldsf(up + (1 + (st + 2) * 2) * 64);
        c2r[(st + 2) % 3] = ldsf(up + (2 + (st + 2) * 2) * 64);
      }
      if constexpr (st == 0) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c2r[0], xs[0][0], zero, 0, 0, 0);
      } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c2r[st % 3], xs[st][0], acc, 0, 0, 0);
      }
      fill(std::integral_constant<int, 2 * st>{});
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c1k[st], xs[st][1], acc, 0, 0, 0);
      fill(std::integral_constant<int, 2 * st + 1>{});
    });
    c2r[0] = ldsf(upn + 2 * 64);
    if constexpr (KS > 1) c2r[1] = ldsf(upn + (2 + 2) * 64);
    static_for<0, KS>([&](auto s_c) {
      constexpr int st = decltype(s_c)::value;
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c1k[st], xs[st][0], acc, 0, 0, 0);
      if constexpr (st < 2) c1k[st] = ldsf(upn + (1 + st * 2) * 64);
      fill(std::integral_constant<int, 2 * KS + st>{});
    });
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cfrag, bones, acc, 0, 0, 0);
    fill(std::integral_constant<int, 3 * KS>{});
    bu[0] = b1[0] > before0 ? FU : bu[0];
    bu[1] = b1[1] > before1 ? FU : bu[1];
  };
  using std::integral_constant;

  bool have_prev = false;
  int t_last = 0;
  auto tile = [&](int t, f16x8 (&cur)[KS][2], f16x8 (&nxt)[PF ? KS : 1][2]) {
    const int voff_next = voff_of(p_nxt);
    n2nxt = load_norm(p_nxt);
    p_nx2 = point_of(t + 2);
    unit(integral_constant<int, 0>{}, accA, accB, voff_next, cur, nxt);
    if (have_prev) finish_tile(p_prev, n2prev, pos_of(t - 1));
    b1[0] = b1[1] = b2[0] = b2[1] = -INFINITY;
    bu[0] = bu[1] = 0;
    unit(integral_constant<int, 1>{}, accB, accA, voff_next, cur, nxt);
    unit(integral_constant<int, 2>{}, accA, accB, voff_next, cur, nxt);
    unit(integral_constant<int, 3>{}, accB, accA, voff_next, cur, nxt);
    unit(integral_constant<int, 4>{}, accA, accB, voff_next, cur, nxt);
    unit(integral_constant<int, 5>{}, accB, accA, voff_next, cur, nxt);
    unit(integral_constant<int, 6>{}, accA, accB, voff_next, cur, nxt);
    unit(integral_constant<int, 7>{}, accB, accA, voff_next, cur, nxt);
    if constexpr (!PF) static_for<0, 2 * KS>([&](auto e_c) { load_frag(voff_next, e_c, cur); });
    p_prev = p_cur;
    p_cur = p_nxt;
    p_nxt = p_nx2;
    n2prev = n2cur;
    n2cur = n2nxt;
    have_prev = true;
    t_last = t;
  };
#pragma unroll 1
  for (int t = 0; t < kTilesR; t += 2) {
    if (((int64_t)blockIdx.x * kTilesR + t) * kWaves * 32 >= cnt) break;
    tile(t, xs, xsn);
    if (t + 1 >= kTilesR || ((int64_t)blockIdx.x * kTilesR + t + 1) * kWaves * 32 >= cnt) break;
    if constexpr (PF) {
      tile(t + 1, xsn, xs);
    } else {
      tile(t + 1, xs, xsn);
    }
  }
  if (have_prev) {  // the last unit of the last tile
    const float before0 = b1[0], before1 = b1[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = (r >> 1) & 1;
      const float v = __int_as_float((__float_as_int(accB[r]) & ~15) | r);
      const float t = fminf(v, b1[c]);
      b1[c] = fmaxf(v, b1[c]);
      b2[c] = fmaxf(b2[c], t);
    }
    bu[0] = b1[0] > before0 ? 7 : bu[0];
    bu[1] = b1[1] > before1 ? 7 : bu[1];
    finish_tile(p_prev, n2prev, pos_of(t_last));
  }
  if (!chunked) flush_list(a, bl, b);
}

// ---- level 2, many centroids --------------------------------------------------------------------------
// The loop order of assign_fast.hip: a wave keeps ITS 32 listed points (hi and mid pieces, gathered once)
// in registers for the whole sweep and ALL centroid chunks stream through a double-buffered LDS ring
// (half a chunk = 4 units = 128 centroids per buffer, LDS-DMA, one barrier per half chunk); the running
// top-2 never leaves the registers.  (refine_kernel per chunk re-gathers the points for every chunk and
// leaves each wave waiting for its gathers: 2.25 ms for 8 % of 1 M points x 16 384 centroids.)
constexpr int kStreamList = kWaves * 32;

template <int KS>
__global__ __launch_bounds__(kWaves * 64, 2) void refine_stream_kernel(StepArgs a, int n_half) {
  constexpr int FPU = 2 * KS + 1;
  constexpr int NM = 3 * KS + 1;  // MFMAs per unit
  constexpr int HB = 4 * FPU * 1024;  // bytes of a half chunk of fragments
  constexpr int Q = (KS + 1) / 2;
  typedef BlockListT<kStreamList> BL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int m = a.m;
  int cnt = a.count_in[0];
  cnt = cnt < m ? cnt : m;
  if ((int64_t)blockIdx.x * kWaves * 32 >= cnt) return;  // block-uniform
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l31 = lane & 31, half = lane >> 5;
  BL* bl = reinterpret_cast<BL*>(smem + 2 * HB);
  if (threadIdx.x == 0) bl->n = 0;
  auto stage = [&](int h) {  // half chunk h -> buffer h & 1 (the fragment blocks of the chunks are contiguous)
    const char* src = reinterpret_cast<const char*>(a.frags) + (size_t)h * HB;
    char* dst = smem + (h & 1) * HB;
    for (int f = wave; f < 4 * FPU; f += kWaves)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + f * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(dst + f * 1024), 16, 0, 0);
  };
  stage(0);
  const int64_t slice = a.T * Q * 2048;
  const __amdgpu_buffer_rsrc_t rs_hi = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.hi)), 0, (int)slice, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_mid = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.mid)), 0, (int)slice, 0x00020000);
  const int64_t pos = ((int64_t)blockIdx.x * kWaves + wave) * 32 + l31;
  const int p = pos < cnt ? a.list_in[pos] : -1;
  const float2 n2 = a.norms[p >= 0 ? p : 0];
  f16x8 xs[KS][2];
  {
    const int voff = p >= 0 ? (p >> 5) * (Q * 2048) + (p & 31) * 64 + half * 16 : 0x7ffffff0;
    static_for<0, 2 * KS>([&](auto e_c) {
      constexpr int e = decltype(e_c)::value, st = e >> 1;
      xs[st][e & 1] = __builtin_bit_cast(
          f16x8, __builtin_amdgcn_raw_buffer_load_b128((e & 1) ? rs_mid : rs_hi, voff, (st >> 1) * 2048 + (st & 1) * 32, 0));
    });
  }
  auto ldsf = [&](const u32x4* q) -> f16x8 { return __builtin_bit_cast(f16x8, *q); };
  f32x16 accA, accB;
#pragma unroll
  for (int r = 0; r < 16; ++r) accB[r] = -3.0e38f;
  float b1[2] = {-INFINITY, -INFINITY}, b2[2] = {-INFINITY, -INFINITY};
  int bu[2] = {0, 0};
  f16x8 c1k[KS], c2r[3];
  const bf16x8 bones = ones3_bf16x8(half);  // B fragment of ones at k = 0, 1, 2
  const f32x16 zero = zero_f32x16();

  // unit U of the half chunk in `base`; the values of the unit before it (`fin`, global unit number gprev)
  // go through the top-2 update between the MFMAs
  auto unit = [&](auto u_c, const u32x4* base, f32x16& acc, const f32x16& fin, int gprev) {
    constexpr int U = decltype(u_c)::value;
    const u32x4* up = base + U * FPU * 64;
    const float before0 = b1[0], before1 = b1[1];
    const bf16x8 cfrag = __builtin_bit_cast(bf16x8, up[0]);
    if constexpr (U == 0) {  // the buffer is only known to have landed after the barrier: cold start
      c1k[0] = ldsf(up + 1 * 64);
      c2r[0] = ldsf(up + 2 * 64);
      if constexpr (KS > 1) {
        c1k[1] = ldsf(up + 3 * 64);
        c2r[1] = ldsf(up + 4 * 64);
      }
    }
    auto fill = [&](auto mi_c) {
      constexpr int mi = decltype(mi_c)::value;
      if constexpr (mi >= 2) {  // 8 register pairs of the previous unit's values over gaps 2 .. NM - 1
        constexpr int lo = ((mi - 2) * 16) / (NM - 2), hi = ((mi - 1) * 16) / (NM - 2);
        static_for<0, 8>([&](auto q_c) {
          constexpr int q = decltype(q_c)::value;
          if constexpr (2 * q + 1 >= lo && 2 * q + 1 < hi)
            take_keys_pair<2 * q>(b1[q & 1], b2[q & 1], fin[2 * q], fin[2 * q + 1]);
        });
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    // small products first: corrections (C2 a1, C1 a2), main (C1 a1), then -N
    static_for<0, KS>([&](auto s_c) {
      constexpr int st = decltype(s_c)::value;
      if constexpr (st + 2 < KS) {
        c1k[st + 2] = ldsf(up + (1 + (st + 2) * 2) * 64);
        c2r[(st + 2) % 3] = ldsf(up + (2 + (st + 2) * 2) * 64);
      }
      if constexpr (st == 0) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c2r[0], xs[0][0], zero, 0, 0, 0);
      } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c2r[st % 3], xs[st][0], acc, 0, 0, 0);
      }
      fill(std::integral_constant<int, 2 * st>{});
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c1k[st], xs[st][1], acc, 0, 0, 0);
      fill(std::integral_constant<int, 2 * st + 1>{});
    });
    if constexpr (U < 3) {  // the next unit of the same buffer
      const u32x4* upn = up + FPU * 64;
      c2r[0] = ldsf(upn + 2 * 64);
      if constexpr (KS > 1) c2r[1] = ldsf(upn + (2 + 2) * 64);
    }
    static_for<0, KS>([&](auto s_c) {
      constexpr int st = decltype(s_c)::value;
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c1k[st], xs[st][0], acc, 0, 0, 0);
      if constexpr (st < 2 && U < 3) c1k[st] = ldsf(up + FPU * 64 + (1 + st * 2) * 64);
      fill(std::integral_constant<int, 2 * KS + st>{});
    });
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cfrag, bones, acc, 0, 0, 0);
    fill(std::integral_constant<int, 3 * KS>{});
    bu[0] = b1[0] > before0 ? gprev : bu[0];
    bu[1] = b1[1] > before1 ? gprev : bu[1];
  };
  using std::integral_constant;
#pragma unroll 1
  for (int h = 0; h < n_half; ++h) {
    __syncthreads();  // half chunk h has landed (vmcnt(0) + barrier); everyone is done with the other buffer
    if (h + 1 < n_half) stage(h + 1);
    const u32x4* base = reinterpret_cast<const u32x4*>(smem + (h & 1) * HB) + lane;
    const int g = 4 * h;
    unit(integral_constant<int, 0>{}, base, accA, accB, g - 1);
    if (h == 0) {  // (the values processed under the very first unit were the -3e38 fill)
      b1[0] = b1[1] = b2[0] = b2[1] = -INFINITY;
      bu[0] = bu[1] = 0;
    }
    unit(integral_constant<int, 1>{}, base, accB, accA, g);
    unit(integral_constant<int, 2>{}, base, accA, accB, g + 1);
    unit(integral_constant<int, 3>{}, base, accB, accA, g + 2);
  }
  {  // the last unit's values
    const int glast = 4 * n_half - 1;
    const float before0 = b1[0], before1 = b1[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = (r >> 1) & 1;
      const float v = __int_as_float((__float_as_int(accB[r]) & ~15) | r);
      const float t = fminf(v, b1[c]);
      b1[c] = fmaxf(v, b1[c]);
      b2[c] = fmaxf(b2[c], t);
    }
    bu[0] = b1[0] > before0 ? glast : bu[0];
    bu[1] = b1[1] > before1 ? glast : bu[1];
  }
  const float s = a.scale[0];
  const float cn = sqrtf(__uint_as_float(a.cmax2_bits[0])), cnr = sqrtf(__uint_as_float(a.cmax2_bits[1]));
  const float c2n = -1.f;  // (level 2)
  const bool exact_all = (a.flag[0] | a.cflag[0]) != 0;
  const float inv_s2 = (1.f / s) * (1.f / s);
  {
    const int r0 = __float_as_int(b1[0]) & 15, r1 = __float_as_int(b1[1]) & 15;
    const int ia = bu[0] * 32 + (r0 & 3) + 8 * (r0 >> 2) + 4 * half;
    const int ib = bu[1] * 32 + (r1 & 3) + 8 * (r1 >> 2) + 4 * half;
    const bool tb = b1[1] > b1[0] || (b1[1] == b1[0] && ib < ia);
    int idx = tb ? ib : ia;
    const float m1 = fmaxf(b1[0], b1[1]);
    const float m2 = fmaxf(fminf(b1[0], b1[1]), fmaxf(b2[0], b2[1]));
    const float o1 = __shfl_xor(m1, 32, 64), o2 = __shfl_xor(m2, 32, 64);
    const int oi = __shfl_xor(idx, 32, 64);
    const float B1 = fmaxf(m1, o1);
    const float B2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
    if (o1 > m1 || (o1 == m1 && oi < idx)) idx = oi;
    emit(a, bl, 0, lane, half == 0 && p >= 0, p, idx, B1, B2, n2, s, cn, cnr, inv_s2, exact_all, c2n);
  }
  flush_list(a, bl, 0);
}

// ---- chunked runs: fold the chunks and decide -----------------------------------------------------------
// One thread per point (level 1) or per list position (level 2): the chunks' (best, second, in-chunk
// index) in chunk order -- on a tie the earlier chunk, the smaller index, stays, and the tie itself makes
// second == best: the point is listed --, then the decision of emit().  grid (ceil(m / 256))
template <int LEVEL>
__global__ __launch_bounds__(256) void decide_kernel(StepArgs a, int n_chunks) {
  const int m = a.m;
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int cnt = m;
  if (LEVEL == 2) {
    cnt = a.count_in[0];
    cnt = cnt < m ? cnt : m;
    if ((int64_t)blockIdx.x * 256 >= cnt) return;  // block-uniform
  }
  const bool valid = pos < cnt;
  const int p = valid ? (LEVEL == 1 ? (int)pos : a.list_in[pos]) : 0;
  float B1 = -INFINITY, B2 = -INFINITY;
  int idx = 0;
  if (valid)
    for (int c = 0; c < n_chunks; ++c) {
      const float2 v = a.part_b[(int64_t)c * m + pos];
      const int i = a.part_i[(int64_t)c * m + pos];
      const float n2 = fmaxf(fminf(B1, v.x), fmaxf(B2, v.y));
      idx = v.x > B1 ? c * 256 + i : idx;
      B1 = fmaxf(B1, v.x);
      B2 = n2;
    }
  const float s = a.scale[0];
  const float cn = sqrtf(__uint_as_float(a.cmax2_bits[0])), cnr = sqrtf(__uint_as_float(a.cmax2_bits[1]));
  const float2 n2 = a.norms[p];
  float n2r, n2m;
  unpack_bound_norms(n2.y, n2r, n2m);
  const float an = sqrtf(n2.x), anr = sqrtf(n2r) * s;
  const float t1 = an + cn, t2 = anr + cnr * s;
  float dropped = 0.f;
  if (LEVEL == 1) {  // (emit())
    const float a2 = sqrtf(n2m), c2 = sqrtf(__uint_as_float(a.cmax2_bits[2]));
    dropped = a2 * (2.002f * cn + c2) + 1.001f * an * c2;
  }
  float delta = 1.25f * (dropped + a.eps * t1 * t1 + a.eta * (2.f * cn + an) + a.eps_exact * t2 * t2);
  if ((a.flag[0] | a.cflag[0]) != 0) delta = INFINITY;
  if (valid) {
    a.inds[p] = idx;
    if (a.vals) a.vals[p] = (B1 - n2.x) * ((1.f / s) * (1.f / s));
  }
  const bool listed = valid && !(B1 - B2 > 2.f * delta);
  int slot;
  if (wave_append(listed, a.count, slot)) {
    a.list[slot] = p;
    // candidate route (cand_stream_kernel): every centroid at or above this may be the exact winner
    // (a flagged problem -- non-finite data, centroids beyond fp16's range: delta = inf, the keys may be inf or
    // NaN -- emits no candidates at all: gdecode_kernel sends its whole list to the exact kernel)
    if (LEVEL == 1 && a.thr && slot < a.thr_cap)
      a.thr[slot] = (a.flag[0] | a.cflag[0]) != 0
                        ? __builtin_nanf("")  // (no value compares >= NaN, not even inf)
                        : B1 - 2.f * delta - (fabsf(B1) * (1.0f / 65536.0f) + 1.0e-30f);
  }
}

// ---- host launchers (fp16_cascade.h) ----------------------------------------------------------------------
int launch_scale(const ScaleArgs& a, hipStream_t st) {
  if (a.centre) {
    hipLaunchKernelGGL(mu_kernel, dim3(a.d, a.l), dim3(256), 0, st, a.B, a.mu, a.d, a.n);
    TPQ_LAUNCH_CHECK("lloyd mu_kernel");
  }
  int chunks = (int)(a.budget / ((int64_t)a.l * a.d));
  if (chunks < 1) chunks = 1;
  if ((int64_t)chunks * 4096 > a.m) chunks = (int)((a.m + 4095) / 4096);
  hipLaunchKernelGGL(maxabs_kernel, dim3(chunks, a.d, a.l), dim3(256), 0, st, a.A, a.mu, a.maxbits, a.flag, a.d, a.m,
                     a.sample);
  TPQ_LAUNCH_CHECK("lloyd maxabs_kernel");
  hipLaunchKernelGGL(scale_kernel, dim3((a.l + 63) / 64), dim3(64), 0, st, a.maxbits, a.flag, a.scale, a.l, a.headroom);
  TPQ_LAUNCH_CHECK("lloyd scale_kernel");
  return TPQ_OK;
}

int launch_split(const float* A, char* prep, const PrepLayout& P, int l, int d, int64_t m, hipStream_t st) {
  hipLaunchKernelGGL(split_kernel, dim3((unsigned)((P.T + 7) / 8), l), dim3(256), 0, st, A,
                     reinterpret_cast<const float*>(prep + P.mu_off), reinterpret_cast<const float*>(prep + P.scale_off),
                     reinterpret_cast<u32x4*>(prep + P.hi_off), reinterpret_cast<u32x4*>(prep + P.mid_off),
                     reinterpret_cast<float2*>(prep + P.norms_off), reinterpret_cast<int*>(prep + P.flag_off), d, m, P.T,
                     P.KS);
  TPQ_LAUNCH_CHECK("lloyd split_kernel");
  return TPQ_OK;
}

int launch_cprep(const float* B, const float* mu, const float* scale, u32x4* frags, unsigned* cmax2_bits, int* cflag,
                 int l, int d, int n, int chunks, int KS, hipStream_t st) {
  hipLaunchKernelGGL(cprep_kernel, dim3(8 * chunks, l), dim3(64), 0, st, B, mu, scale, frags, cmax2_bits, cflag, d, n, KS);
  TPQ_LAUNCH_CHECK("lloyd cprep_kernel");
  return TPQ_OK;
}

int launch_coarse(int KS, const StepArgs& sa, int grid_y, hipStream_t st) {
  const int64_t wide = (sa.T + 1) / 2, per_block = (int64_t)kWaves * kWide;
  const dim3 grid((unsigned)((wide + per_block - 1) / per_block), grid_y);
  return dispatch_ks<8>(KS, [&](auto ks) -> int {
    constexpr int K = decltype(ks)::value;
    return launch_with_lds(coarse_kernel<K>, "lloyd coarse_kernel", grid, dim3(kWaves * 64),
                           (size_t)8 * (K + 1) * 1024 + sizeof(BlockListT<kCoarseList>), st, sa);
  });
}

int launch_refine(int KS, const StepArgs& sa, int grid_y, hipStream_t st) {
  const int64_t per_block = (int64_t)kWaves * kTilesR;
  const dim3 grid((unsigned)((sa.T + per_block - 1) / per_block), grid_y);
  return dispatch_ks<8>(KS, [&](auto ks) -> int {
    constexpr int K = decltype(ks)::value;
    return launch_with_lds(refine_kernel<K>, "lloyd refine_kernel", grid, dim3(kWaves * 64),
                           (size_t)8 * (2 * K + 1) * 1024 + sizeof(BlockListT<kRefineList>), st, sa);
  });
}

int launch_refine_stream(int KS, const StepArgs& sa, int n_half, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)sa.m + kWaves * 32 - 1) / (kWaves * 32)));
  return dispatch_ks<8>(KS, [&](auto ks) -> int {
    constexpr int K = decltype(ks)::value;
    return launch_with_lds(refine_stream_kernel<K>, "lloyd refine_stream_kernel", grid, dim3(kWaves * 64),
                           (size_t)2 * 4 * (2 * K + 1) * 1024 + sizeof(BlockListT<kStreamList>), st, sa, n_half);
  });
}

int launch_decide_level1(const StepArgs& sa, int n_chunks, hipStream_t st) {
  hipLaunchKernelGGL(decide_kernel<1>, dim3((unsigned)(((int64_t)sa.m + 255) / 256)), dim3(256), 0, st, sa, n_chunks);
  TPQ_LAUNCH_CHECK("lloyd decide_kernel");
  return TPQ_OK;
}

}  // namespace lloyd
}  // namespace tpq
