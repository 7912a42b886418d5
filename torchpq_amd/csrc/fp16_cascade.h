// What the units of the fp16 cascade share -- cascade_core.hip (the preparation and the level kernels, each compiled
// once, there), lloyd.hip (the Lloyd step), assign_cascade.hip (the coarse assign), probe_sims.hip (the coarse probe):
// types, layouts, the level kernels' arguments, device helpers of more than one unit's kernels, the host launchers
// of the shared kernels and the hooks other units call.  All work on centred, scaled, split data (lloyd.hip):
//   a' = s (x - mu) = h + m + rho,  c' = s (c - mu),  h = fp16(a'), m = fp16(a' - h),  |rho| <= 2^-22 |a'| + eta
//
// Selection (same scheme as assign_fast.hip section 2b, re-derived for fp16; all in scaled-centred
// units): per 32 x 32 tile  f = sum_k (C2 a1 + C1 a2 + C1 a1) - N  on v_mfma_f32_32x32x16_f16 (C = 2 c'
// split the same way; small products first) and one bf16 MFMA for N = fl |c'|^2 (three exact bf16
// pieces against ones);  g = 2 a'.c' - |c'|^2 is what the real-number distance orders by.
//   |f - g| <= [3.03 2^-22 + (16 KS + 13) 2^-23 + (d + 1) 2^-24] (|a'| + |c'|max)^2      dropped
//              products, worst-case fp32 accumulation of all MFMA terms, the norm chain
//            + 2^-22 (|a'| + |c'|max)^2                          rounding of x - mu, c - mu
//            + eta sqrt(d) (2 |c'|max + |a'|),  eta = 2^-13     fp16 subnormals, flushed or not
//            + s^2 (d + 4) 2^-24 (|x| + |c|max)^2                the exact fp32 chain's own rounding
// delta = 1.25 x that.  A point whose two best fast values differ by more than 2 delta has its
// label decided -- the arg-max of tpq_max_sim, bit for bit; the others are listed and re-evaluated
// by the exact fp32-MFMA kernel (launch_max_sim_list, max_sim.hip) on the raw data.
#pragma once
#include "mfma_util.h"

#define TPQ_LOCAL __attribute__((visibility("hidden")))  // crosses units, but is no part of the library's surface

namespace tpq {
int launch_max_sim_list(const float* A, const float* B, float* vals, int64_t* inds, int l, int d, int m, int n,
                        int euclid, const int* list, const int* count, unsigned long long* keys, float* Ac, int cap,
                        hipStream_t st);  // max_sim.hip
// tpq_coarse_assign (assign_fast.hip) -> assign_cascade.hip: one problem with many centroids through the cascade
// (euclidean, d <= 128), and the GEMM-shaped cascade of wide vectors (128 < d <= 1024)
int lloyd_assign_supported(int d, int64_t m, int n, int route);
size_t lloyd_assign_workspace_bytes(int d, int64_t m, int n);
size_t lloyd_assign_count_offset(int d, int64_t m, int n);
int lloyd_wide_supported(int d, int64_t m, int n);
int lloyd_assign(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n, int euclid, char* ws,
                 hipStream_t st);
namespace lloyd {

constexpr int kWaves = 8;
constexpr int kMu = 128;  // floats per sub-problem in the centring table (d <= 128)
#ifndef TPQ_LL_TILES
#define TPQ_LL_TILES 32
#endif
constexpr int kTiles = TPQ_LL_TILES;  // 32-point tiles per wave and block
constexpr int kWide = kTiles / 2;     // wide tiles (64 points, level 1) per wave and block
static int ks_of(int d) { return (d + 15) / 16; }

// f(std::integral_constant<int, KS>{}) for the run-time KS in [1, MAX] (beyond: MAX): picks a template instance
template <int MAX, class F>
static int dispatch_ks(int KS, F&& f) {
  if constexpr (MAX > 1) {
    if (KS < MAX) return dispatch_ks<MAX - 1>(KS, f);
  }
  return f(std::integral_constant<int, MAX>{});
}

// ---- prepared block --------------------------------------------------------------------------
struct PrepLayout {
  int KS;
  int64_t T;  // 32-point tiles per sub-problem
  size_t hi_off, mid_off, norms_off, mu_off, scale_off, flag_off, maxbits_off, total;
};
static PrepLayout prep_layout(int l, int d, int64_t m) {
  PrepLayout L;
  L.KS = ks_of(d);
  L.T = (m + 31) / 32;
  // hi and mid pieces in two arrays [l][T tiles][Q = ceil(KS / 2) k-step pairs][32 points][64 B]: a point's
  // 32 dimensions of a k-step pair are 64 contiguous bytes -- chunk 2 (st % 2) + half is what lane (point,
  // half) of the B operand of k-step st reads.  The coarse pass streams the hi array only; the update
  // streams one pair per wave; level 2 gathers a listed point as Q 64-byte pieces per array.  (Plain
  // MFMA-fragment order -- tile x k-step x lane x 16 B -- scatters a point over 16 cache lines: 1 KiB of
  // traffic per gathered point, level 2 at 1.6 ms instead of 0.6; plain row-major -- one 32 KS-byte row
  // per point -- makes every 64-lane load touch 32 lines: the streaming kernels turn address-unit-bound,
  // the update at 4.75 ms.  Here a 64-lane load touches 16 lines and uses half of each.)
  L.hi_off = 0;
  L.mid_off = (size_t)l * L.T * ((L.KS + 1) / 2) * 2048;
  L.norms_off = 2 * L.mid_off;
  L.mu_off = L.norms_off + (size_t)l * L.T * 32 * 8;       // [l][T * 32] float2
  L.scale_off = L.mu_off + (size_t)l * kMu * 4;            // [l][kMu] f32
  L.flag_off = L.scale_off + (size_t)l * 4;                // [l] f32
  L.maxbits_off = L.flag_off + (size_t)l * 4;              // [l] i32
  L.total = (L.maxbits_off + (size_t)l * 4 + 255) / 256 * 256;
  return L;
}

constexpr int kCm = 4;  // words per sub-problem in cmax2_bits: max N, max |c|^2, max |C - Ch|^2, -

// Level 1's keys carry 6 bits -- register number + 16 x (unit mod 4) -- so that the unit of the best value
// needs no bookkeeping of its own (which half of the tile's units it came from is one compare per tile).
// 2^-17 |v| off: in level 1's bound.
// The tagging itself is plain C++ (the compiler selects v_and_or_b32): these instructions READ MFMA
// results right behind the MFMAs, and the wait states that takes are only inserted for instructions
// the hazard recogniser can see -- as operands of an asm block the accumulators were read too early
// (labels wrong, differently on every run).
template <int TAG>
__device__ __forceinline__ float key6(float v) {
  return __int_as_float((int)((__float_as_uint(v) & 0xffffffc0u) | (unsigned)TAG));
}
__device__ __forceinline__ void top2_keys_pair(float& p1, float& p2, float k0, float k1) {
  float t0;
  asm volatile(
      "v_med3_f32 %2, %0, %3, %4\n\t"
      "v_max3_f32 %0, %0, %3, %4\n\t"
      "v_max_f32 %1, %1, %2"
      : "+v"(p1), "+v"(p2), "=&v"(t0)
      : "v"(k0), "v"(k1));
}

// ---- the cascade on prepared pieces ------------------------------------------------------------------
// Level 1 (coarse_kernel): ONE product per k-step -- f0 = sum_k Ch ah - N on the hi pieces only (half the
// bytes, 5 MFMAs per 32 x 32 tile instead of 13).  |f0 - g| carries the dropped pieces,
//   (2^-11 + 2^-23) (|a'| + |c'|max)^2      (|a - ah| <= 2^-11 |a|, |C - Ch| <= 2^-11 |C|, 2 |c'||a'| <= (.)^2 / 2)
// in place of 3.03 2^-22 (.)^2: the bound is ~36x wider and 5-13 % of the points stay undecided.
// Level 2 (refine_kernel): those points, gathered through the level-1 list, with all three products
// (the bound of the header comment): 0.2-0.7 % stay undecided.
// Level 3: the exact fp32 kernel over the level-2 list (launch_max_sim_list, max_sim.hip).
// Every level decides a point only when its two best fast values are further apart than twice its
// own rigorous bound, so the labels are tpq_max_sim's whatever the split between the levels.
struct StepArgs {
  const u32x4* hi;             // [l][T][Q][32 points][64 B]
  const u32x4* mid;            // likewise
  const float2* norms;         // [l][T * 32]: (|a'|^2, |x|^2)
  const u32x4* frags;          // [l][8][2 KS + 1][64]
  const unsigned* cmax2_bits;  // [l][kCm]: max N, max |c|^2, max |C - Ch|^2
  const float* scale;          // [l]
  const int* flag;             // [l] data not finite / out of range (prepare)
  const int* cflag;            // [l] centroids out of fp16 range (this iteration)
  int64_t* inds;               // [l][m]
  float* vals;                 // optional [l][m]
  const int* list_in;          // level 2: [l][m] points to refine, count_in [l]
  const int* count_in;
  int* list;                   // [l][m] points this level leaves undecided
  int* count;                  // [l]
  int m;
  int64_t T;
  float eps, eps_exact, eta;   // eps: this level's fast-path bound, relative to (|a'| + |c'|max)^2; eta times sqrt(d)
  int level;                   // 1: the dropped pieces are bounded per point (emit), on top of eps
  float* thr;                  // chunked level 1, candidate route: [thr_cap] threshold of the listed point (or null)
  int thr_cap;
  // more than 256 centroids (tpq_coarse_assign): blockIdx.y = CHUNK of 256 centroids (all chunks in one
  // launch: one chunk's blocks alone fill half the chip); a chunk's (best, second) and in-chunk index of
  // every point go to part_*[chunk][point or list position], decide_kernel folds the chunks and decides
  float2* part_b;              // [chunks][m]  (nullptr: a single chunk, decided in the kernel)
  uint8_t* part_i;             // [chunks][m]
  int chunk_frag_stride;       // 16-byte units between the fragment blocks of consecutive chunks
};

// the fast-path bounds of level 1 / level 2, relative to (|a'| + |c'|max)^2
static float level_eps(int KS, int d, int level) {
  const int terms = KS * 16 + 2 + 3;
  const float common = (float)(terms + 8) / 8388608.0f + (float)(d + 1) / 16777216.0f + 1.0f / 4194304.0f +
                       1.0f / 524288.0f;  // accumulation, norm chain, shift rounding, key bits
  return level == 1 ? common + 1.0f / 131072.0f  // (the dropped pieces: per point, emit()); 6-bit keys: 2^-17
                    : 3.03f / 4194304.0f + common;
}

// ---- host launchers of the kernels of cascade_core.hip (KS at run time) -----------------------------------
// The start of every preparation: mu = mean of the centroids B (centre; else mu stays as it is: zero), max |x - mu| over A
// in `budget` / (l d) blocks per row, the power-of-two scale.  The split that follows is the caller's next line.
struct ScaleArgs {
  const float* A;  // [l][d][m]
  int64_t m;
  const float* B;  // [l][d][n]
  int n, l, d;
  int budget;            // 4096 or 8192: as each path was tuned
  int sample, headroom;  // maxabs_kernel, scale_kernel
  bool centre;
  float* mu;
  unsigned* maxbits;
  int* flag;  // (the probe's centroids: their cflag)
  float* scale;
};
TPQ_LOCAL int launch_scale(const ScaleArgs& a, hipStream_t st);
// split_kernel over a prepared block of layout P at `prep` (mu, scale and flag inside it)
TPQ_LOCAL int launch_split(const float* A, char* prep, const PrepLayout& P, int l, int d, int64_t m, hipStream_t st);
// cprep_kernel: grid (8 chunks, l)
TPQ_LOCAL int launch_cprep(const float* B, const float* mu, const float* scale, u32x4* frags, unsigned* cmax2_bits,
                           int* cflag, int l, int d, int n, int chunks, int KS, hipStream_t st);
// the levels; grid_y = sub-problems, or chunks of 256 centroids when sa.part_b is set
TPQ_LOCAL int launch_coarse(int KS, const StepArgs& sa, int grid_y, hipStream_t st);
TPQ_LOCAL int launch_refine(int KS, const StepArgs& sa, int grid_y, hipStream_t st);
TPQ_LOCAL int launch_refine_stream(int KS, const StepArgs& sa, int n_half, hipStream_t st);
TPQ_LOCAL int launch_decide_level1(const StepArgs& sa, int n_chunks, hipStream_t st);

}  // namespace lloyd
}  // namespace tpq
