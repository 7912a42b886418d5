// One Lloyd iteration of MultiKMeans.fit on PREPARED data (tpq_lloyd_prepare / tpq_lloyd_step):
// the PQ-codebook training shape -- l sub-problems, n <= 256 centroids, d <= 64 (configs[4]).
// Replaces, per iteration, the pair  get_labels -> compute_centroids  of the reference's driver
// (torchpq/clustering/MultiKMeans.py:415-453: max_sim_tn torchpq/kernels/cuda/max_sim.cu:182-309 +
// compute_centroids torchpq/kernels/cuda/compute_centroids.cu:10-86).
//
// What "prepared" buys.  The data of a fit() never changes, only the centroids do,
// yet tpq_max_sim_select re-reads the fp32 points every iteration and spends a third of its
// instructions centring and splitting them.  tpq_lloyd_prepare does it ONCE per fit:
//   a' = s (x - mu)          mu = mean of the initial centroids (distances are translation-
//                            invariant; any fixed shift works), s = the power of two that puts
//                            max |x - mu| of the sub-problem in [2^13, 2^14)
//   a' = h + m + rho         h = fp16(a'), m = fp16(a' - h):  |rho| <= 2^-22 |a'| + eta
// and stores (h, m) in MFMA-fragment order -- tile of 32 points x k-step x piece x lane x 16 B, 4 bytes
// per element, exactly the bytes of the fp32 original -- plus |a'|^2 and |x|^2 per point.  A tile's
// B operands are then eight 16-byte loads per lane, no VALU work at all.
// fp16 pieces instead of the bf16 pieces of assign_fast.hip: two fp16 pieces carry 22 significant
// bits (two bf16: 16), so the dropped products shrink from 3 x 2^-16 to 3 x 2^-22 and the bound of the
// selection by ~4x -- a quarter of the points go to the exact re-check -- and h + m is precise
// enough (2^-22 relative: two ulps of fp32) to feed the centroid UPDATE from the same bytes.  The
// price is fp16's range: hence the per-sub-problem scale, the overflow / non-finite flags (a
// flagged sub-problem sends every point to the exact path) and eta below.
//
// The selection (three levels, each deciding only what its rigorous bound allows: the labels are tpq_max_sim's, bit for
// bit) is shared with the coarse assign and the coarse probe: fp16_cascade.h (the bound), cascade_core.hip (the kernels).
#include <stdlib.h>

#include "fp16_cascade.h"

namespace tpq {
namespace lloyd {

#ifndef TPQ_LL_PF
#define TPQ_LL_PF 0  // update kernel: tiles ahead of an L2 prefetch by LDS-DMA (0 = none; see the kernel)
#endif

// ---- update from the pieces -------------------------------------------------------------------------
// sums[cluster][dim] = sum_i onehot(label_i)[cluster] * (h_i + m_i)[dim] on v_mfma_f32_32x32x16_f16 (exact
// products 1.0 * piece, fp32 sums: x is represented to 2^-22 relative, two ulps of fp32; the sums are
// of the centred, scaled values s (x - mu), undone by finalize).  Against centroid_accum_mfma_kernel
// (max_sim.hip) on the fp32 data: no splitting (it spends ~6.5 VALU instructions per element on three
// bf16 pieces), no LDS staging of the data, 64 + 8 MFMAs per 32 points x 64 dimensions instead of 96.
// The pieces are stored point-major (a lane of the assign kernels = one point, 8 dimensions); the
// update contracts over POINTS, so its B operand wants lane = dimension, 8 points.  The transposition
// runs on the matrix pipe: D = X I with the piece fragment as A (row = point, k = 16 dimensions)
// and an identity slice as B puts X[point][dim] into the accumulator layout -- lane = column = dimension,
// registers = rows = points -- exactly (one non-zero product per sum); eight v_cvt_pkrtz pack each
// 16 registers into the two k-steps' B fragments.  Point of k-slot i of k-group g in k-step s:
// 16 s + (i & 3) + 8 (i >> 2) + 4 g (the accumulator's row order) -- the one-hot operand uses the same.
// One wave owns 256 clusters x 32 dimensions (128 accumulator registers); the block's waves are the
// dimension tiles of the SAME points (their loads hit the same cache lines together).
struct UpdArgs {
  const u32x4* hi;
  const u32x4* mid;
  const int64_t* labels;  // [l][m]
  const int* flag;        // [l]: flagged sub-problems are skipped here (flagged_accum_kernel)
  float* sums;            // [l][d][k]
  float* counts;          // [l][k]
  int d, k, m;
  int64_t T;
};

// Wave (dt, ch) of a block owns dimensions [32 dt, 32 dt + 32) x clusters [128 ch, 128 ch + 128): 64
// accumulator registers, ~150 VGPRs in all -> three waves per SIMD.  (256 clusters per wave -- 128
// accumulator registers, two waves per SIMD -- ran 4.75 ms at C5: with one staging set a wave has one
// tile's loads in flight half of the time, 2048 waves x ~2 KiB, a third of what HBM latency x bandwidth
// asks for; a second or third staging set does not fit beside 128 accumulator registers -- 116 / 465
// spilled.  The four waves of a block read the same rows: one trip to HBM, the rest from L2 / L1.)
// NH = cluster halves per dimension tile (1: a wave owns all 256 clusters, 128 accumulator registers, two
// waves per SIMD; 2: 128 clusters, three waves per SIMD)
// (Round 5, same box, C5: one extra dword load per wave and tile touching the 32 cache lines of the tile two / four steps
// on -- to start their trip from HBM early, since a wave has one tile's fragments in flight -- made the update SLOWER:
// 3.85 -> 4.0 / 5.0 ms.  The kernel is not waiting on HBM latency: matrix pipe 41 % busy, 46 % of the wave cycles issuing,
// profiles/r04_c5.json; its time is the per-tile chain load -> transposing MFMAs -> pack -> one-hot rows through LDS -> MFMAs
// of two waves per SIMD, and more requests on the memory path lengthen it.)
template <int KS, int NH>
__global__ __launch_bounds__(64 * NH * ((KS + 1) / 2), (NH == 1 ? 2 : 3)) void update_kernel(UpdArgs a) {
  constexpr int DT = (KS + 1) / 2;
  constexpr int NW = NH * DT;
  constexpr int CW = 256 / NH, RT = 8 / NH;  // clusters / row tiles per wave
  __shared__ __attribute__((aligned(16))) uint16_t otab_s[NW][2 * CW * 8];  // [k-group][cluster][8 slots] fp16
  __shared__ int cnt_s[NW][CW];
  const int b = blockIdx.y;
  if (a.flag[b]) return;
  const int wave = threadIdx.x >> 6, dt = wave / NH, ch = wave % NH;
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  uint16_t* otab = otab_s[wave];
  int* cnt = cnt_s[wave];
  const int64_t slice = a.T * DT * 2048;
  const __amdgpu_buffer_rsrc_t rs_hi = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.hi) + (size_t)b * slice), 0, (int)slice, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_mid = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(a.mid) + (size_t)b * slice), 0, (int)slice, 0x00020000);
  const int64_t* __restrict__ lrow = a.labels + (int64_t)b * a.m;
  f32x16 acc[RT];  // [cluster row tile] x this wave's 32 dimensions
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
#pragma unroll
  for (int u = 0; u < CW / 64; ++u) cnt[lane + 64 * u] = 0;
#pragma unroll
  for (int u = 0; u < CW / 32; ++u) reinterpret_cast<u32x4*>(otab)[lane + 64 * u] = u32x4{0u, 0u, 0u, 0u};
  // identity slices: B[k][j] = (j == 16 ks2 + k), lane (j = l31, k-group half) holds k = 8 half .. + 7
  f16x8 ident[2];
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
    for (int i = 0; i < 8; ++i) ident[ks2][i] = (l31 == 16 * ks2 + 8 * half + i) ? (_Float16)1.0f : (_Float16)0.0f;
  // **The points of a tile are taken in the order of their clusters.**  A k-step of 16 random labels
  // touches 7 of the 8 cluster row tiles, so the one-hot multiply runs 8 x 2 MFMAs per k-step for 16
  // non-zero rows; with the tile's 32 points SORTED by label the first k-step holds the lower half of
  // the labels and the second the upper half -- 4 to 5 row tiles each -- and the row tiles outside
  // [first label, last label] of the k-step are skipped (wave-uniform branches): 4 + 2 x ~4.5 x 2 = 22
  // MFMAs per tile instead of 36.  The permutation costs nothing to apply: a lane loads the fragment of the
  // point of its SORTED position (the loads are per-lane addressed anyway), so the transposed pieces come
  // out in sorted order.  Cost: the labels of a tile are needed before its pieces (they are fetched three
  // steps ahead) and the grouping below, one step ahead, behind the MFMAs.
  constexpr unsigned kBad = 256u << 5;  // key of a point that is not this wave's (sorts last, row tile 8)
  // (grouping by cluster ROW TILE is all the skipping needs: a counting sort over the 9 row-tile values --
  // one ballot + two popcounts each -- and ONE ds_permute, instead of a 15-stage bitonic network whose
  // dependent cross-lane round trips cost more than the MFMAs they saved: 3.8 vs 3.5 ms at C5)
  auto sort32 = [&](unsigned key) -> unsigned {
    const unsigned rt = key >> 10;  // 0..7, 8 = not this wave's point
    const unsigned below_me = (1u << l31) - 1u;
    unsigned pos = 0, base = 0;
#pragma unroll
    for (unsigned r = 0; r <= 8; ++r) {
      const unsigned m32 = (unsigned)__ballot(rt == r);  // lanes 0..31 (32..63 hold the same points)
      pos = rt == r ? base + __popc(m32 & below_me) : pos;
      base += __popc(m32);
    }
    // lane `pos` (of the same half-wave) receives this lane's key
    return (unsigned)__builtin_amdgcn_ds_permute((int)((pos + 32 * half) * 4), (int)key);
  };
  // raw label of point l31 of `tile` (int64, clamped address: validity is applied when it is used)
  auto load_label = [&](int64_t tile) -> int64_t {
    const int64_t p = tile * 32 + l31;
    return lrow[(tile < a.T && p < a.m) ? p : 0];
  };
  auto key_of = [&](int64_t tile, int64_t label) -> unsigned {
    const int64_t p = tile * 32 + l31;
    const int64_t rel = label - CW * ch;  // this wave's clusters only: label - CW ch in [0, CW)
    const bool ok = tile < a.T && p < a.m && label < a.k && rel >= 0 && rel < CW;
    return ok ? (((unsigned)rel << 5) | (unsigned)l31) : (kBad | (unsigned)l31);
  };
  f16x8 x[2][2];  // [piece][k-step of the pair] of the tile in flight, rows in sorted order
  auto load_pieces = [&](int64_t tile, unsigned skey) {
    // lane (sorted position l31, half) takes the fragment of point (skey & 31) of the tile
    const int voff = tile < a.T ? (int)((tile * DT + dt) * 2048) + (int)(skey & 31u) * 64 + half * 16 : 0x7ffffff0;
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      x[0][ks2] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_hi, voff, ks2 * 32, 0));
      x[1][ks2] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_mid, voff, ks2 * 32, 0));
    }
  };
  const f32x16 zero = zero_f32x16();
  // tiles dealt round-robin to the blocks of a sub-problem (adjacent rows are read side by side).  A
  // tile's fragments are consumed by its four transposing MFMAs right at the start; the loads of the
  // next tile go into the same registers immediately afterwards.
  const int64_t step = gridDim.x;
  unsigned skey = sort32(key_of(blockIdx.x, load_label(blockIdx.x)));  // sorted keys of the tile in flight
  load_pieces(blockIdx.x, skey);
  unsigned skey_n1 = sort32(key_of(blockIdx.x + step, load_label(blockIdx.x + step)));  // ... of the next tile
  int64_t lab_n2 = load_label(blockIdx.x + 2 * step);                  // raw labels of the tile after that
#pragma unroll 1
  for (int64_t tile = blockIdx.x; tile < a.T; tile += step) {
    const unsigned rt_mine = skey >> 10;                       // cluster row tile of this lane's point (8: none)
    const int lab = skey < kBad ? (int)(skey >> 5) : -1;
    // transposition: [32 points][32 dims] of each piece into accumulator layout, packed at once into the
    // two k-steps' B fragments (one piece at a time: 16 transient registers)
    u32x4 bop[2][2];  // [piece][k-step of 16 points], fp16 pairs
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      f32x16 tr = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[pc][0], ident[0], zero, 0, 0, 0);
      tr = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[pc][1], ident[1], tr, 0, 0, 0);
#pragma unroll
      for (int sk = 0; sk < 2; ++sk)
#pragma unroll
        for (int i = 0; i < 4; ++i)  // (exact: every value IS an fp16 number)
          bop[pc][sk][i] = __builtin_bit_cast(
              uint32_t, __builtin_amdgcn_cvt_pkrtz(tr[8 * sk + 2 * i], tr[8 * sk + 2 * i + 1]));
    }
    __builtin_amdgcn_sched_barrier(0);
    // the next tile's pieces, in the order sorted during the previous step (the fragments are free now)
    load_pieces(tile + step, skey_n1);
    __builtin_amdgcn_sched_barrier(0);
    if (dt == 0 && half == 0 && lab >= 0) atomicAdd(&cnt[lab], 1);  // integer LDS atomic: fast
    // this lane's point (sorted position l31; half 0 lanes write): k-step l31 >> 4, k-group (l31 >> 2) & 1,
    // slot (l31 & 3) + 4 ((l31 >> 3) & 1)
    uint16_t* oslot = &otab[((l31 >> 2) & 1) * (CW * 8) + (lab >= 0 ? lab : 0) * 8 + (l31 & 3) + 4 * ((l31 >> 3) & 1)];
#pragma unroll
    for (int sk = 0; sk < 2; ++sk) {
      // row tiles of this k-step's 16 (sorted) points: [lo, hi]; invalid points sort last (row tile 8)
      const int lo = (int)__builtin_amdgcn_readlane((int)rt_mine, 16 * sk);
      int hi = (int)__builtin_amdgcn_readlane((int)rt_mine, 16 * sk + 15);
      hi = hi < RT ? hi : RT - 1;
      const bool writer = half == 0 && (l31 >> 4) == sk && lab >= 0;
      if (writer) *oslot = (uint16_t)0x3C00;  // fp16 1.0
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const f16x8* orow = reinterpret_cast<const f16x8*>(&otab[half * (CW * 8) + l31 * 8]);
      f16x8 aop[RT];  // all A operands of the k-step are requested before its first MFMA
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        if (rt >= lo && rt <= hi) aop[rt] = orow[32 * rt];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        if (rt >= lo && rt <= hi) {
          acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aop[rt], __builtin_bit_cast(f16x8, bop[0][sk]), acc[rt], 0, 0, 0);
          acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aop[rt], __builtin_bit_cast(f16x8, bop[1][sk]), acc[rt], 0, 0, 0);
        }
      __builtin_amdgcn_wave_barrier();
      if (writer) *oslot = (uint16_t)0;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    // the tile two steps on: sort its labels (fetched a step ago) -- 15 dependent cross-lane stages, behind
    // this tile's MFMAs and in front of nothing: the pieces just requested have that long to land -- and
    // fetch the labels of the tile three steps on
    skey = skey_n1;
    skey_n1 = sort32(key_of(tile + 2 * step, lab_n2));
    lab_n2 = load_label(tile + 3 * step);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int dim = 32 * dt + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cluster = CW * ch + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float v = acc[rt][r];
      if (dim < a.d && cluster < a.k && v != 0.f) unsafeAtomicAdd(&a.sums[((int64_t)b * a.d + dim) * a.k + cluster], v);
    }
  }
  if (dt == 0) {
#pragma unroll
    for (int u = 0; u < CW / 64; ++u) {
      const int c = lane + 64 * u;
      if (CW * ch + c < a.k && cnt[c]) unsafeAtomicAdd(&a.counts[(int64_t)b * a.k + CW * ch + c], (float)cnt[c]);
    }
  }
}

// flagged sub-problems (data not finite / out of the fp16 range): raw fp32 sums straight to global atomics
// (each point confined to its own cluster, as compute_centroids.cu:10-86 has it).  grid (64, l): the
// blocks of an unflagged sub-problem leave at once (a grid over all points x dimensions was 16 M
// empty blocks: 3.7 ms)
__global__ __launch_bounds__(256) void flagged_accum_kernel(const float* __restrict__ data,
                                                           const int64_t* __restrict__ labels,
                                                           const int* __restrict__ flag, float* __restrict__ sums,
                                                           float* __restrict__ counts, int d, int m, int k) {
  const int b = blockIdx.y;
  if (!flag[b]) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const int64_t lab = labels[(int64_t)b * m + i];
    if (lab < 0 || lab >= k) continue;
    unsafeAtomicAdd(&counts[(int64_t)b * k + lab], 1.0f);
    for (int e = 0; e < d; ++e)
      unsafeAtomicAdd(&sums[((int64_t)b * d + e) * k + lab], data[((int64_t)b * d + e) * m + i]);
  }
}

// centroid = mu + (sums / count) / s (raw sums / count for flagged sub-problems); empty cluster -> 0
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ sums, const float* __restrict__ counts,
                                                      const float* __restrict__ mu, const float* __restrict__ scale,
                                                      const int* __restrict__ flag, float* __restrict__ out, int d,
                                                      int k, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int c = (int)(t % k);
  const int dim = (int)((t / k) % d);
  const int64_t b = t / ((int64_t)d * k);
  const float cnt = counts[b * k + c];
  float v = 0.f;  // compute_centroids.cu:82
  if (cnt != 0.f) v = flag[b] ? sums[t] / cnt : mu[b * kMu + dim] + (sums[t] / cnt) * (1.f / scale[b]);
  out[t] = v;
}

template <int KS>
static int run_update(const UpdArgs& ua, const float* data, const float* mu, const float* scale, float* out, int l,
                      hipStream_t st) {
  constexpr int DT = (KS + 1) / 2;
  // one round of resident waves: every wave ends with its (256 / NH) x 32 global atomics
  const char* e = TPQ_AB_ENV("TPQ_LL_NH");  // (variant builds, A/B)
  const int nh = e ? atoi(e) : 1;
  int64_t chunks = (nh == 1 ? 2048 : 3072) / ((int64_t)l * nh * DT);
  if (chunks < 1) chunks = 1;
  if (chunks > ua.T) chunks = ua.T;
  if (nh == 1)
    hipLaunchKernelGGL((update_kernel<KS, 1>), dim3((unsigned)chunks, l), dim3(64 * DT), 0, st, ua);
  else
    hipLaunchKernelGGL((update_kernel<KS, 2>), dim3((unsigned)chunks, l), dim3(128 * DT), 0, st, ua);
  TPQ_LAUNCH_CHECK("lloyd update_kernel");
  hipLaunchKernelGGL(flagged_accum_kernel, dim3(64, l), dim3(256), 0, st, data,
                     ua.labels, ua.flag, ua.sums, ua.counts, ua.d, ua.m, ua.k);
  TPQ_LAUNCH_CHECK("lloyd flagged_accum_kernel");
  const int64_t total = (int64_t)l * ua.d * ua.k;
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ua.sums, ua.counts, mu,
                     scale, ua.flag, out, ua.d, ua.k, total);
  TPQ_LAUNCH_CHECK("lloyd finalize_kernel");
  return TPQ_OK;
}

// ---- step workspace --------------------------------------------------------------------------------
struct StepLayout {
  size_t frags_off, cmax_off, count_off, cflag_off, count2_off, list_off, list2_off, upd_off, total;
};
static StepLayout step_layout(int l, int d, int64_t m, int n) {
  StepLayout L;
  const int KS = ks_of(d);
  L.frags_off = 0;
  L.cmax_off = (size_t)l * 8 * (2 * KS + 1) * 1024;   // [l][kCm] u32
  L.count_off = L.cmax_off + (size_t)l * 4 * kCm;      // [l] i32: left undecided by level 1
  L.cflag_off = L.count_off + (size_t)l * 4;           // [l] i32
  L.count2_off = L.cflag_off + (size_t)l * 4;          // [l] i32: left undecided by level 2
  L.list_off = (L.count2_off + (size_t)l * 4 + 255) / 256 * 256;   // [l][m] i32
  L.list2_off = (L.list_off + (size_t)l * m * 4 + 255) / 256 * 256;  // [l][m] i32
  L.upd_off = (L.list2_off + (size_t)l * m * 4 + 255) / 256 * 256;
  L.total = L.upd_off + tpq_compute_centroids_workspace_bytes(l, d, n);
  return L;
}

// levels 1 and 2 of all l sub-problems; level 2's list is what the exact kernel re-evaluates
static int run_levels(StepArgs sa, int l, int d, int* list2, int* count2, hipStream_t st) {
  const int KS = ks_of(d);
  sa.eps = level_eps(KS, d, 1);
  sa.level = 1;
  int rc = launch_coarse(KS, sa, l, st);
  if (rc) return rc;
  sa.eps = level_eps(KS, d, 2);
  sa.level = 2;
  sa.list_in = sa.list;
  sa.count_in = sa.count;
  sa.list = list2;
  sa.count = count2;
  return launch_refine(KS, sa, l, st);
}

}  // namespace lloyd
}  // namespace tpq

using namespace tpq;

extern "C" int tpq_lloyd_supported(int l, int d, int64_t m, int n) {
  if (!(l >= 1 && l <= 65535 && d >= 1 && d <= 64 && n >= 1 && n <= 256 && m >= 1 && m < (1LL << 31))) return 0;
  const lloyd::PrepLayout L = lloyd::prep_layout(l, d, m);
  return (L.T * ((L.KS + 1) / 2) * 2048 <= 0x7fffffffLL && (int64_t)d * m * 4 <= 0x7fffffffLL) ? 1 : 0;
}

extern "C" size_t tpq_lloyd_prepared_bytes(int l, int d, int64_t m) {
  if (l < 1 || d < 1 || d > 64 || m < 1) return 0;
  return lloyd::prep_layout(l, d, m).total;
}

extern "C" int tpq_lloyd_prepare(const float* data, const float* centroids0, void* prepared, size_t prepared_bytes,
                                 int l, int d, int64_t m, int n, tpq_stream_t stream) {
  TPQ_REQUIRE(data && centroids0 && prepared, "lloyd_prepare: null pointer");
  if (!tpq_lloyd_supported(l, d, m, n)) {
    set_error("lloyd_prepare: shape l=%d d=%d m=%lld n=%d not supported (d <= 64, n <= 256, slices < 2 GiB)", l, d,
              (long long)m, n);
    return TPQ_ERR_UNSUPPORTED;
  }
  const lloyd::PrepLayout L = lloyd::prep_layout(l, d, m);
  TPQ_REQUIRE(prepared_bytes >= L.total, "lloyd_prepare: prepared block of %zu bytes needed", L.total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* p = reinterpret_cast<char*>(prepared);
  int rc = check_hip(hipMemsetAsync(p + L.mu_off, 0, L.total - L.mu_off, st), "lloyd_prepare memset");
  if (rc) return rc;
  // the scale is a power of two: read a sixteenth of a large problem for it (every sixteenth 4-KiB run of each
  // row) and leave one bit of headroom; split_kernel flags the sub-problem whose data exceed it after all
  const int sample = m >= (1 << 18) ? 16 : 1;
  rc = lloyd::launch_scale({data, m, centroids0, n, l, d, 4096, sample, sample > 1 ? 1 : 0, true,
                            reinterpret_cast<float*>(p + L.mu_off), reinterpret_cast<unsigned*>(p + L.maxbits_off),
                            reinterpret_cast<int*>(p + L.flag_off), reinterpret_cast<float*>(p + L.scale_off)}, st);
  if (rc) return rc;
  return lloyd::launch_split(data, p, L, l, d, m, st);
}

extern "C" size_t tpq_lloyd_step_workspace_bytes(int l, int d, int64_t m, int n) {
  if (!tpq_lloyd_supported(l, d, m, n)) return 0;
  return lloyd::step_layout(l, d, m, n).total;
}

// diagnostics: byte offsets of the int32 [l] counts of points left undecided by level 1 / level 2
extern "C" size_t tpq_lloyd_step_count_offset(int l, int d, int64_t m, int n, int level) {
  if (!tpq_lloyd_supported(l, d, m, n)) return 0;
  const lloyd::StepLayout L = lloyd::step_layout(l, d, m, n);
  return level == 1 ? L.count_off : L.count2_off;
}

extern "C" int tpq_lloyd_step(const float* data, const void* prepared, const float* centroids, float* new_centroids,
                              float* vals, int64_t* inds, int l, int d, int64_t m, int n, void* workspace,
                              size_t workspace_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(data && prepared && centroids && inds, "lloyd_step: null pointer");
  if (!tpq_lloyd_supported(l, d, m, n)) {
    set_error("lloyd_step: shape l=%d d=%d m=%lld n=%d not supported", l, d, (long long)m, n);
    return TPQ_ERR_UNSUPPORTED;
  }
  const lloyd::PrepLayout P = lloyd::prep_layout(l, d, m);
  const lloyd::StepLayout L = lloyd::step_layout(l, d, m, n);
  TPQ_REQUIRE(workspace && workspace_bytes >= L.total, "lloyd_step: workspace of %zu bytes needed", L.total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const char* p = reinterpret_cast<const char*>(prepared);
  char* ws = reinterpret_cast<char*>(workspace);
  const float* mu = reinterpret_cast<const float*>(p + P.mu_off);
  const float* scale = reinterpret_cast<const float*>(p + P.scale_off);
  u32x4* frags = reinterpret_cast<u32x4*>(ws + L.frags_off);
  unsigned* cmax = reinterpret_cast<unsigned*>(ws + L.cmax_off);
  int* count = reinterpret_cast<int*>(ws + L.count_off);
  int* cflag = reinterpret_cast<int*>(ws + L.cflag_off);
  int* count2 = reinterpret_cast<int*>(ws + L.count2_off);
  int* list = reinterpret_cast<int*>(ws + L.list_off);
  int* list2 = reinterpret_cast<int*>(ws + L.list2_off);
  int rc = check_hip(hipMemsetAsync(ws + L.cmax_off, 0, L.list_off - L.cmax_off, st), "lloyd_step memset");
  if (rc) return rc;
  rc = lloyd::launch_cprep(centroids, mu, scale, frags, cmax, cflag, l, d, n, 1, P.KS, st);
  if (rc) return rc;
  lloyd::StepArgs sa{reinterpret_cast<const u32x4*>(p + P.hi_off),
                     reinterpret_cast<const u32x4*>(p + P.mid_off),
                     reinterpret_cast<const float2*>(p + P.norms_off),
                     frags, cmax, scale, reinterpret_cast<const int*>(p + P.flag_off), cflag, inds, vals,
                     nullptr, nullptr, list, count, (int)m, P.T,
                     0.f, (float)(d + 4) / 16777216.0f, sqrtf((float)d) / 8192.0f, 1, nullptr, 0,
                     nullptr, nullptr, 0};
  rc = lloyd::run_levels(sa, l, d, list2, count2, st);
  if (rc) return rc;
  rc = launch_max_sim_list(data, centroids, vals, inds, l, d, (int)m, n, 1, list2, count2, nullptr, nullptr, 0, st);
  if (rc) return rc;
  if (new_centroids) {
    if (TPQ_AB_ENV("TPQ_LL_OLD_UPDATE"))  // (A/B: the fp32-data update of max_sim.hip)
      return tpq_compute_centroids(data, inds, new_centroids, l, d, m, n, ws + L.upd_off,
                                   tpq_compute_centroids_workspace_bytes(l, d, n), stream);
    float* sums = reinterpret_cast<float*>(ws + L.upd_off);
    float* counts = sums + (size_t)l * d * n;
    rc = check_hip(hipMemsetAsync(sums, 0, tpq_compute_centroids_workspace_bytes(l, d, n), st), "lloyd_step memset");
    if (rc) return rc;
    lloyd::UpdArgs ua{reinterpret_cast<const u32x4*>(p + P.hi_off),
                      reinterpret_cast<const u32x4*>(p + P.mid_off), inds,
                      reinterpret_cast<const int*>(p + P.flag_off), sums, counts, d, n, (int)m, P.T};
    return lloyd::dispatch_ks<4>(P.KS, [&](auto ks) -> int {
      return lloyd::run_update<decltype(ks)::value>(ua, data, mu, scale, new_centroids, l, st);
    });
  }
  return TPQ_OK;
}
