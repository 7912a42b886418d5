// K-means update (centroids = the means of their points) for gfx950.
//
// tpq_compute_centroids replaces compute_centroids (torchpq/kernels/cuda/compute_centroids.cu:10-86):
// the reference launches l*d blocks that each re-read all labels; here data and labels are read
// exactly once (LDS atomics per block, one global atomic flush, tiny finalize kernel).
#include "mfma_util.h"

namespace tpq {

// ---- update --------------------------------------------------------------------------------
constexpr int kCcDT = 16;        // dimensions per block

// grid (ceil(n/points), ceil(d/kCcDT), l); LDS: [kCcDT][k] sums + [k] counts
__global__ __launch_bounds__(256) void centroid_accum_kernel(const float* __restrict__ data,
                                                             const int64_t* __restrict__ labels,
                                                             float* __restrict__ sums,
                                                             float* __restrict__ counts, int d,
                                                             int64_t n, int k, int64_t points) {
  extern __shared__ __attribute__((aligned(16))) float sh[];
  float* ssum = sh;               // [kCcDT][k]
  float* scnt = sh + kCcDT * k;   // [k]
  const int b = blockIdx.z;
  const int e0 = blockIdx.y * kCcDT;
  const int ne = (d - e0) < kCcDT ? (d - e0) : kCcDT;
  for (int t = threadIdx.x; t < (kCcDT + 1) * k; t += 256) sh[t] = 0.f;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * points;
  const int64_t i1 = (i0 + points) < n ? (i0 + points) : n;
  const bool count_here = (blockIdx.y == 0);
  const float* __restrict__ drow = data + ((int64_t)b * d + e0) * n;
  const int64_t* __restrict__ lrow = labels + (int64_t)b * n;
  // 16-byte loads need 16-byte addresses: with n % 4 == 0 every row of data and labels starts a
  // multiple of 16 bytes after its base, so the two bases decide (a contiguous view with a storage
  // offset is not aligned); block-uniform, misaligned input takes the scalar loop
  const bool aligned16 =
      ((reinterpret_cast<uintptr_t>(data) | reinterpret_cast<uintptr_t>(labels)) & 15) == 0;
  if (ne == kCcDT && (n & 3) == 0 && aligned16) {
    // full 16-dimension tile, 4 points per thread: 16 independent 16-byte loads in flight per
    // thread before the first LDS atomic (the scalar loop below is latency-bound: one 4-byte
    // load per ds_add)
    for (int64_t i = i0 + (int64_t)threadIdx.x * 4; i < i1; i += 256 * 4) {
      float4 x[kCcDT];
#pragma unroll
      for (int e = 0; e < kCcDT; ++e) x[e] = *reinterpret_cast<const float4*>(drow + (int64_t)e * n + i);
      const longlong2 la = *reinterpret_cast<const longlong2*>(lrow + i);
      const longlong2 lb = *reinterpret_cast<const longlong2*>(lrow + i + 2);
      const long long lab[4] = {la.x, la.y, lb.x, lb.y};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i + u >= i1 || lab[u] < 0 || lab[u] >= k) continue;
        if (count_here) atomicAdd(&scnt[lab[u]], 1.0f);
#pragma unroll
        for (int e = 0; e < kCcDT; ++e) {
          const float v = u == 0 ? x[e].x : u == 1 ? x[e].y : u == 2 ? x[e].z : x[e].w;
          atomicAdd(&ssum[e * k + lab[u]], v);
        }
      }
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const int64_t lab = lrow[i];
      if (lab < 0 || lab >= k) continue;
      if (count_here) atomicAdd(&scnt[lab], 1.0f);
      for (int e = 0; e < ne; ++e) atomicAdd(&ssum[e * k + lab], drow[(int64_t)e * n + i]);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < ne * k; t += 256) {
    const float s = ssum[t];
    if (s != 0.f) unsafeAtomicAdd(&sums[((int64_t)b * d + e0) * k + t], s);
  }
  if (count_here)
    for (int t = threadIdx.x; t < k; t += 256) {
      const float c = scnt[t];
      if (c != 0.f) unsafeAtomicAdd(&counts[(int64_t)b * k + t], c);
    }
}

// ---- update, many clusters (coarse quantiser: k in the thousands) ------------------------------
// With thousands of bins per dimension an LDS privatisation no longer fits and contention on any
// one bin is low, so each (point, dimension) goes straight to an L2 float atomic.
__global__ __launch_bounds__(256) void centroid_accum_global_kernel(
    const float* __restrict__ data, const int64_t* __restrict__ labels, float* __restrict__ sums,
    float* __restrict__ counts, int d, int64_t n, int k) {
  const int b = blockIdx.z;
  const int e0 = blockIdx.y * kCcDT;
  const int ne = (d - e0) < kCcDT ? (d - e0) : kCcDT;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t lab = labels[(int64_t)b * n + i];
  if (lab < 0 || lab >= k) return;
  if (blockIdx.y == 0) unsafeAtomicAdd(&counts[(int64_t)b * k + lab], 1.0f);
  for (int e = 0; e < ne; ++e)
    unsafeAtomicAdd(&sums[((int64_t)b * d + e0 + e) * k + lab], data[((int64_t)b * d + e0 + e) * n + i]);
}

// ---- update on the bf16 matrix cores (k <= 256) ---------------------------------------------
// sums[cluster][dim] = sum_i onehot(label_i)[cluster] * x_i[dim] is a GEMM whose left operand is a
// 0/1 matrix.  fp32 MFMA would waste 255/256 of its multiplies at 1/16 of the bf16 rate; instead x
// is split EXACTLY into three bf16 pieces (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi -
// mid): 3 x 8 significant bits), the one-hot tile is built in registers from the labels, and
// v_mfma_f32_32x32x16_bf16 accumulates 1.0 * piece products in fp32 -- exact products, fp32 sums,
// 16 points per instruction.  Operand layout (tools/ubench/mfma_bf16_layout.hip): A[row][k] in
// lane row + 32 (k / 8), element k % 8; B[k][col] likewise; D as the f32 forms.
// LDS float atomics are the trap on the scalar route: ds_add_f32 retires ~0.38 lanes per clock
// per CU on gfx950 whatever the access pattern (tools/ubench/lds_atomic.hip; integer atomics are
// 16x faster); an atomic-free LDS read-add-write version reached 9.2 ms at C5, this one 4.8 ms.
// (A NaN / Inf coordinate reaches every cluster of its 16-point group through 0 * x; the scalar
// kernels confine it to its own cluster.)
constexpr int kUmP = 64;              // points per staged tile (4 MFMA k-steps of 16)
constexpr int kUmStride = kUmP + 4;   // floats per dimension row in LDS (b128 reads stay conflict-free)

// One WAVE per block owns all 256 clusters x 32*CT dimensions of its tiles: 8 x CT accumulator
// tiles.  CT = 2 (64 dimensions, 256 accumulator registers) leaves one wave per SIMD: its VALU
// work and its tile staging then run in series with its own MFMAs (5.9 ms at C5 against 2.5 ms of
// matrix-pipe time).  CT = 1 (32 dimensions, 128 registers) puts two independent waves on every
// SIMD -- no barrier between them, each splits only its own dimensions -- so one wave's VALU / LDS
// / load phases sit under the other's MFMAs.  (A first version spread the CLUSTERS over the 4
// waves of a block: every wave then split the same tile into bf16 pieces again and the block met
// at a barrier per 64 points -- 7.4 ms at C5; the LDS read-add-write kernel above: 9.2 ms.)
// The B fragment wants 8 consecutive points of ONE dimension per lane; straight from global memory
// that is one 32-byte request per lane (address-unit bound, 32 ms), so [dims][64 points] tiles
// go through LDS, loaded two tiles ahead (below).
// r02 at C5: 5.9 -> 4.8 ms (3.5 TB/s; the bare read pattern streams at 6.2 TB/s --
// tpq_ubench_rows_read -- and the MFMAs need 2.5 ms; what is left is a wave waiting, 59 % of its
// cycles by SQ_WAIT_INST_ANY, for its own LDS round trips at the head of every k-step: two waves
// per SIMD do not cover them, and a second one-hot table to pipeline k-steps does not fit 20 KiB
// of LDS per wave).
#ifndef TPQ_UM_CT
#define TPQ_UM_CT 1
#endif
#ifndef TPQ_UM_EXP
#define TPQ_UM_EXP 0  // experiments (tools/build_variant.sh): 1 = no MFMAs, 2 = no tile reloads
#endif

// (Lesson kept from the version that built the one-hot operand in registers with three
// packed-u16 instructions per label pair: written as inline asm they produced scheduling-dependent
// WRONG sums -- the hazard recogniser cannot see a VALU write inside an asm block that an MFMA reads
// as its A operand a few cycles later; the same instructions selected by the compiler from plain
// vector code (__builtin_elementwise_sub_sat, u16x2 multiply) were correct.)

template <int CT, bool VEC>
__global__ __launch_bounds__(64, (CT == 1 ? 2 : 1)) void centroid_accum_mfma_kernel(
    const float* __restrict__ data, const int64_t* __restrict__ labels, float* __restrict__ sums,
    float* __restrict__ counts, int d, int64_t n, int k) {
  constexpr int ND = 32 * CT;  // dimensions per wave
  // one wave per block: its DS operations execute in order, so ONE tile buffer is enough (the
  // stores of tile t+1 queue up behind the reads of tile t) and no barrier is ever needed
  __shared__ __attribute__((aligned(16))) float xt[ND * kUmStride];
  // the one-hot operand of the current k-step: [2 k-groups][256 clusters][8 points] bf16, all zero
  // except one 1.0 per point (see below)
  __shared__ __attribute__((aligned(16))) uint16_t otab[256 * 16];
  __shared__ int cnt[256];
  const int b = blockIdx.z;
  const int lane = threadIdx.x;
  const int l31 = lane & 31, half = lane >> 5;
  const int e0 = blockIdx.y * ND;
  const int nd = (d - e0) < ND ? (d - e0) : ND;  // dimensions of this block that exist
  // Tiles are dealt round-robin to the gridDim.x blocks of a (sub-problem, dimension tile): the
  // blocks run side by side, so at any moment they read ADJACENT 256-byte pieces of the same
  // 32 rows -- whole DRAM pages get used while they are open.  (With one contiguous point range
  // per block every 256-byte access opened a page of its own: the kernel read at 3.4 TB/s.)
  const int64_t step = (int64_t)gridDim.x * kUmP;
  const int64_t i0 = (int64_t)blockIdx.x * kUmP;  // first tile of this block (exists: host)
  const int64_t i1 = n;
  const int64_t* __restrict__ lrow = labels + (int64_t)b * n;
  const float* __restrict__ dbase = data + ((int64_t)b * d + e0) * n;
  f32x16 acc[8][CT];  // [cluster row tile][dimension column tile]
#pragma unroll
  for (int rt = 0; rt < 8; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][ct][r] = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) cnt[lane + 64 * u] = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) reinterpret_cast<u32x4*>(otab)[lane + 64 * u] = u32x4{0u, 0u, 0u, 0u};
  const bool count_here = blockIdx.y == 0;

  // Tiles travel global -> registers -> LDS, TWO tiles ahead of the MFMAs: the loads of tile t+2
  // are issued in four quarters, one per MFMA k-step of tile t (so the wave's load issue hides
  // behind its MFMAs), and reach LDS at the end of tile t+1 -- more than two tile times in flight
  // (with one tile ahead the wave waited out part of every memory latency: 5.65 ms at C5 against
  // 3.7 ms with the reloads knocked out).  VEC (n % 4 == 0): a lane loads 4 consecutive points of
  // one dimension row (16 B), a wave-instruction 4 rows x 256 B; otherwise one point per lane.
  // Loads are unconditional on clamped addresses: out-of-range points carry label 0xFFFF (their
  // one-hot column is zero) and out-of-range dimension rows land in accumulator columns that are
  // never written out; no exec-mask branches, no selects behind the loads.
  constexpr int NV = VEC ? ND / 4 : ND;  // load instructions (registers: NV float4 / NV floats)
  typedef typename std::conditional<VEC, f32x4, float>::type xreg_t;
  struct Staged {
    xreg_t x[NV];
    int64_t label;
    bool label_valid;
  };
  const int vrow = VEC ? (lane >> 4) : 0, vpt = VEC ? (lane & 15) * 4 : lane;
  auto load_quarter = [&](Staged& st, int64_t p0, int qt) {
    const int64_t pt = p0 + vpt;
    const bool pv = pt < i1;
    const float* __restrict__ p = dbase + (pv ? pt : i0);
#pragma unroll
    for (int j = (NV / 4) * qt; j < (NV / 4) * (qt + 1); ++j) {
      const int row = VEC ? 4 * j + vrow : j;
      st.x[j] = *reinterpret_cast<const xreg_t*>(p + (int64_t)(row < nd ? row : 0) * n);
    }
    if (qt == 0) {  // the raw label: any arithmetic on it here would wait for the load on the spot
      const int64_t lp = p0 + lane;
      st.label_valid = lp < i1;
      st.label = lrow[st.label_valid ? lp : i0];
    }
  };
  int lab_cur = -1;  // label of point (tile in LDS) + lane, -1 = none
  auto store_tile = [&](const Staged& st) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int row = VEC ? 4 * j + vrow : j;
      *reinterpret_cast<xreg_t*>(&xt[row * kUmStride + vpt]) = st.x[j];
    }
    lab_cur = (st.label_valid && st.label >= 0 && st.label < k) ? (int)st.label : -1;
  };
  // one tile: MFMAs from the LDS tile; `fill` receives tile it+2; `drain` (tile it+1) replaces the
  // LDS tile afterwards.
  // The one-hot A operand costs NO VALU work: the [256 clusters][16 points] bf16 matrix of a
  // k-step lives in LDS, all zero; the 16 lanes that own the k-step's points each store one 1.0
  // at [label][point] (ds_write_b16), every lane then reads its 8 row tiles as ds_read_b128 --
  // 16 contiguous bytes = the 8 consecutive points of its k-group, exactly the fragment -- and the
  // writers store the zero back.  (Built in registers from packed label pairs the operand took
  // 96 VALU instructions per k-step, 3 per pair and row tile, next to 44 for the bf16 splitting:
  // the two waves of a SIMD then issue as many VALU cycles as MFMA cycles and the update ran at
  // 5.2 ms against 2.5 ms of matrix-pipe time.)
  auto run_tile = [&](int64_t p0, Staged& fill, const Staged& drain) {
    // (no "is there a tile t+1 / t+2" branches: beyond the range the loads read clamped addresses
    // and the store fills a tile nobody reads.  With conditional loads the compiler's waitcnt
    // bookkeeping merges the two paths and falls back to vmcnt(0) before the LDS stores, i.e. it
    // waits for the loads of tile t+2 that were only just issued)
    if (count_here && lab_cur >= 0) atomicAdd(&cnt[lab_cur], 1);  // integer LDS atomic: fast
    // layout [k-group (2)][cluster (256)][8 points]: the 16 lanes of a ds_read_b128 group then read
    // 256 contiguous bytes (with [cluster][16 points] rows two lanes of a group met on a bank:
    // SQ_LDS_BANK_CONFLICT was 36 % of the LDS cycles)
    uint16_t* oslot = &otab[((lane >> 3) & 1) * 2048 + (lab_cur >= 0 ? lab_cur : 0) * 8 + (lane & 7)];
#pragma unroll
    for (int ks = 0; ks < kUmP / 16; ++ks) {
      if (!(TPQ_UM_EXP & 2)) load_quarter(fill, p0 + 2 * step, ks);
      const bool writer = (lane >> 4) == ks && lab_cur >= 0;
      if (writer) *oslot = (uint16_t)0x3F80;  // bf16 1.0
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int pts = 16 * ks + 8 * half;  // this lane's 8 points (its k-group)
      const bf16x8* orow = reinterpret_cast<const bf16x8*>(&otab[half * 2048 + l31 * 8]);
      bf16x8 aring[3];  // A operands are fetched two row tiles ahead of their MFMAs
      aring[0] = orow[0];
      aring[1] = orow[32];
      bf16x8 piece[3][CT];  // [hi, mid, lo][column tile]
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const float* xrow = &xt[(32 * ct + l31) * kUmStride + pts];
        const float4 xa = *reinterpret_cast<const float4*>(xrow);
        const float4 xb = *reinterpret_cast<const float4*>(xrow + 4);
        const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          __bf16 h, m, lo;
          split3_bf16(xv[i], h, m, lo);
          piece[0][ct][i] = h;
          piece[1][ct][i] = m;
          piece[2][ct][i] = lo;
        }
      }
      // the accumulator tiles take turns: an MFMA never waits for the one issued before it
#pragma unroll
      for (int rt = 0; rt < 8; ++rt) {
        if (rt + 2 < 8) aring[(rt + 2) % 3] = orow[32 * (rt + 2)];  // 32 rows x 16 B
        const bf16x8 aop = aring[rt % 3];
        // (all column tiles always: a wave-uniform branch around the second one when d <= 32
        // broke the MFMA interleaving and cost more than the multiplies it saved)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            if (TPQ_UM_EXP & 1) {
              acc[rt][ct][pc] += (float)aop[pc] + (float)piece[pc][ct][rt];
              continue;
            }
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aop, piece[pc][ct], acc[rt][ct], 0, 0, 0);
          }
      }
      __builtin_amdgcn_wave_barrier();
      if (writer) *oslot = (uint16_t)0;  // after the last read of this k-step has been issued
    }
    store_tile(drain);
    // the next tile's reads see these stores without a barrier (in-order DS) -- and a
    // __syncthreads() would bring an s_waitcnt vmcnt(0) with it, i.e. wait for the loads of tile
    // t+2 that were only just issued
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  Staged sa, sb;
  sa.label = sb.label = -1;
  sa.label_valid = sb.label_valid = false;
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) load_quarter(sa, i0, qt);
  store_tile(sa);
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) load_quarter(sa, i0 + step, qt);  // clamped when out of range
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (int64_t p0 = i0; p0 < i1; p0 += 2 * step) {
    run_tile(p0, sb, sa);                             // tile 2j: fill sb (2j+2), drain sa (2j+1)
    if (p0 + step < i1) run_tile(p0 + step, sa, sb);  // tile 2j+1: fill sa (2j+3), drain sb (2j+2)
  }
#pragma unroll
  for (int rt = 0; rt < 8; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int dim = e0 + 32 * ct + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cluster = 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float v = acc[rt][ct][r];
        if (dim < d && cluster < k && v != 0.f)
          unsafeAtomicAdd(&sums[((int64_t)b * d + dim) * k + cluster], v);
      }
    }
  if (count_here) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = lane + 64 * u;
      if (c < k && cnt[c]) unsafeAtomicAdd(&counts[(int64_t)b * k + c], (float)cnt[c]);
    }
  }
}

__global__ __launch_bounds__(256) void centroid_finalize_kernel(const float* __restrict__ sums,
                                                               const float* __restrict__ counts,
                                                               float* __restrict__ out, int d, int k,
                                                               int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int c = (int)(t % k);
  const int64_t b = t / ((int64_t)d * k);
  const float cnt = counts[b * k + c];
  out[t] = cnt == 0.f ? 0.f : sums[t] / cnt;  // compute_centroids.cu:82
}

}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_compute_centroids_workspace_bytes(int l, int d, int k) {
  return ((size_t)l * d * k + (size_t)l * k) * sizeof(float);
}

extern "C" int tpq_compute_centroids(const float* data, const int64_t* labels, float* centroids,
                                     int l, int d, int64_t n, int k, void* workspace,
                                     size_t workspace_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(data && labels && centroids, "compute_centroids: null pointer");
  TPQ_REQUIRE(l >= 1 && d >= 1 && n >= 0 && k >= 1, "compute_centroids: bad shape");
  TPQ_REQUIRE(l <= 65535, "compute_centroids: batch l=%d exceeds grid.z", l);
  const size_t need = tpq_compute_centroids_workspace_bytes(l, d, k);
  if (!workspace || workspace_bytes < need) {
    set_error("compute_centroids: workspace too small (%zu < %zu)", workspace_bytes, need);
    return TPQ_ERR_WORKSPACE;
  }
  const size_t lds = (size_t)(kCcDT + 1) * k * sizeof(float);
  const bool lds_fits = lds <= 160 * 1024;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc = check_hip(hipMemsetAsync(workspace, 0, need, st), "compute_centroids memset");
  if (rc) return rc;
  float* sums = reinterpret_cast<float*>(workspace);
  float* counts = sums + (size_t)l * d * k;
  if (n > 0) {
    if (k <= 256 && d >= 32) {  // wide PQ-codebook shape: bf16 matrix cores
      constexpr int CT = TPQ_UM_CT;
      const int dtiles = (d + 32 * CT - 1) / (32 * CT);
      // blocks per (sub-problem, dimension tile): a few rounds of the 2048 / CT resident waves,
      // but at least 64 tiles (4096 points) per block -- every block ends with 256 x 32 CT global
      // atomics -- and never more blocks than tiles
      int64_t chunks = (4096 / CT) / ((int64_t)l * dtiles);
      const int64_t n_tiles = (n + kUmP - 1) / kUmP;
      if (chunks > n_tiles / 64) chunks = n_tiles / 64;
      if (chunks < 1) chunks = 1;
      const dim3 grid((unsigned)chunks, dtiles, l);
      if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(data) & 15) == 0)
        hipLaunchKernelGGL((centroid_accum_mfma_kernel<CT, true>), grid, dim3(64), 0, st, data, labels,
                           sums, counts, d, n, k);
      else
        hipLaunchKernelGGL((centroid_accum_mfma_kernel<CT, false>), grid, dim3(64), 0, st, data, labels,
                           sums, counts, d, n, k);
      TPQ_LAUNCH_CHECK("centroid_accum_mfma_kernel");
      const int64_t total = (int64_t)l * d * k;
      hipLaunchKernelGGL(centroid_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256),
                         0, st, sums, counts, centroids, d, k, total);
      TPQ_LAUNCH_CHECK("centroid_finalize_kernel");
      return TPQ_OK;
    }
    if (!lds_fits) {
      hipLaunchKernelGGL(centroid_accum_global_kernel,
                         dim3((unsigned)((n + 255) / 256), (d + kCcDT - 1) / kCcDT, l), dim3(256), 0,
                         st, data, labels, sums, counts, d, n, k);
      TPQ_LAUNCH_CHECK("centroid_accum_global_kernel");
      const int64_t total = (int64_t)l * d * k;
      hipLaunchKernelGGL(centroid_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256),
                         0, st, sums, counts, centroids, d, k, total);
      TPQ_LAUNCH_CHECK("centroid_finalize_kernel");
      return TPQ_OK;
    }
    // Each block flushes kCcDT*k global atomics, so blocks must own many points; aim for ~8 k
    // blocks in total (>> 256 CUs) but never fewer than 4096 points per block.
    const int dtiles = (d + kCcDT - 1) / kCcDT;
    int64_t chunks = 8192 / ((int64_t)l * dtiles);
    if (chunks < 1) chunks = 1;
    int64_t points = (n + chunks - 1) / chunks;
    if (points < 4096) points = 4096;
    points = (points + 255) / 256 * 256;
    rc = launch_with_lds(centroid_accum_kernel, "centroid_accum_kernel", dim3((unsigned)((n + points - 1) / points), dtiles, l),
                         dim3(256), lds, st, data, labels, sums, counts, d, n, k, points);
    if (rc) return rc;
  }
  const int64_t total = (int64_t)l * d * k;
  hipLaunchKernelGGL(centroid_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     st, sums, counts, centroids, d, k, total);
  TPQ_LAUNCH_CHECK("centroid_finalize_kernel");
  return TPQ_OK;
}
