// IVF list scan: the packed-layout kernel -- wave, slot and tile policy, scan_packed_kernel and its stages.
#pragma once
#include "scan_list.h"  // clamped_n_probe
#include "scan_lut.h"
#include "scan_exact.h"

namespace tpq {

// ---- packed-layout kernel ------------------------------------------------------------------
// LUT in LDS in block order (scan_layout.h): entry (j, c) at dword lut_dword(M, j, c); the slot at
// address s stores at byte position p the code of sub-quantizer subq_at(M, p, s), so lane (slot s)
// step p reads a bank that differs from every other lane of its half-wave.
//
// The permuted order changes the fp32 summation order, so the streamed value f ("fast") is
// used for SELECTION only: with |f - e| <= delta (e = the reference's ascending-order value),
// every element of the exact top-k has f >= F_k - 2*delta (F_k = k-th best fast value).  Each
// wave keeps its best 64R > k candidates by f and admits everything down to threshold - 2*delta.
// At the end of the query a wave re-evaluates the entries that can still matter
// (f >= shared threshold - 2*delta: ~k/8 of them) exactly -- ascending j, from the packed bytes
// un-permuted through a private LDS row, LUT still resident -- re-ranks them by (e desc, address
// asc) and dumps the list; scan_merge_refine_kernel merges the per-wave lists of a query and
// writes the best k: bit-identical to the reference-layout kernel.  If a merged list ends up so
// full of near-ties (more than 64R candidates within 2*delta of the k-th) that a member of the
// exact top-k may have been evicted, the query is flagged and redone by scan_ref_kernel.

// waves per workgroup: 8 while two workgroups share a CU (LUT <= 64 KiB); 16 when the LUT is so
// large that only one workgroup fits (m > 64, e.g. GIST m=120: 120 KiB) -- same 16 waves per CU.
// Short codes (m <= 32, LUT <= 32 KiB): 4 waves, FOUR workgroups per CU -- a query is then a
// quarter of the CU's waves, so its fixed costs (launch, staging, end-of-query barrier, counting
// rounds, refinement: ~40 % of a query's life at m=16) overlap with three other queries' streaming
// instead of one (r02, 10 000 queries x 32 probes: m=8 0.98 -> 0.79 ms, 16 1.30 -> 1.12,
// 24 1.63 -> 1.51, 32 1.98 -> 1.73)
constexpr int packed_waves(int M) { return M <= 32 ? 4 : (M <= 64 ? 8 : 16); }
// Short codes are instruction-bound, not bandwidth-bound (~61 + 3.4 m cycles per 64-slot
// tile per CU, the 61 being table walk, address arithmetic, exec-mask handling, threshold poll and
// ballot): a lane therefore takes S slots (64 apart) per iteration and pays that part once.
// (measured, 10 000 queries x 32 probes: m=4 +18 %, 8 +16 %, 12 +12 %, 16 +9 %, 20 +10 %, 24 +10 %;
// neutral from m=28 on, where one slot per lane is kept)
#ifdef TPQ_SLOTS_LOG2  // experiments (tools/build_variant.sh): slots per lane = 1 << TPQ_SLOTS_LOG2
constexpr int packed_slots(int M) { return 1 << TPQ_SLOTS_LOG2; }
constexpr int packed_tile_shift(int M) { return 6 + TPQ_SLOTS_LOG2; }
#else
// (r02 sweep, 10 000 queries x 32 probes, ms for S = 1 / 2 / 4: m=28 1.97 / 2.06 / 2.04,
// m=32 2.25 / 2.05 / 1.98, m=40 2.37 / 2.44 / 2.47, m=48 2.84 / 2.65 / 4.82, m=56 3.35 / 3.21 / -,
// m=64 3.09 / 5.84 / -: the 16-byte-chunk layouts (m % 16 == 0) gain until the second tile's
// registers spill; with 4-wave workgroups (m <= 32): m=16 1.17 / 1.13 / 1.12, m=24 1.62 / 1.52 /
// 1.58, m=28 1.93 / 1.81 / 1.78, m=32 2.02 / 1.82 / 1.76)
// (round 6, after the look-ups of the small blocks went from 3.25 to 2 VALU: the per-tile part weighs more, and four
// slots per lane now win from m = 12 on -- same box, S = 2 -> 4, C2 shape k = 100 / k = 1 / 244-slot cells: m = 12 +5 / +6 /
// +2 %, 16 +7 / +9 / +7 %, 20 +8 / +6 / +4 %, 24 0 / +3 / +3 %; m = 40 -13 %, 48 -10 %, 56 -26 %: those keep theirs)
// (m = 40: two slots per lane once the per-slot part had shrunk -- +4 % at the C2 shape, +8 % on 244-slot cells, same box)
constexpr int packed_slots(int M) {
  return M <= 32 ? 4 : ((M == 40 || M == 48 || M == 56) ? 2 : 1);
}
constexpr int packed_tile_shift(int M) { return packed_slots(M) == 4 ? 8 : (packed_slots(M) == 2 ? 7 : 6); }
#endif

// per-wave scratch of the end-of-query exact re-evaluation: un-permute rows of M/4+1 dwords,
// 16 per pass (8 when the LUT leaves little LDS: m > 64)
constexpr int refine_rows(int M) { return M <= 64 ? 16 : 8; }
constexpr int packed_aux_bytes(int /*R*/, int M) {
  return packed_waves(M) * refine_rows(M) * (M / 4 + 1) * 4;
}

// 2 workgroups per CU (LDS: 2 x (64 KiB LUT + ~14 KiB)) need <= 128 VGPRs: 4 waves per SIMD.
// Long lists (R = 8, 16) are held to the same cap: a handful of spilled registers in the (cold)
// flush path cost far less than running one workgroup per CU (k = 300: 8.9 -> 6.4 ms).
//
// RES = residual PQ (replaces ivfpq_topk_residual_precomputed, ivfpq_topk.cu:1039-1208, at full
// scan speed): the reference rebuilds LUT_p = part1[q] + part2[cell_p] in shared memory for every
// probe (128 KiB read per 62 KiB of codes at C2).  Here only part1[q] is staged, once per query;
// the cell-dependent half of the fast value, sum_j part2[cell(s)][j][code_j(s)], is a per-SLOT
// constant precomputed at index-build time (ResidualArgs::slot_term, 4 B per slot) and
//   f(s) = sum_j part1[j][code_j] (permuted order) + (base_p + slot_term[s]).
// f is again a selection key only (|f - e| <= delta with the bound below); survivors are
// re-evaluated with the reference's arithmetic: v = base_p; v += fl(part1 + part2) ascending j.
//
// RM > 0 ("fused finish", small batches): the workgroup also FINISHES -- its waves' exact lists are
// tree-merged through LDS, a query split over several workgroups meets in the last one to arrive (a ticket
// per query), which writes the result; an overflowing candidate band is redone, exactly, by that same
// workgroup.  One launch instead of three (scan, scan_merge_refine_kernel, the flagged redo): at one query
// the two extra launches were 25 of 64 us.  RM = registers of the merged list (list_regs_packed(k)).
//
// RM < 0 ("pool mode", k > 504 -- k > 248 at m <= 32 --, plain PQ; scan.hip holds the rule): folding 64 candidates into a sorted list of k + 8 (or even 2k / NW)
// entries is what made large k slow -- at k = 1000 the tile loop ran 275 us per query against 106 at k = 100.
// Here the sorted per-wave list (R registers) only serves the ADMISSION THRESHOLD: it holds the wave's
// ceil(k / NW) best (bound (b) below needs no more), and every admitted candidate is also appended to an
// unsorted pool in the workspace.  Nothing is ever evicted from a pool, so at the end of the query the counting
// rounds run over the pools, the entries at or above the cut are compacted through the wave's queue, re-evaluated
// exactly and written back -- unsorted; scan_pool_merge_kernel ranks a query's ~k exact candidates in LDS.
// A pool that fills up flags the query for the exact kernel.
// RM <= kDumpF32 ("dump", large batches of plain PQ, k <= 248): the workgroup ENDS after the tile loop -- its waves store
// their lists of fast values and scan_finish_exact_kernel does the rest at full occupancy (the end of a query -- barrier,
// counting rounds, refinement, merge: 17 of the 43 us a 16-probe query of 244-slot cells lives -- held a 64-KiB-LDS
// workgroup slot idle).  RM = kDumpSel16: the table is the 16-bit one (above), four waves per workgroup.
constexpr int scan_waves(int M, int RM) { return RM == kDumpSel16 ? 4 : packed_waves(M); }
template <int R, int M, bool RES, int RM = 0>
__global__ __launch_bounds__(scan_waves(M, RM) * 64, 4) void scan_packed_kernel(ScanArgs a,
                                                                                      ResidualArgs ra,
                                                                                      float delta_rel) {
  using L = scan_layout::Layout<M>;
  constexpr bool DUMP = is_dump(RM), SEL16 = is_sel16(RM), POOL = is_pool(RM);
  static_assert(!(DUMP && RES), "dump mode serves plain PQ");
  constexpr int NW = scan_waves(M, RM);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int lut_bytes = SEL16 ? M * 512 : M * 1024;
  constexpr int aux_bytes = DUMP ? 0 : packed_aux_bytes(R, M);
  float* lut = reinterpret_cast<float*>(smem);
  uint32_t* scratch_all = reinterpret_cast<uint32_t*>(smem + lut_bytes);
  float* qv_all = reinterpret_cast<float*>(smem + lut_bytes + aux_bytes);
  int* qi_all = reinterpret_cast<int*>(smem + lut_bytes + aux_bytes + NW * 256);
  int* ptab = reinterpret_cast<int*>(smem + lut_bytes + aux_bytes + NW * 512);
  ProbeTable tab{ptab, ptab + a.max_nprobe, ptab + 2 * a.max_nprobe};
  unsigned* tau_key = reinterpret_cast<unsigned*>(ptab + 3 * a.max_nprobe + 1);
  int* tile_ctr = reinterpret_cast<int*>(tau_key + 1);  // m > 64: next tile to hand out
  float* red = reinterpret_cast<float*>(tile_ctr + 1);  // [2 NW] reduction scratch
  float* wave_q = red + 2 * NW;                // [NW] each wave's r-th best
  float* pbase = wave_q + NW;                  // RES: [max_nprobe] base_sims of the probe
  int* pcell = reinterpret_cast<int*>(pbase + (RES ? a.max_nprobe : 0));  // RES: [max_nprobe] cell
  float* xq = reinterpret_cast<float*>(pcell + (RES ? a.max_nprobe : 0));
  // (wave-uniform by construction: told to the compiler, so that the tile index, the probe cursor and their compares
  // live on the scalar unit instead of in VGPRs behind exec masks -- the scan is VALU-issue-bound)
  // (same box, caller-supplied table, C2 shape, TB/s without / with the hint: m = 16 4.60 / 4.71, 20 4.37 / 4.71,
  // 24 4.69 / 5.02, 32 5.88 / 5.90, 64 6.92 / 7.07)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = lane_id();
  {
    // scan_layout's look-up address folds the table's LDS address into lane constants that are XORed with position bits
    // (accumulate, accumulate16): the table must start at a multiple of 128 bytes.  It does -- the dynamic allocation starts
    // at 0 as long as this kernel declares no static __shared__ --; a build that breaks that traps instead of mis-scanning.
    typedef const __attribute__((address_space(3))) char* lds_char_ptr;
    if (((uint32_t)(uintptr_t)(lds_char_ptr)smem & 127u) != 0u) __builtin_trap();
  }
  int q, part, parts;  // query, this workgroup's part of it, the parts it is dealt in
  if (DUMP && (int)blockIdx.x < a.unsplit) {  // (tail split, ScanArgs::unsplit: the leading queries are not split)
    q = (int)blockIdx.x;
    part = 0;
    parts = 1;
  } else {
    const int first = DUMP ? a.unsplit : 0;
    const int b = (int)blockIdx.x - first;
    q = first + b / a.n_split;
    part = b - (q - first) * a.n_split;
    parts = a.n_split;
  }
  // (dispatch order, ScanArgs::order: the position dealt above is a RANK -- workgroups start in blockIdx order, the
  // longest queries first, the split tail is the shortest; one wave-uniform load, the pointer is null in index order)
  if constexpr (DUMP) {
    if (a.order) q = __builtin_amdgcn_readfirstlane(a.order[q]);
  }
  TPQ_PROF(a, blockIdx.x, 0);
  const int n_probe = clamped_n_probe(a, q);

  unsigned* jmax = reinterpret_cast<unsigned*>(qv_all);  // [M] (the queues are not live yet)
  if (threadIdx.x < M) jmax[threadIdx.x] = 0u;
  __syncthreads();
  // (wave 0 issues the loads of the probe table FIRST and builds the table after the LUT is staged: done up front,
  // its two dependent global round trips kept the other waves at the staging barrier for 1.7 us per query)
  ProbeRegs probes0{0, 0};
  if (wave == 0) {
    probes0 = fetch_probes(a, q, n_probe, 0);
    if (lane == 0) {
      *tau_key = f2key(-INFINITY);
      *tile_ctr = 0;
    }
    if (lane < NW) wave_q[lane] = -INFINITY;
  }
  TPQ_PROF(a, blockIdx.x, 1);
  const float* part1 = RES ? ra.part1 : nullptr;
  if (!a.lut && !part1) stage_query(a, q, xq, NW * 64);
  TPQ_PROF(a, blockIdx.x, 10);  // (dump modes: sub-phases of the prologue, slots 10 ... 14)
  [[maybe_unused]] float inv16 = 0.f;  // SEL16: table units per unit of value
  if constexpr (SEL16) {
    float4 ent[M * 64 / (NW * 64)];
    lut16_compute<M, NW * 64>(a, q, xq, jmax, ent);
    TPQ_PROF(a, blockIdx.x, 11);
    if (wave == 0) build_probe_table(a, q, n_probe, tab, packed_tile_shift(M), &probes0);
    __syncthreads();
    TPQ_PROF(a, blockIdx.x, 12);
    unsigned jb = 0u;
    float sum = 0.f;
#pragma unroll
    for (int j0 = 0; j0 < M; j0 += 64) {
      if (j0 + lane < M) {
        jb = jmax[j0 + lane] > jb ? jmax[j0 + lane] : jb;
        sum += __uint_as_float(jmax[j0 + lane]);
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)jb, d, 64);
      jb = o > jb ? o : jb;
      sum += __shfl_xor(sum, d, 64);
    }
    const float J = __uint_as_float(jb);
    // a table that cannot be scaled (NaN / Inf entries, overflow of 2 J or of the bound, all zeros): the exact kernel
    // takes the query (scan.hip launches it over the flagged ones)
    const bool scalable = jb < 0x7f800000u && J >= 1e-30f && J <= 1e37f && sum <= 1e37f;
    if (threadIdx.x == 0 && part == 0) a.flags[q] = scalable ? 0 : a.epoch;
    if (!scalable) return;  // (workgroup-uniform: every wave reduced the same words)
    inv16 = 65535.f / (2.f * J);
    lut16_store<M, NW * 64>(ent, jmax, inv16, reinterpret_cast<uint16_t*>(lut));
    TPQ_PROF(a, blockIdx.x, 13);
  } else {
    stage_lut_blocked<M>(a, q, lut, NW * 64, jmax, xq, part1);
    TPQ_PROF(a, blockIdx.x, 11);
    if (wave == 0) build_probe_table(a, q, n_probe, tab, packed_tile_shift(M), &probes0);
    TPQ_PROF(a, blockIdx.x, 13);
  }
  float probe_mx = 0.f;
  if constexpr (RES) {
    for (int pp = threadIdx.x; pp < n_probe; pp += NW * 64) {
      const float b = ra.base_sims[(int64_t)q * a.max_nprobe + pp];
      const int c = (int)ra.cells[(int64_t)q * a.max_nprobe + pp];
      pbase[pp] = b;
      pcell[pp] = c;
      probe_mx = fmaxf(probe_mx, fabsf(b) + ra.cell_bound[c]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) probe_mx = fmaxf(probe_mx, __shfl_xor(probe_mx, d, 64));
    if (lane == 0) red[NW + wave] = probe_mx;
  }
  __syncthreads();
  TPQ_PROF(a, blockIdx.x, 2);

  // delta >= |fast - exact|: both are fp32 sums of the same M terms in different orders, each
  // within (M-1) u * sum|x_i| of the real sum (u = 2^-24), and sum|x_i| <= sum_j max_c|LUT[j][c]|.
  // RES: the terms are base_p, part1_j, part2_j: exact = M sequential adds of fl(part1_j+part2_j)
  // onto base_p, fast = (M-1)-add sums of the part1's and of the part2's plus two more adds: each
  // within (M+1) u A of the real sum, A = |base_p| + sum_j max|part1_j| + cell_bound[cell_p]
  // (the host passes delta_rel with M+1 in place of M-1).
  // (sum_j max_c|LUT[j][c]| from the maxima collected while staging; every wave reduces the same
  // M words in the same order, so all of them hold the identical bound)
  float bound = 0.f;
#pragma unroll
  for (int j0 = 0; j0 < M; j0 += 64)
    if (j0 + lane < M) bound += __uint_as_float(jmax[j0 + lane]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) bound += __shfl_xor(bound, d, 64);
  __syncthreads();  // jmax lives in the queue area: everyone has read it before the first push
  if constexpr (RES) {
    float mx = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) mx = fmaxf(mx, red[NW + w]);
    bound += mx;
  }
  float delta2 = 2.f * delta_rel * bound;  // 2*delta: width of the candidate band
  if constexpr (SEL16) {
    // in table units: the quantisation (0.51 per entry, + 1) and the exact value's own distance from the real sum
    // ((M - 1) u bound = delta_rel bound / 2.1, taken as delta_rel bound / 2)
    delta2 = ceilf(2.f * (0.51f * (float)M + 1.f + 0.5f * delta_rel * bound * inv16)) + 1.f;
  } else if constexpr (DUMP) {
    // (a bound that is not finite: leave the query to the exact kernel, as the 16-bit table does)
    const bool ok = bound <= 1e37f;
    if (threadIdx.x == 0 && part == 0) a.flags[q] = ok ? 0 : a.epoch;
    if (!ok) return;
  }
  TPQ_PROF(a, blockIdx.x, 3);

  WaveSelector<R> sel;
  sel.init(qv_all + wave * 64, qi_all + wave * 64, a.k);
  sel.margin = delta2;
  typename WaveSelector<R>::Pool pool{nullptr, nullptr, 0, 0};
  if constexpr (POOL) {
    const int64_t o = (((int64_t)q * a.n_split + part) * NW + wave) * a.pool_cap;
    pool = {a.pool_hi + o, a.pool_lo + o, 0, a.pool_cap};
  }

  const int total_tiles = tab.tile_begin[n_probe];
  const int t_begin = (int)(((int64_t)total_tiles * part) / parts);
  const int t_end = (int)(((int64_t)total_tiles * (part + 1)) / parts);

  // Workgroup-shared admission threshold.  Two valid lower bounds of the final k-th best:
  //  (a) any wave's own k-th best (tau_key, atomic max);
  //  (b) min over the 8 waves of each wave's r-th best, r = ceil(k/8): the 8 lists then hold
  //      >= 8r >= k candidates at or above it.  Tiles are dealt round-robin to the waves, so
  //      (b) tracks the true k-th best closely and keeps the pass rate near k*ln(N/k)/N.
  const int r_share = (a.k + NW - 1) / NW;
  // readers poll ONE word per tile; the (rare) publisher folds bound (b) into it
  auto refresh_tau = [&]() {
    sel.tau = fmaxf(sel.tau, key2f(lds_poll_u32(tau_key)));
  };
  auto publish = [&](float /*tau_before*/) {
    // readlane must run with every lane active: inside `if (lane == 0)` the source lane is
    // inactive and its register contents are undefined to the compiler
    const float mine = sel.top.kth_value(r_share);
    if (lane == 0) {
      lds_post_f32(wave_q + wave, mine);
      float qmin = lds_poll_f32(wave_q);
#pragma unroll
      for (int w = 1; w < NW; ++w) qmin = fminf(qmin, lds_poll_f32(wave_q + w));
      atomicMax(tau_key, f2key(fmaxf(sel.tau, qmin)));
    }
  };

  constexpr bool kOneAhead = R > 4 || (R >= 2 && NW == 8 && !DUMP);  // (tile loop of m <= 64: see there)
  if constexpr (packed_slots(M) == 1) {
    constexpr int kFetchLoads = L::kChunks + (RES ? 1 : 0);  // global loads of one fetch (without tombstones)
    struct Tile {
      int s;
      bool valid;
      float add;      // RES: base_p + slot_term[s]
      uint32_t lim;   // the cell's last slot (a wave past its last tile: slot 0)
    };
    int p = 0;
    // Every global load of the tile loop is UNCONDITIONAL, on a clamped address (round 6).  With the prefetch under
    // `if (next tile exists) if (lane has a slot)` hipcc's waitcnt bookkeeping merged the two paths at the join and
    // put `s_waitcnt vmcnt(3 .. 0)` in front of the four chunks of the CURRENT tile's look-ups -- i.e. the wave waited for
    // the first chunks of the tile it had just prefetched before consuming the tile already in its registers (the ISA
    // of the loop: eight loads in flight wanted vmcnt(7 .. 4)).  A lane without a slot, and the whole wave past its
    // last tile, read the LAST slot of the tile's cell instead (one v_min_u32 against a wave-uniform bound -- was compare +
    // select of slot 0; the line is one the live lanes touch anyway; a wave past its last tile: slot 0, a tile exists, so
    // slot 0 does) and drop the value.
    auto locate = [&](int T) -> Tile {
      while (T >= tab.tile_begin[p + 1]) ++p;
      const int off = ((T - tab.tile_begin[p]) << 6) + lane;
      const int st = tab.start[p], sz = tab.size[p];
      Tile t{st + off, off < sz, 0.f, (uint32_t)(st + sz - 1)};
      return t;
    };
    auto fetch = [&](int T, Tile& t, typename L::chunk_t (&w)[L::kChunks]) {
      if (T < t_end) {  // (wave-uniform; nothing is loaded from global memory inside)
        t = locate(T);
      } else {
        t.valid = false;
        t.lim = 0u;
      }
      const uint32_t s = min((uint32_t)t.s, t.lim);
      L::load_u(a.packed, a.n_slots, s, w);
      if constexpr (RES) t.add = (T < t_end ? pbase[p] : 0.f) + ra.slot_term[s];
    };
    // (a lane without a slot carries NaN: it fails the admission compare by itself -- no `live` flag is kept in a register
    // next to the value; the scan is VALU-issue-bound.  Tombstones -- a foreign index with holes inside its cells,
    // ivfpq_topk.cu:878,883-884 -- are looked up for the candidates that PASS the threshold only (round 6; the flag bytes
    // used to travel with the prefetch: one more load per slot in flight, a number of loads per fetch that depended on the
    // call, and a fetch whose loads hipcc's waitcnt bookkeeping could not count exactly).)
    auto consume = [&](const typename L::chunk_t(&w)[L::kChunks], const Tile& t) {
      float v = __builtin_nanf("");
      if (t.valid) {
        if constexpr (SEL16) v = (float)L::accumulate16(w, t.s, reinterpret_cast<const uint16_t*>(lut));
        else v = L::accumulate(w, t.s, lut);
        if constexpr (RES) v += t.add;
      }
      // Every load of THIS tile has landed on every path past this point -- said explicitly (round 6): a wave whose tile has
      // no live lane branches around the look-ups and their `s_waitcnt vmcnt(7 .. 4)`, hipcc's waitcnt bookkeeping merged
      // that path in at the loop header, saw a load pending on the registers the next fetch reuses as temporaries and put
      // `s_waitcnt vmcnt(0)` in front of every other prefetch: the wave drained its loads before issuing the next tile's.
      // What remains in flight here is the prefetched tile (one fetch = kFetchLoads loads; with tombstones one more per
      // slot: that call waits for the first of them too).
      if constexpr (M <= 64) wait_vmcnt<kFetchLoads>();
      refresh_tau();
      const float tau_before = sel.tau;
      const int flushes_before = sel.n_flush;
      bool pass = v >= sel.tau - delta2;
      if (a.is_empty) {  // (wave-uniform)
        if (pass) pass = a.is_empty[t.s] == 0;
      }
      if constexpr (POOL) sel.push_pool(pool, pass, v, t.s);
      else sel.push(pass, v, t.s);
      if (sel.n_flush != flushes_before) publish(tau_before);
    };

    // software pipeline: the codes of tile T+NW are in flight while tile T is being consumed
    // (m <= 64; larger m runs 16 waves per workgroup under a 128-VGPR cap and relies on them)
    if constexpr (M <= 64) {
      typename L::chunk_t w0[L::kChunks], w1[L::kChunks];
      Tile m0{0, false, 0.f, 0u}, m1{0, false, 0.f, 0u};
      // TWO tiles ahead (round 6): a register set is refilled -- with the tile after next -- right behind its own
      // look-ups, so one to two tiles of loads are in flight at every moment and the probe-table walk of a fetch uses the
      // registers of the tile just consumed as its temporaries: m = 16 +5 %, 24 +4..13 %, 48 +4..7 % on the same box.
      // (hipcc re-rotates the loop and still puts `s_waitcnt vmcnt(0)` in front of every other prefetch -- DESIGN 3.1 --,
      // so the wave does drain once per two tiles; what the order buys is the earlier issue of the other prefetch.)
      // (Lists of two registers and more in the eight-wave workgroups of the sorted-list path -- m > 32, k = 300 / 500 --
      // keep the one-ahead order: two ahead cost them 4-5 % on the same box.)
      int T = t_begin + wave;
      if constexpr (kOneAhead) {
        if (T < t_end) fetch(T, m0, w0);
        while (T < t_end) {
          fetch(T + NW, m1, w1);
          consume(w0, m0);
          T += NW;
          if (T >= t_end) break;
          fetch(T + NW, m0, w0);
          consume(w1, m1);
          T += NW;
        }
      } else if (T < t_end) {  // (a wave without a tile loads nothing: slot 0 need not exist)
        fetch(T, m0, w0);
        fetch(T + NW, m1, w1);
#ifdef TPQ_SCAN_PROFILE
        bool first_tile = true;
#endif
        while (true) {
          consume(w0, m0);
#ifdef TPQ_SCAN_PROFILE
          if (first_tile) TPQ_PROF(a, blockIdx.x, 14);
          first_tile = false;
#endif
          fetch(T + 2 * NW, m0, w0);
          T += NW;
          if (T >= t_end) break;
          consume(w1, m1);
          fetch(T + 2 * NW, m1, w1);
          T += NW;
          if (T >= t_end) break;
        }
      }
    } else {
      // One 16-wave workgroup per CU and one tile in flight per wave: with a static deal the waves
      // drift apart (the oldest wave of a SIMD wins the issue arbitration), the early finishers
      // idle at the end-of-query barrier and the stragglers run alone, latency-bound -- 37-41 % of
      // the workgroup's life at m = 120.  Tiles are therefore handed out from an LDS counter (one
      // integer atomic per tile, fetched while the previous tile is consumed); a wave's tile
      // indices still increase, which is all locate() needs.
      auto grab = [&]() -> int {
        int t = 0;
        if (lane == 0) t = atomicAdd(tile_ctr, 1);
        return t_begin + __builtin_amdgcn_readfirstlane(t);
      };
      typename L::chunk_t w0[L::kChunks];
      Tile m0{0, false, 0.f, 0u};
      int T = grab();
      while (T < t_end) {
        fetch(T, m0, w0);
        const int Tn = grab();
        consume(w0, m0);
        T = Tn;
      }
    }
  } else {
    constexpr int S = packed_slots(M);          // slots per lane per tile, 64 apart
    constexpr int TS = packed_tile_shift(M);    // log2(slots per tile)
    constexpr int kFetchLoads = S * (L::kChunks + (RES ? 1 : 0));  // global loads of one fetch (without tombstones)
    struct Tile {
      int s;      // the lane's first slot; its u-th slot is s + 64 u
      int rem;    // slots of the cell from s on: the u-th slot exists iff 64 u < rem
      float add;  // RES: base_p (slot_term is added per slot)
      uint32_t lim;  // the cell's last slot (a wave past its last tile: slot 0)
    };
    int p = 0;
    auto locate = [&](int T) -> Tile {
      while (T >= tab.tile_begin[p + 1]) ++p;
      const int off = ((T - tab.tile_begin[p]) << TS) + lane;
      const int st = tab.start[p], sz = tab.size[p];
      Tile t{st + off, sz - off, 0.f, (uint32_t)(st + sz - 1)};
      if constexpr (RES) t.add = pbase[p];
      return t;
    };
    // (every global load unconditional, on a clamped address: see the one-slot-per-lane loop above)
    struct Side {
      float term[S];     // RES: slot_term of the lane's slots
    };
    auto fetch = [&](int T, Tile& t, typename L::chunk_t (&w)[S][L::kChunks], Side& sd) {
      if (T < t_end) {  // (wave-uniform; nothing is loaded from global memory inside)
        t = locate(T);
      } else {
        t.rem = 0;
        t.lim = 0u;
      }
  #pragma unroll
      for (int u = 0; u < S; ++u) {
        // (a slot past the end of the cell: the cell's last slot; a wave past its last tile: slot 0 -- read and dropped)
        const uint32_t su = min((uint32_t)(t.s + 64 * u), t.lim);
        L::load_u(a.packed, a.n_slots, su, w[u]);
        if constexpr (RES) sd.term[u] = ra.slot_term[su];
      }
    };
    auto consume = [&](const typename L::chunk_t (&w)[S][L::kChunks], const Side& sd, const Tile& t) {
      // (a lane's missing slot carries NaN: it fails the admission compare by itself; tombstones are looked up for the
      // passing candidates only: see the one-slot-per-lane loop above)
      float v[S];
  #pragma unroll
      for (int u = 0; u < S; ++u) {
        v[u] = __builtin_nanf("");
        if (64 * u < t.rem) {
          if constexpr (SEL16) v[u] = (float)L::accumulate16(w[u], t.s + 64 * u, reinterpret_cast<const uint16_t*>(lut));
          else v[u] = L::accumulate(w[u], t.s + 64 * u, lut);
          if constexpr (RES) v[u] += t.add + sd.term[u];
        }
      }
      // (this tile's loads have landed on every path: see the one-slot-per-lane loop above)
      if constexpr (M <= 64) wait_vmcnt<kFetchLoads>();
      refresh_tau();
      if constexpr (S > 1) {
        bool any = false;
  #pragma unroll
        for (int u = 0; u < S; ++u) any = any || (v[u] >= sel.tau - delta2);
        if (__ballot(any) == 0ull) return;  // the common case: one ballot for S x 64 slots
      }
  #pragma unroll
      for (int u = 0; u < S; ++u) {
        const float tau_before = sel.tau;
        const int flushes_before = sel.n_flush;
        bool pass = v[u] >= sel.tau - delta2;
        if (a.is_empty) {  // (wave-uniform)
          if (pass) pass = a.is_empty[t.s + 64 * u] == 0;
        }
        if constexpr (POOL) sel.push_pool(pool, pass, v[u], t.s + 64 * u);
        else sel.push(pass, v[u], t.s + 64 * u);
        if (sel.n_flush != flushes_before) {
          publish(tau_before);
          // (the tile's remaining slots meet the threshold the flush just raised -- the first tiles of a query admit
          // everything, and a short list, 32 probes of 244 slots at k = 100, spends as much on its flushes as on its look-ups)
          refresh_tau();
        }
      }
    };

    // software pipeline: the codes of tile T+NW are in flight while tile T is being consumed
    // (m <= 64; larger m runs 16 waves per workgroup under a 128-VGPR cap and relies on them)
    if constexpr (M <= 64) {
      typename L::chunk_t w0[S][L::kChunks], w1[S][L::kChunks];
      Side r0 = {}, r1 = {};
      Tile m0{0, 0, 0.f, 0u}, m1{0, 0, 0.f, 0u};
      // (two tiles ahead, one ahead for long lists: see the one-slot-per-lane loop above)
      int T = t_begin + wave;
      if constexpr (kOneAhead) {
        if (T < t_end) fetch(T, m0, w0, r0);
        while (T < t_end) {
          fetch(T + NW, m1, w1, r1);
          consume(w0, r0, m0);
          T += NW;
          if (T >= t_end) break;
          fetch(T + NW, m0, w0, r0);
          consume(w1, r1, m1);
          T += NW;
        }
      } else if (T < t_end) {  // (a wave without a tile loads nothing: slot 0 need not exist)
        fetch(T, m0, w0, r0);
        fetch(T + NW, m1, w1, r1);
        while (true) {
          consume(w0, r0, m0);
          fetch(T + 2 * NW, m0, w0, r0);
          T += NW;
          if (T >= t_end) break;
          consume(w1, r1, m1);
          fetch(T + 2 * NW, m1, w1, r1);
          T += NW;
          if (T >= t_end) break;
        }
      }
    } else {
      // One 16-wave workgroup per CU and one tile in flight per wave: with a static deal the waves
      // drift apart (the oldest wave of a SIMD wins the issue arbitration), the early finishers
      // idle at the end-of-query barrier and the stragglers run alone, latency-bound -- 37-41 % of
      // the workgroup's life at m = 120.  Tiles are therefore handed out from an LDS counter (one
      // integer atomic per tile, fetched while the previous tile is consumed); a wave's tile
      // indices still increase, which is all locate() needs.
      auto grab = [&]() -> int {
        int t = 0;
        if (lane == 0) t = atomicAdd(tile_ctr, 1);
        return t_begin + __builtin_amdgcn_readfirstlane(t);
      };
      typename L::chunk_t w0[S][L::kChunks];
      Side r0 = {};
      Tile m0{0, 0, 0.f, 0u};
      int T = grab();
      while (T < t_end) {
        fetch(T, m0, w0, r0);
        const int Tn = grab();
        consume(w0, r0, m0);
        T = Tn;
      }
    }
  }
  TPQ_PROF(a, blockIdx.x, 4);
  {
    const float tau_before = sel.tau;
    sel.flush();
    publish(tau_before);
  }
  TPQ_PROF(a, blockIdx.x, 5);

  if constexpr (DUMP) {
    // ---- dump mode: the wave's list of fast values, whether it may have lost one, the band -- and out ----
    // (a flush folds at most 64 candidates in: a list of 64 R entries that has seen no more than R flushes evicted nothing)
    const int64_t li = ((int64_t)q * a.n_split + part) * NW + wave;
    store_list<R>(sel.top, a.ws_vals + li * (R * 64), a.ws_idx + li * (R * 64));
    if (lane == 0) a.list_evict[li] = sel.n_flush > R ? 1 : 0;
    if (part == 0 && wave == 0 && lane == 0) a.ws_delta[q] = delta2;
    TPQ_PROF(a, blockIdx.x, 6);
    return;
  } else if constexpr (POOL) {
    // ---- pool mode: cut, compaction, exact values ----
    static_assert(!RES, "pool mode serves plain PQ");
    __syncthreads();  // every wave has published its quantile
    TPQ_PROF(a, blockIdx.x, 6);
    float shared_tau;
    {
      float qmin = lds_poll_f32(wave_q);
#pragma unroll
      for (int w = 1; w < NW; ++w) qmin = fminf(qmin, lds_poll_f32(wave_q + w));
      shared_tau = fmaxf(qmin, key2f(lds_poll_u32(tau_key)));
    }
    constexpr int PR = pool_regs(RM);  // pool registers: pool_cap = 64 PR entries (1024 / 2048)
    constexpr int kRounds = pool_rounds(RM);
    const bool overflow = pool.n > pool.cap;
    const int n_use = overflow ? 0 : pool.n;
    unsigned ph[PR], pl[PR];
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      ph[r] = 0u;
      pl[r] = 0u;
    }
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      if (r * 64 >= n_use) break;  // wave-uniform
      const int e = r * 64 + lane;
      const bool valid = e < n_use;
      // (agent-scope loads: the wave reads back what it stored itself, past its L1)
      ph[r] = valid ? __hip_atomic_load(pool.hi + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      pl[r] = valid ? __hip_atomic_load(pool.lo + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    }
    // counting rounds over the pools: invariant "at least k pool entries of the workgroup are >= lo"
    unsigned lo = f2key(shared_tau), hi = 0xFFFFFFFFu;
    {
      unsigned* cnt = reinterpret_cast<unsigned*>(qv_all);  // [3][NW][NW] (the queues are empty)
      auto count_ge = [&](unsigned t) -> unsigned {
        unsigned c = 0;
#pragma unroll
        for (int r = 0; r < PR; ++r) {
          if (r * 64 >= n_use) break;  // wave-uniform
          c += (unsigned)__popcll(__ballot(ph[r] >= t && ph[r] != 0u));
        }
        return c;
      };
      auto wave_max = [&](unsigned x) -> unsigned {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
          const unsigned o = (unsigned)__shfl_xor((int)x, d, 64);
          x = o > x ? o : x;
        }
        return x;
      };
#pragma unroll 1
      for (int round = 0; round < kRounds; ++round) {
        unsigned my_t = 0;
        if (round == 0) {
          if (lane < NW) my_t = f2key(lds_poll_f32(wave_q + lane));
        } else {
          const unsigned long long span = (unsigned long long)(hi - lo);
          my_t = lo + (unsigned)((span * (unsigned)(lane + 1)) / (unsigned)(NW + 1));
        }
        unsigned mine = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          const unsigned c = count_ge((unsigned)__builtin_amdgcn_readlane((int)my_t, j));
          mine = (lane == j) ? c : mine;
        }
        unsigned* cr = cnt + (round % 2) * NW * NW;
        if (lane < NW) cr[wave * NW + lane] = mine;
        __syncthreads();
        unsigned total = 0;
        if (lane < NW) {
#pragma unroll
          for (int w = 0; w < NW; ++w) total += cr[w * NW + lane];
        }
        const bool in = lane < NW;
        const bool ok = in && total >= (unsigned)a.k;
        const unsigned best_ok = wave_max(ok ? my_t : 0u);
        const unsigned best_no = ~wave_max((in && !ok) ? ~my_t : 0u);
        lo = best_ok > lo ? best_ok : lo;
        hi = best_no < hi ? best_no : hi;
        if (hi == 0xFFFFFFFFu || hi <= lo) break;  // workgroup-uniform
      }
    }
    __syncthreads();  // the counts lay over the queues
    TPQ_PROF(a, blockIdx.x, 7);
    const float cut = fmaxf(shared_tau, key2f(lo)) - delta2;
    constexpr int RR = refine_rows(M);
    constexpr int RX = NW == 4 ? 8 : 4;  // the wave's exact candidates, sorted: ~2 ceil(k / NW) entries at k = 1000
    uint32_t* scratch = scratch_all + wave * RR * (M / 4 + 1);
    int* qi = qi_all + wave * 64;
    int qn = 0, n_out = 0;
    WaveTopK<RX> ex;
    ex.init();
    auto drain = [&]() {  // the (<= 64) queued addresses: exact values, folded into the wave's sorted list
      if (qn == 0) return;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      const bool act = lane < qn;
      const int idx = act ? qi[lane] : 0;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      typename L::chunk_t cw[L::kChunks] = {};
      if (act) L::load(a.packed, a.n_slots, idx, cw);
      const float e = exact_lane<M>(cw, idx, lut);
      ex.insert_unsorted(act ? make_key(e + 0.0f, idx) : pad_key());
      n_out += qn;
      qn = 0;
    };
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      if (r * 64 >= n_use) break;  // wave-uniform
      const bool want = ph[r] != 0u && key2f(ph[r]) >= cut;
      const unsigned long long wmask = __ballot(want);
      if (wmask == 0ull) continue;
      const int n = __popcll(wmask);
      if (qn + n > 64) drain();
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(wmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)wmask, 0));
      if (want) qi[qn + rank] = (int)~pl[r];
      qn += n;
    }
    drain();
    // the sorted list goes where the pool was (its entries are all in registers by now); more candidates than
    // the list holds, or a pool that filled up: the exact kernel redoes the query
    store_list<RX>(ex, reinterpret_cast<float*>(pool.hi), reinterpret_cast<int*>(pool.lo));
    if (lane == 0 && (overflow || n_out > 64 * RX)) a.flags[q] = a.epoch;
    TPQ_PROF(a, blockIdx.x, 8);
    TPQ_PROF(a, blockIdx.x, 9);
    return;
  } else {

  // End of query, per wave and without any barrier: re-evaluate the surviving candidates of
  // this wave's list exactly (ascending j, LUT still in LDS), re-rank them by exact value and
  // dump the list; scan_merge_refine_kernel (one wave per query) merges the 8 x n_split lists.
  // Only entries that can still reach the top-k (f >= shared threshold - 2*delta) are touched:
  // with the quantile-shared threshold that is ~k/8 per wave, i.e. one 16-lane pass.
  {
    // One barrier: every wave has folded its last queue in and published its r-th best, so the
    // shared bound (b) is now computed from FRESH lists.  During the scan the lists lag (a wave
    // admits only ~k*ln(N/k)/NW candidates in its whole life and folds them in 64 at a time), so
    // the running threshold leaves ~100 entries per wave above it; the fresh bound leaves ~2k/NW.
    __syncthreads();
    TPQ_PROF(a, blockIdx.x, 6);
    float shared_tau;  // identical in every wave (the loop below must be workgroup-uniform)
    {
      float qmin = lds_poll_f32(wave_q);
#pragma unroll
      for (int w = 1; w < NW; ++w) qmin = fminf(qmin, lds_poll_f32(wave_q + w));
      shared_tau = fmaxf(qmin, key2f(lds_poll_u32(tau_key)));
      sel.tau = fmaxf(sel.tau, shared_tau);
    }
    // Two counting rounds pull the bound up to (nearly) the exact k-th best fast value of the
    // workgroup: invariant "at least k list entries are >= lo".  Round 0 tests the NW published
    // quantiles themselves, round 1 NW keys evenly spaced inside the bracket round 0 leaves; every
    // wave counts its own sorted registers (ballots), the NW x NW counts meet in the dead queue
    // area, and each wave reduces them redundantly -- two barriers, no list ever leaves registers.
    // Every candidate kept beyond the k-th costs an exact re-evaluation (M gathers; M cache lines
    // of the part2 table in the residual kernel), so the tight cut pays for itself.
    {
      unsigned* cnt = reinterpret_cast<unsigned*>(qv_all);  // [2][NW][NW]
      auto count_ge = [&](unsigned t) -> unsigned {
        unsigned c = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) c += (unsigned)__popcll(__ballot(sel.top.k[r].hi >= t));
        return c;
      };
      auto wave_max = [&](unsigned x) -> unsigned {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
          const unsigned o = (unsigned)__shfl_xor((int)x, d, 64);
          x = o > x ? o : x;
        }
        return x;
      };
      unsigned lo = f2key(shared_tau), hi = 0xFFFFFFFFu;
#pragma unroll 1
      for (int round = 0; round < 2; ++round) {
        unsigned my_t = 0;  // lane j < NW: threshold j of this round
        if (round == 0) {
          if (lane < NW) my_t = f2key(lds_poll_f32(wave_q + lane));
        } else {
          const unsigned long long span = (unsigned long long)(hi - lo);
          my_t = lo + (unsigned)((span * (unsigned)(lane + 1)) / (unsigned)(NW + 1));
        }
        unsigned mine = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          const unsigned c = count_ge((unsigned)__builtin_amdgcn_readlane((int)my_t, j));
          mine = (lane == j) ? c : mine;
        }
        unsigned* cr = cnt + round * NW * NW;
        if (lane < NW) cr[wave * NW + lane] = mine;
        __syncthreads();
        unsigned total = 0;
        if (lane < NW) {
#pragma unroll
          for (int w = 0; w < NW; ++w) total += cr[w * NW + lane];
        }
        const bool in = lane < NW;
        const bool ok = in && total >= (unsigned)a.k;
        const unsigned best_ok = wave_max(ok ? my_t : 0u);           // largest threshold still >= k
        const unsigned best_no = ~wave_max((in && !ok) ? ~my_t : 0u);  // smallest one below k
        lo = best_ok > lo ? best_ok : lo;
        hi = best_no < hi ? best_no : hi;
        if (hi == 0xFFFFFFFFu || hi <= lo) break;  // wave-uniform: nothing left to bracket
      }
      sel.tau = fmaxf(sel.tau, key2f(lo));
    }
    TPQ_PROF(a, blockIdx.x, 7);
    const float cut = sel.tau - delta2;
    if (a.small_lists) {
      // Large k: the per-wave lists hold 64R < k + 8 entries (tiles are dealt round-robin, so a
      // wave's share of the top-k is ~k/NW; R is sized for twice that).  A wave whose list is FULL
      // of candidates that can still matter may have evicted one that matters too: flag the query
      // for the exact kernel.  (A list whose worst entry is below the cut lost nothing: everything
      // it evicted was worse still.)
      // (A flush folds at most 64 candidates in, so a list of 64 R entries that has seen no more than R
      // flushes evicted nothing at all: a query of a few hundred slots -- n_probe 1 or 2 on the reference's
      // benchmark grid -- fills lists whose cut is still -inf, and must not take the exact redo for it.)
      const Key kl = readlane_key(sel.top.k[R - 1], 63);
#ifndef TPQ_EXP_NO_OVERFLOW_FLAG  // knock-out for tests/test_gpu_kernels.py's adversarial case
      // (write-through, agent scope: with the fused finish the reader is the query's LAST workgroup, possibly on
      // another XCD, inside this launch -- a plain store could still sit in this XCD's L2 when it looks)
      if (sel.n_flush > R && key_index(kl) != kPadIdx && key_value(kl) >= cut && lane == 0)
        __hip_atomic_store(a.flags + q, a.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
    constexpr int RR = refine_rows(M);
    uint32_t* scratch = scratch_all + wave * RR * (M / 4 + 1);
    WaveTopK<R> ex;
    ex.init();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int idx = key_index(sel.top.k[r]);
      const bool want = (idx != kPadIdx) && (key_value(sel.top.k[r]) >= cut);
      const unsigned long long wmask = __ballot(want);
      if (wmask == 0ull) break;  // sorted by fast value: nothing further down qualifies either
      float e = -INFINITY;
      float init = 0.f;
      const float* p2 = ra.part2;
      if constexpr (RES) {
        // which probe does the candidate's slot belong to?  (first match in probe order; a slot
        // covered by two probes -- a cell listed twice, non-adjacent -- is scanned twice by the
        // reference with two different bases: leave such queries to the exact kernel)
        int myp = -1, n_match = 0;
        for (int pp = 0; pp < n_probe; ++pp) {
          const bool hit = want && ((unsigned)(idx - tab.start[pp]) < (unsigned)tab.size[pp]);
          myp = (hit && myp < 0) ? pp : myp;
          n_match += hit ? 1 : 0;
        }
        if (n_match > 1) a.flags[q] = a.epoch;
        myp = myp < 0 ? 0 : myp;
        init = pbase[myp];
        p2 = ra.part2 + (int64_t)pcell[myp] * (M * 256);
      }
      // every wanted lane fetches its candidate's packed bytes NOW, in one batch: loaded inside the passes
      // below (16 rows each: the un-permute scratch is 16 rows per wave), each pass waited out a memory
      // latency of its own -- 6.5 of the 45 us a 16-probe query of 244-slot cells lives at k = 100
      typename L::chunk_t cw[L::kChunks] = {};
      if (want) L::load(a.packed, a.n_slots, idx, cw);
#pragma unroll 1
      for (int pass = 0; pass < 64 / RR; ++pass) {
        if (((wmask >> (RR * pass)) & ((1ull << RR) - 1ull)) == 0ull) continue;  // wave-uniform
        const bool mine = want && ((lane / RR) == pass);
        float ep;
        if constexpr (RES)
          ep = exact_from_chunks<M>(cw, idx, mine, scratch, lane % RR, ResidualLut<M>{lut, p2}, init);
        else
          ep = exact_from_chunks<M>(cw, idx, mine, scratch, lane % RR, LdsLut<M>{lut});
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        e = mine ? ep : e;
      }
      ex.insert_unsorted(want ? make_key(e, idx) : pad_key());
    }
    TPQ_PROF(a, blockIdx.x, 8);
    if constexpr (is_fused(RM) && !RES) {
      static_assert(RM >= R, "merged list shorter than the per-wave lists");
      // ---- fused finish ----
      WaveTopK<RM> mt;
      mt.init();
#pragma unroll
      for (int r = 0; r < R; ++r) mt.k[r] = ex.k[r];  // (sorted; the pads of init() rank last)
      float* lv = reinterpret_cast<float*>(smem);     // [NW][RM 64] x 2: over the LUT, the rows and the queues
      int* li = reinterpret_cast<int*>(smem + (size_t)NW * RM * 64 * 4);
      int* s_flag = tile_ctr;                         // (dead: m > 64 hands tiles out of it during the scan only)
      auto tree = [&]() {  // NW lists -> wave 0
        for (int stride = 1; stride < NW; stride <<= 1) {
          if ((wave & (2 * stride - 1)) == stride) store_list<RM>(mt, lv + wave * RM * 64, li + wave * RM * 64);
          __syncthreads();
          if ((wave & (2 * stride - 1)) == 0)
            merge_list<RM>(mt, lv + (wave + stride) * RM * 64, li + (wave + stride) * RM * 64);
          __syncthreads();
        }
      };
      // (merge area: over the LUT, the rows and the queues -- everything below the probe table: fuse_fits())
      unsigned* mhi = reinterpret_cast<unsigned*>(smem);
      auto load_merged = [&](const unsigned* ohi, const unsigned* olo) {
#pragma unroll
        for (int r = 0; r < RM; ++r) mt.k[r] = Key{ohi[r * 64 + lane], olo[r * 64 + lane]};
      };
      __syncthreads();  // every wave is done with the LUT and its rows
      {  // the workgroup's NW lists -> one, by rank (rank_merge)
        constexpr int LEN = 64 * R;
        unsigned* mlo = mhi + NW * LEN;
        unsigned* ohi = mlo + NW * LEN;
        unsigned* olo = ohi + RM * 64;
        store_list<R>(ex, reinterpret_cast<float*>(mhi + wave * LEN), reinterpret_cast<int*>(mlo + wave * LEN));
        const Key pad = pad_key();
        for (int i = threadIdx.x; i < RM * 64; i += NW * 64) {
          ohi[i] = pad.hi;
          olo[i] = pad.lo;
        }
        __syncthreads();
        rank_merge<LEN>(mhi, mlo, NW, ohi, olo, RM * 64, (int)threadIdx.x, NW * 64);
        __syncthreads();
        if (wave == 0) load_merged(ohi, olo);
      }
      TPQ_PROF(a, blockIdx.x, 9);
      bool last = true;
      if (a.n_split > 1) {
        // the workgroup's list -> workspace; release; ticket.  (G16 of the CDNA guide: plain stores, wait,
        // agent-scope release by one lane, relaxed agent-scope ticket; the last arriver acquires)
        if (wave == 0) {
          const int64_t o = ((int64_t)q * a.n_split + part) * (RM * 64);
          // (write-through stores -- relaxed, agent scope: sc1 -- need no cache write-back before the ticket)
#pragma unroll
          for (int r = 0; r < RM; ++r) {
            __hip_atomic_store(reinterpret_cast<unsigned*>(a.ws_vals) + o + r * 64 + lane, mt.k[r].hi, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(reinterpret_cast<unsigned*>(a.ws_idx) + o + r * 64 + lane, mt.k[r].lo, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) {
            const int t = __hip_atomic_fetch_add(a.tickets + q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int is_last = t == a.n_split - 1;
            if (is_last) {
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
              a.tickets[q] = 0;  // (zero on exit: the next call's workgroups start from it)
            }
            *s_flag = is_last;
          }
        }
        __syncthreads();
        last = *s_flag != 0;
        TPQ_PROF(a, blockIdx.x, 10);
        if (last) {  // block-uniform
          // (plain loads: the acquire above invalidated this CU's view; the lists were written back by their
          // producers' releases)
          // (wave w folds the lists of splits w, w + NW, ...; then the tree.  Ranking 16 x 128 entries against
          // each other in LDS, as the workgroup's own lists are merged above, measured 26 us against 7)
          mt.init();
          for (int pp = wave; pp < a.n_split; pp += NW) {
            const int64_t o = ((int64_t)q * a.n_split + pp) * (RM * 64);
            merge_list<RM>(mt, a.ws_vals + o, a.ws_idx + o);
          }
          __syncthreads();
          tree();
        }
      } else {
        TPQ_PROF(a, blockIdx.x, 10);
      }
      if (!last) return;
      TPQ_PROF(a, blockIdx.x, 11);
      // wave 0 holds the query's list, exact values: write, and decide whether the band overflowed
      if (wave == 0) {
        const float ek = mt.kth_value(a.k);
        const Key klast = readlane_key(mt.k[RM - 1], 63);
        bool overflow = (key_index(klast) != kPadIdx) && !(key_value(klast) < ek - delta2);
        if (a.small_lists) overflow = overflow || (__hip_atomic_load(a.flags + q, __ATOMIC_RELAXED,
                                                                     __HIP_MEMORY_SCOPE_AGENT) == a.epoch);
        write_final<RM>(a, q, mt);
        if (lane == 0) {
          // the flag is consumed here: a graph replays with the SAME epoch, and a flag left raised would send
          // every later replay of this query through the redo (diagnostics: ws_delta[q] = 1 when it was redone)
          a.flags[q] = 0;
          a.ws_delta[q] = overflow ? 1.f : 0.f;
          *s_flag = overflow;
        }
      }
      __syncthreads();
      TPQ_PROF(a, blockIdx.x, 12);
      if (*s_flag == 0) return;
      // ---- the exact redo (normally never): this workgroup rescans the query's probed cells with the
      // reference's arithmetic (ascending j, from the packed bytes) and overwrites the result ----
      __syncthreads();
      if (threadIdx.x < M) jmax[threadIdx.x] = 0u;
      __syncthreads();
      stage_lut_blocked<M>(a, q, lut, NW * 64, jmax, xq, nullptr);  // (the merge buffers lay over it)
      __syncthreads();
      if (wave == 0 && lane == 0) *tau_key = f2key(-INFINITY);
      __syncthreads();
      WaveSelector<RM> xs;
      xs.init(qv_all + wave * 64, qi_all + wave * 64, a.k);
      for (int pp = 0; pp < n_probe; ++pp) {
        const int size = tab.size[pp], start = tab.start[pp];
        for (int off0 = wave * 64; off0 < size; off0 += NW * 64) {
          const int off = off0 + lane;
          const bool valid = off < size;
          const int sidx = start + (valid ? off : 0);
          float e = -INFINITY;
#pragma unroll 1
          for (int pass = 0; pass < 64 / RR; ++pass) {
            const bool mine = valid && ((lane / RR) == pass);
            const float ep = exact_from_packed<M>(a.packed, a.n_slots, sidx, mine, scratch, lane % RR, LdsLut<M>{lut});
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            e = mine ? ep : e;
          }
          bool live = valid;
          if (valid && a.is_empty) live = (a.is_empty[sidx] == 0);
          xs.tau = fmaxf(xs.tau, key2f(lds_poll_u32(tau_key)));
          const float tau_before = xs.tau;
          xs.push(live && (e >= xs.tau), e, sidx);
          if (xs.tau > tau_before && lane == 0) atomicMax(tau_key, f2key(xs.tau));
        }
      }
      xs.flush();
      mt = xs.top;
      __syncthreads();  // every wave is done with the LUT
      tree();
      if (wave == 0) write_final<RM>(a, q, mt);
      return;
    }
    const int64_t o = (((int64_t)q * a.n_split + part) * NW + wave) * (R * 64);
    store_list<R>(ex, a.ws_vals + o, a.ws_idx + o);
    TPQ_PROF(a, blockIdx.x, 9);
    if (part == 0 && wave == 0 && lane == 0) a.ws_delta[q] = delta2;
  }
  }  // (neither dump nor pool mode)
}

}  // namespace tpq
