// Scan-layout list scan: one translation unit per sub-quantizer count, compiled with
// -DTPQ_PACKED_M=<M> (build.sh) so the 5 x 2 x 5 kernel instantiations build in parallel.
// Device code: scan_device.h (one header per stage; the kernel itself: scan_packed_kernel.h); C ABI: scan.hip.
#include "scan_device.h"

#ifndef TPQ_PACKED_M
#error "compile with -DTPQ_PACKED_M=<n_subvectors>"
#endif

namespace tpq {

// delta = 1.05 * 2 (M-1) u * sum_j max|LUT_j|,  u = 2^-24   (residual: M+1 roundings, see the kernel)
constexpr float delta_rel(int M, bool RES) { return 1.05f * 2.0f * 5.9604645e-8f * (float)(RES ? M + 1 : M - 1); }

template <int RL, int R, int M, bool RES>
static int launch_packed(ScanArgs a, ResidualArgs ra, hipStream_t st) {
  size_t lds = scan_lds_bytes_packed(M, RL, a.max_nprobe, fused_floats_of(a), RES);
#ifdef TPQ_EXTRA_LDS  // experiment: force fewer workgroups per CU
  lds += TPQ_EXTRA_LDS;
#endif
  if constexpr (!RES && R <= kFuseMaxR) {
    if (a.fuse) {  // fused finish: one launch (scan.hip decides)
      int rc = set_lds(scan_packed_kernel<RL, M, false, R>, lds, "scan_packed_kernel (fused finish)");
      if (rc) return rc;
      hipLaunchKernelGGL((scan_packed_kernel<RL, M, false, R>), dim3((unsigned)a.nq * a.n_split),
                         dim3(packed_waves(M) * 64), lds, st, a, ra, delta_rel(M, false));
      TPQ_LAUNCH_CHECK("scan_packed_kernel (fused finish)");
      return TPQ_OK;
    }
  }
  int rc = set_lds(scan_packed_kernel<RL, M, RES>, lds, "scan_packed_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((scan_packed_kernel<RL, M, RES>), dim3((unsigned)a.nq * a.n_split),
                     dim3(packed_waves(M) * 64), lds, st, a, ra, delta_rel(M, RES));
  TPQ_LAUNCH_CHECK("scan_packed_kernel");
  const int n_lists = a.n_split * packed_waves(M);
  // merge waves per query: the largest power of two <= min(8, n_lists / 2) that divides n_lists
  // (n_lists = n_split x 4 / 8 / 16 waves: 2, 4 or 8)
  int W = 8;
  while (W > 1 && (W > n_lists / 2 || n_lists % W != 0)) W >>= 1;
  const size_t merge_lds = (size_t)W * R * 64 * 8;
  rc = set_lds(scan_merge_refine_kernel<RL, R, M, RES>, merge_lds, "scan_merge_refine_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((scan_merge_refine_kernel<RL, R, M, RES>), dim3(a.nq), dim3(W * 64), merge_lds, st, a);
  TPQ_LAUNCH_CHECK("scan_merge_refine_kernel");
  return TPQ_OK;
}

// pool mode (k > 248): scan with threshold lists of RL registers + pools (RM = -1: 1 024 entries per wave, -2: 2 048),
// then the ranking kernel
template <int RL, int M, int RM>
static int launch_pool(ScanArgs a, hipStream_t st) {
  const size_t lds = scan_lds_bytes_packed(M, RL, a.max_nprobe, fused_floats_of(a), false);
  int rc = set_lds(scan_packed_kernel<RL, M, false, RM>, lds, "scan_packed_kernel (pool mode)");
  if (rc) return rc;
  hipLaunchKernelGGL((scan_packed_kernel<RL, M, false, RM>), dim3((unsigned)a.nq * a.n_split),
                     dim3(packed_waves(M) * 64), lds, st, a, ResidualArgs{}, delta_rel(M, false));
  TPQ_LAUNCH_CHECK("scan_packed_kernel (pool mode)");
  constexpr int NW = packed_waves(M), LEN = 64 * (NW == 4 ? 8 : 4);
  const size_t mlds = (size_t)a.n_split * NW * LEN * 8 + (size_t)((a.k + 63) / 64 * 64) * 8;
  rc = set_lds(scan_pool_merge_kernel<NW>, mlds, "scan_pool_merge_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((scan_pool_merge_kernel<NW>), dim3(a.nq), dim3(kPoolMergeThreads), mlds, st, a);
  TPQ_LAUNCH_CHECK("scan_pool_merge_kernel");
  return TPQ_OK;
}

// the finish kernel at 4, 8 or 16 chunks of 64 keys per query, by the T = splits x waves x list registers a query comes in
template <int RM, int M, int DS, bool FROM_LUT, class Go>
static int finish_by_chunks(int T, Go&& go) {
  return T <= 4 ? go(scan_finish_exact_kernel<RM, M, DS, 4, FROM_LUT>)
                : (T <= 8 ? go(scan_finish_exact_kernel<RM, M, DS, 8, FROM_LUT>)
                          : go(scan_finish_exact_kernel<RM, M, DS, 16, FROM_LUT>));
}

// dump modes (scan_packed_kernel.h): the scan ends with the waves' lists of fast values; scan_finish_exact_kernel, one wave per
// query, evaluates the band's survivors exactly and writes the result.  m = 64: the 16-bit table (kDumpSel16 / W8);
// m = 8, 16, 32 (round 6): the fp32 table the four-wave workgroups of the short codes stream over anyway (kDumpF32) --
// what they gain is the early end of the scan workgroup.
// the finish kernel: survivors in RM = 2, 4 or 8 registers (k <= 56 rides on 2); the exact entries from the codebook
// in LDS (fused calls; sub-vector length 1 / 2 compiled in at m = 64, read from the arguments otherwise) or gathered from
// the caller's table (m <= 32); 4, 8 or 16 chunks of 64 keys per query.  seed_chunks, cnt: the cell-major form's stage 5
// (scan_finish.h) -- one list per query whose first seed_chunks chunks hold exact values, cnt[q] entries behind them
template <int RM, int M>
static int launch_finish(const ScanArgs& a, int nw_scan, int RL, hipStream_t st, int seed_chunks = 0,
                         const int* cnt = nullptr) {
  const bool from_lut = a.lut != nullptr;
  TPQ_REQUIRE(seed_chunks >= 0 && seed_chunks <= RM && seed_chunks <= a.n_split * nw_scan * RL,
              "scan_packed (finish): %d seed chunks beside %d list registers", seed_chunks, RM);
  TPQ_REQUIRE(!cnt || (a.n_split == 1 && RL == 1), "scan_packed (finish): entry counts take one list per query");
  const size_t flds = finish_lds_bytes(M, a.ds, RM, from_lut);
  // one persistent workgroup per CU (its LDS holds the codebook)
  int dev = 0, n_cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cus <= 0)
    n_cus = 256;
  constexpr int FW = finish_waves(RM);
  const int want = (a.nq + FW - 1) / FW;
  // (the table-gathering form holds no codebook: workgroups are cheap, two per CU hide the gathers' latency)
  const int cap = from_lut ? 2 * n_cus : n_cus;
  const dim3 grid((unsigned)(want < cap ? want : cap)), block(FW * 64);
  auto go = [&](auto kernel) -> int {
    int rc = set_lds(kernel, flds, "scan_finish_exact_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, grid, block, flds, st, a, nw_scan, RL, seed_chunks, cnt);
    TPQ_LAUNCH_CHECK("scan_finish_exact_kernel");
    return TPQ_OK;
  };
  const int T = a.n_split * nw_scan * RL;  // (16: the split tail of a batch, ScanArgs::unsplit)
  if constexpr (dump_built(M, kDumpSel16)) {
    if (a.ds == 1) return finish_by_chunks<RM, M, 1, false>(T, go);
    return finish_by_chunks<RM, M, 2, false>(T, go);
  } else {
    if (from_lut) return finish_by_chunks<RM, M, 0, true>(T, go);
    // (the sub-vector length of a 128-dimensional index compiled in: SIFT's m = 32 -> ds = 4; others read it)
    if (a.ds == 128 / M) return finish_by_chunks<RM, M, 128 / M, false>(T, go);
    return finish_by_chunks<RM, M, 0, false>(T, go);
  }
}

template <int RL, int R, int M, int MODE>
static int launch_dump(ScanArgs a, hipStream_t st) {
  const size_t lds = scan_lds_bytes_dump(M, is_sel16(MODE), scan_waves(M, MODE), a.max_nprobe, fused_floats_of(a));
  int rc = set_lds(scan_packed_kernel<RL, M, false, MODE>, lds, "scan_packed_kernel (dump mode)");
  if (rc) return rc;
  constexpr int NW = scan_waves(M, MODE);
  const unsigned blocks = (unsigned)a.unsplit + (unsigned)(a.nq - a.unsplit) * (unsigned)a.n_split;
  hipLaunchKernelGGL((scan_packed_kernel<RL, M, false, MODE>), dim3(blocks), dim3(NW * 64), lds, st, a,
                     ResidualArgs{}, delta_rel(M, false));
  TPQ_LAUNCH_CHECK("scan_packed_kernel (dump mode)");
  return launch_finish<(R < 2 ? 2 : R), M>(a, NW, RL, st);
}
// the pairs of TPQ_DUMP_PAIRS (scan_args.h), in its order; scan.hip plans no other (plan_scan)
template <int M, int MODE>
static int dispatch_dump_mode(const ScanArgs& a, int RL, int R, hipStream_t st) {
  if constexpr (dump_built(M, MODE)) {
#define TPQ_PAIR(MD, A, B) \
    if constexpr (MD == MODE) if (RL == A && R == B) return launch_dump<A, B, M, MODE>(a, st);
    TPQ_DUMP_PAIRS(TPQ_PAIR)
#undef TPQ_PAIR
  }
  set_error("scan_packed (dump mode %d): no instantiation for list registers (%d, %d) at m = %d", MODE, RL, R, M);
  return TPQ_ERR_UNSUPPORTED;
}

template <int M, bool RES>
static int dispatch_r(const ScanArgs& a, const ResidualArgs& ra, int RL, int R, hipStream_t st) {
  if (RL == R) {
    switch (R) {
      case 1: return launch_packed<1, 1, M, RES>(a, ra, st);
      case 2: return launch_packed<2, 2, M, RES>(a, ra, st);
      case 4: return launch_packed<4, 4, M, RES>(a, ra, st);
      case 8: return launch_packed<8, 8, M, RES>(a, ra, st);
      default: return launch_packed<16, 16, M, RES>(a, ra, st);
    }
  }
  // short per-wave lists (list_regs_scan): every (RL < R) pair
#define TPQ_PAIR(A, B) if (RL == A && R == B) return launch_packed<A, B, M, RES>(a, ra, st);
  TPQ_PAIR(1, 2) TPQ_PAIR(1, 4) TPQ_PAIR(1, 8) TPQ_PAIR(1, 16) TPQ_PAIR(2, 4) TPQ_PAIR(2, 8)
  TPQ_PAIR(2, 16) TPQ_PAIR(4, 8) TPQ_PAIR(4, 16) TPQ_PAIR(8, 16)
#undef TPQ_PAIR
  set_error("scan_packed: no instantiation for list registers (%d, %d)", RL, R);
  return TPQ_ERR_UNSUPPORTED;
}

#define TPQ_CAT2(a, b) a##b
#define TPQ_CAT(a, b) TPQ_CAT2(a, b)

int TPQ_CAT(dispatch_pool_, TPQ_PACKED_M)(const ScanArgs& a, int RL, hipStream_t st) {
  const bool big = a.pool_cap > 1024;
  switch (RL) {
    // (-3: the large pool without the counting rounds -- see kPoolRoundsFromK)
#define TPQ_POOL_CASE(RL)                                                                              \
  case RL:                                                                                             \
    return !big ? launch_pool<RL, TPQ_PACKED_M, -1>(a, st)                                             \
                : (a.k <= kPoolRoundsFromK ? launch_pool<RL, TPQ_PACKED_M, -3>(a, st)                  \
                                           : launch_pool<RL, TPQ_PACKED_M, -2>(a, st));
    TPQ_POOL_CASE(1)
    TPQ_POOL_CASE(2)
    TPQ_POOL_CASE(4)
#undef TPQ_POOL_CASE
    default: break;
  }
  set_error("scan_packed (pool mode): no instantiation for %d list registers", RL);
  return TPQ_ERR_UNSUPPORTED;
}

int TPQ_CAT(dispatch_dump_, TPQ_PACKED_M)(const ScanArgs& a, int RL, int R, int mode, hipStream_t st) {
  if (mode == kDumpSel16W8) return dispatch_dump_mode<TPQ_PACKED_M, kDumpSel16W8>(a, RL, R, st);
  if (mode == kDumpF32) return dispatch_dump_mode<TPQ_PACKED_M, kDumpF32>(a, RL, R, st);
  return dispatch_dump_mode<TPQ_PACKED_M, kDumpSel16>(a, RL, R, st);
}

// the finish kernel on its own (the cell-major form, scan_cells.hip): a query's lists arrive as `chunks` (8 or 16) lists
// of one chunk of 64 keys each; R = registers of the exact list (dump_finish_regs); the first seed_chunks of them hold
// exact values, cnt[q] entries follow (launch_finish)
int TPQ_CAT(dispatch_finish_, TPQ_PACKED_M)(const ScanArgs& a, int chunks, int R, int seed_chunks, const int* cnt,
                                            hipStream_t st) {
  if constexpr (dump_built(TPQ_PACKED_M, kDumpSel16)) {
    if (R <= 2) return launch_finish<2, TPQ_PACKED_M>(a, chunks, 1, st, seed_chunks, cnt);
    if (R == 4) return launch_finish<4, TPQ_PACKED_M>(a, chunks, 1, st, seed_chunks, cnt);
    if (R == 8) return launch_finish<8, TPQ_PACKED_M>(a, chunks, 1, st, seed_chunks, cnt);
  }
  set_error("scan_packed (finish): no instantiation for %d list registers at m = %d", R, TPQ_PACKED_M);
  return TPQ_ERR_UNSUPPORTED;
}

// workgroups of the dump-mode scan kernel (RL = 1, a 64-probe table, fused LUT at ds = 2) one CU holds; 0 = not built
template <int M, int MODE>
static int dump_occupancy_of() {
  if constexpr (!dump_built(M, MODE)) {
    return 0;
  } else {
    constexpr int NW = scan_waves(M, MODE);
    const size_t lds = scan_lds_bytes_dump(M, is_sel16(MODE), NW, 64, M * 2 + M);
    int n = 0;
    if (set_lds(scan_packed_kernel<1, M, false, MODE>, lds, "scan_packed_kernel (dump mode)") != TPQ_OK) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scan_packed_kernel<1, M, false, MODE>, NW * 64, lds) != hipSuccess)
      return 0;
    return n;
  }
}
int TPQ_CAT(dump_occupancy_, TPQ_PACKED_M)(int mode) {
  if (mode == kDumpSel16W8) return dump_occupancy_of<TPQ_PACKED_M, kDumpSel16W8>();
  if (mode == kDumpF32) return dump_occupancy_of<TPQ_PACKED_M, kDumpF32>();
  return dump_occupancy_of<TPQ_PACKED_M, kDumpSel16>();
}

int TPQ_CAT(dispatch_packed_, TPQ_PACKED_M)(const ScanArgs& a, const ResidualArgs* ra, int RL, int R,
                                            hipStream_t st) {
  if (ra) return dispatch_r<TPQ_PACKED_M, true>(a, *ra, RL, R, st);
  return dispatch_r<TPQ_PACKED_M, false>(a, ResidualArgs{}, RL, R, st);
}

}  // namespace tpq
