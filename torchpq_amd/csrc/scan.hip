// IVF list scan + top-k for gfx950 (MI355X).
//
// Replaces ivfpq_topk / ivfpq_top1 (torchpq/kernels/cuda/ivfpq_topk.cu:822-971,
// ivfpq_top1.cu:385-455) and their launchers (torchpq/kernels/IVFPQTopkCuda.py:81-142).
//
// Structure:
//   * one workgroup per (query, split); the query's 256-entry-per-sub-quantizer LUT (m KiB fp32)
//     is staged in LDS; each wave walks its round-robin share of the probed cells in 64-slot
//     tiles, one slot per lane, codes streamed straight from HBM to VGPRs;
//   * value(slot) = sum_j LUT[j][code_j] in fp32, ascending j from 0.f -- bit-identical to
//     consume_data (ivfpq_topk.cu:662-679);
//   * per-wave register top-k (wave_topk.h) + a workgroup-shared admission threshold in LDS;
//     no barrier inside the scan loop;
//   * n_split > 1 splits a query's tiles over several workgroups (small batches must still
//     fill 256 CUs; the reference's grid=(nq,) cannot).
//
// Kernels:
//   scan_ref_kernel      streams CellContainer._storage as is ([m/4][n_slots][4], any m % 4 == 0):
//                        the drop-in at the IVFPQTopkCuda.topk boundary and the exact fallback.
//                        LDS look-ups hit random banks (~3.5 cycles per half-wave access); the 8
//                        waves' lists are tree-merged in the workgroup.
//   scan_residual_kernel residual PQ (per-cell LUT), reference layout, exact.
//   scan_packed_kernel   streams the MI355X scan layout (pack.hip / scan_layout.h): per-slot
//                        XOR-permuted sub-quantizer order so the 32 lanes of a half-wave always
//                        read 32 distinct banks.  The permuted summation order makes its value
//                        a SELECTION key only; each wave re-evaluates its few surviving
//                        candidates exactly (ascending j) at the end of the query and dumps its
//                        list; scan_merge_refine_kernel (one wave per query) merges the lists.
//                        Results are bit-identical to scan_ref_kernel.
#include <atomic>
#include <chrono>

#include "scan_cells.h"
#include "scan_device.h"
#include "scan_order.h"
#include "scan_ref.h"

namespace tpq {

// part1[q][j][c] = 2 * (q_j . r_jc), dots as ascending-dimension fma chains
// (IVFPQIndex.precomputed_adc_residual_precomputed, index/IVFPQIndex.py:366-379)
__global__ __launch_bounds__(256) void residual_part1_kernel(const float* __restrict__ query,
                                                            const float* __restrict__ codebook,
                                                            float* __restrict__ part1, int m,
                                                            int ds, int nq) {
  const int j = blockIdx.y, q = blockIdx.x, c = threadIdx.x;
  float dot = 0.f;
  for (int e = 0; e < ds; ++e)
    dot = fmaf(query[(int64_t)(j * ds + e) * nq + q], codebook[((int64_t)j * ds + e) * 256 + c], dot);
  part1[((int64_t)q * m + j) * 256 + c] = 2.f * dot;
}


// LDS of the reference-layout kernels: the m KiB table in region0, the staged query behind the frame
static size_t ref_lds_bytes(int m, int R, int max_nprobe, int fused_floats) {
  return list_scan_lds_bytes(list_region0((size_t)m * 1024, R), max_nprobe, (size_t)fused_floats * 4);
}

static int dispatch_ref(const ScanArgs& a, int R, hipStream_t st) {
  return with_list_regs(R, [&](auto r_c) {
    constexpr int RC = decltype(r_c)::value;
    return launch_list_scan(scan_ref_kernel<RC>, scan_merge_kernel<RC>, "scan_ref_kernel", a,
                            ref_lds_bytes(a.m, RC, a.max_nprobe, fused_floats_of(a)), st);
  });
}

static int run_residual_ref(ScanArgs a, ResidualArgs ra, hipStream_t st) {
  const int R = list_regs(a.k);
  const bool build_part1 = !ra.full && !ra.part1;
  const size_t lds = ref_lds_bytes(a.m, R, a.max_nprobe, build_part1 ? a.m * a.ds + a.m : 0);
  auto go = [&](auto kernel) -> int {
    int rc2 = set_lds(kernel, lds, "scan_residual_kernel");
    if (rc2) return rc2;
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.nq), dim3(kScanThreads), lds, st, a, ra);
    TPQ_LAUNCH_CHECK("scan_residual_kernel");
    return TPQ_OK;
  };
  return with_list_regs(R, [&](auto r_c) { return go(scan_residual_kernel<decltype(r_c)::value>); });
}

static int run_ref(ScanArgs a, void* workspace, size_t workspace_bytes, hipStream_t st) {
  int rc = validate(a);
  if (rc || a.nq == 0) return rc;
  const int R = list_regs(a.k);
  if (a.n_split > 1) {
    rc = need_ws(workspace, workspace_bytes, ws_bytes_for(a.nq, R, a.n_split), "ivfpq_scan");
    if (rc) return rc;
    fill_ws(a, workspace, R, a.n_split);
  }
  return dispatch_ref(a, R, st);
}

// exact redo of the (normally zero) queries a packed route flagged: the reference-layout kernels, one workgroup per query
static int redo_flagged(const ScanArgs& a, const ResidualArgs* ra, hipStream_t st) {
  ScanArgs b = a;
  b.n_split = 1;
  b.only_flagged = a.flags;
  return ra ? run_residual_ref(b, *ra, st) : dispatch_ref(b, list_regs(a.k), st);
}

// the per-M translation units (scan_packed.hip)
struct PackedUnit {
  int m;
  int (*packed)(const ScanArgs& a, const ResidualArgs* ra, int RL, int R, hipStream_t st);
  int (*pool)(const ScanArgs& a, int RL, hipStream_t st);
  int (*dump)(const ScanArgs& a, int RL, int Rf, int mode, hipStream_t st);
  int (*dump_occupancy)(int mode);
  int (*finish)(const ScanArgs& a, int chunks, int Rf, int seed_chunks, const int* cnt, hipStream_t st);
};
static const PackedUnit* packed_unit(int m) {
#define TPQ_UNIT(M) \
  {M, dispatch_packed_##M, dispatch_pool_##M, dispatch_dump_##M, dump_occupancy_##M, dispatch_finish_##M},
  static const PackedUnit units[] = {TPQ_PACKED_M_LIST(TPQ_UNIT)};
#undef TPQ_UNIT
  for (const PackedUnit& u : units)
    if (u.m == m) return &u;
  return nullptr;
}

}  // namespace tpq

using namespace tpq;

extern "C" size_t tpq_ivfpq_scan_workspace_bytes(int nq, int k, int n_split, int m) {
  if (nq <= 0 || k <= 0) return 0;
  if (n_split < 1) n_split = 1;
  int R = list_regs_packed(k) > list_regs(k) ? list_regs_packed(k) : list_regs(k);
  if (R > 16) R = 16;
  // covers both kernels -- and, on the dump routes, the split tail: 4 parts x 4 waves of lists per query
  size_t lists = ws_bytes_for(nq, R, n_split * packed_waves(m));
  if ((dump_built(m, kDumpSel16) || dump_built(m, kDumpF32)) && dump_finish_regs(k, 1) <= kDumpMaxR) {
    const int rp = list_regs_packed(k);
    const size_t tail = ws_bytes_for(nq, rp < 2 ? rp : 2, 16), whole = ws_bytes_for(nq, rp < 4 ? rp : 4, 4);
    lists = tail > lists ? tail : lists;
    lists = whole > lists ? whole : lists;
  }
  const size_t pools = list_regs_packed(k) >= pool_min_list_regs(m) ? pool_ws_bytes(nq, k, m, n_split * packed_waves(m)) : 0;  // pool mode
  return lists > pools ? lists : pools;
}

#ifdef TPQ_SCAN_PROFILE
// private instrumentation build: phase timestamps of scan_packed_kernel (tools/scan_phase_profile.py)
static unsigned long long* g_scan_prof = nullptr;
extern "C" void tpq_debug_set_scan_profile(void* buf) { g_scan_prof = (unsigned long long*)buf; }
#endif
// ---- tickets of the fused finish ---------------------------------------------------------------------
// A query split over several workgroups is finished by the last one to arrive: one int32 ticket per query,
// ZERO when the kernel starts and zero again when it ends (the finisher resets it).  The tickets belong to the
// CALLER (tpq_ivfpq_scan_tickets_bytes; zeroed once, then reusable by every later call that is ordered after
// this one): the workspace arrives uninitialised and zeroing it would be a launch of its own, and a buffer
// owned by the library would be state the boundary does not allow.  No tickets: a split query takes the
// three-launch path (scan, merge, flagged redo).
static bool fuse_enabled() {
  static const bool v = [] {
    const char* e = TPQ_AB_ENV("TPQ_SCAN_FUSE");  // (variant builds, A/B: TPQ_SCAN_FUSE=0 runs the three-launch path)
    return !(e && atoi(e) == 0);
  }();
  return v;
}
// the value that marks a raised flag in this call: non-zero, different from call to call (the flags live in
// the caller's uninitialised workspace, which may be the memory an earlier call used) -- from the clock, so
// that the library keeps no counter
// INVARIANT (captured graphs replay with the SAME epoch and the same workspace): every path that raises flags also
// consumes them before the call's last kernel ends -- the fused finisher and scan_ref_kernel / scan_residual_kernel
// reset a flag they act on; scan_pool_merge_kernel and scan_finish_exact_kernel only skip (or raise) and rely on the
// redo_flagged launch that follows them IN THE SAME CALL.  A call that returns an error between those two launches
// leaves flags raised: harmless for the next call (another epoch), and a capture that saw a failed launch is dead
// anyway.  A stale word that happens to equal the epoch costs one needless exact redo, never a wrong result.
static int fresh_epoch() {
  const uint64_t ns = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
  return (int)(((uint32_t)(ns ^ (ns >> 29)) * 0x9e3779b1u) | 1u);
}

// large batches of plain PQ at m = 64, k <= 504: dump mode over the 16-bit table (scan_packed_kernel.h, scan_finish.h).
// (variants: TPQ_SCAN_DUMP=0 keeps the one-launch finish / the lists)
// returns 0 (not this route), kDumpSel16 (four-wave workgroups) or kDumpSel16W8 (eight-wave workgroups: k in (248, 504]
// where four waves would need longer lists than eight -- long cells; lists of <= 2 registers, 16 chunks per query)
static int dump_min_queries() {  // (variants: TPQ_SCAN_DUMP_MINQ=n takes batches from n queries on, whatever n_split says)
  const char* e = TPQ_AB_ENV("TPQ_SCAN_DUMP_MINQ");
  return e ? atoi(e) : kDumpMinQueries;
}
static int dump_route(const ScanArgs& a, bool residual, int R) {
  if (residual || R > kDumpMaxR) return 0;
  // (the route deals the queries itself -- dump_tail --: a caller's n_split > 1 belongs to batches below its threshold)
  if (a.n_split != 1 && dump_min_queries() == kDumpMinQueries) return 0;
  if (a.nq < dump_min_queries()) return 0;
  const char* e = TPQ_AB_ENV("TPQ_SCAN_DUMP");
  if (e && atoi(e) == 0) return 0;
  // (the finish kernel takes a query's lists as at most 16 chunks of 64 keys: four waves x RL <= 4, eight x RL <= 2)
  const int rl4 = list_regs_scan(a.k, a.m, a.max_nprobe, a.slots_hint, 4);
  if (dump_built(a.m, kDumpF32)) {
    // Short codes (round 6): the fp32 table their four-wave workgroups stream over anyway; the finish kernel takes the
    // exact entries from the codebook in LDS (fused calls, m * ds <= 128) or from the caller's table.  k <= 248: the
    // pools keep the larger k (TPQ_SCAN_DUMP_SHORT_K=n in variant builds moves the limit for A/B).
    const char* ek = TPQ_AB_ENV("TPQ_SCAN_DUMP_SHORT_K");
    const int kmax = ek ? atoi(ek) : kDumpShortMaxK;
    if (a.k > kmax || rl4 > 4) return 0;
    if (!a.lut && a.m * a.ds > 128) return 0;
    // a caller's table: the finish kernel gathers m entries per survivor from it -- pays only behind long scans (the
    // reference grid at m = 16, IVF4096 cells of 244 slots, scan fraction of 8 TB/s, one-launch finish / this route:
    // 32 probes 0.44 / 0.39, 64 probes 0.49 / 0.50, 128 probes 0.58 / 0.63)
    if (a.lut && a.slots_hint < kDumpLutMinSlots) return 0;
    return kDumpF32;
  }
  // m = 64: the 16-bit table.  The finish kernel recomputes the survivors' table entries from the codebook, held in
  // LDS next to nothing else: fused calls (query + codebook) only, m * ds <= 128
  if (a.lut || !dump_built(a.m, kDumpSel16) || a.ds > 2) return 0;
  const int rl8 = list_regs_scan(a.k, a.m, a.max_nprobe, a.slots_hint);
  // Lists of 4 registers in four-wave workgroups only where eight waves would need them as well (short cells, k > 256):
  // folding into a 256-entry list is what a large k costs, and four waves see twice the candidates each.
  // Same box, 10 000 queries, ms, four waves / the sorted lists of the three-launch path: k = 300, 244-slot cells x
  // 16 / 32 / 64 probes: 1.48 / 1.98 / 2.92 against 2.23 / 2.83 / 3.91 (k = 500: 1.74 / 2.51 / 3.61 against 2.63 / 3.33
  // / 4.47) -- both at 4 registers; 977-slot cells x 8 / 32 probes, k = 300: 1.91 / 4.37 against 1.69 / 3.45 -- 4
  // registers against 2: those take the eight-wave form.
  if (rl4 <= 2 || (rl4 <= 4 && rl4 <= rl8)) return kDumpSel16;
  if (e && atoi(e) == 1) return 0;  // (variants: TPQ_SCAN_DUMP=1 = four waves or the lists)
  if (a.k > 248 && rl8 <= 2) return kDumpSel16W8;
  return 0;
}

// Per-device caches of device properties (relaxed atomics: concurrent first calls from several host threads write the
// same value); `query` runs on the current device, `fallback` stands in when it fails.
template <int N, class Query>
static int device_cached(std::atomic<int> (&cache)[64][N], int i, int fallback, Query query) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fallback;
  int n = cache[dev][i].load(std::memory_order_relaxed);
  if (n <= 0) {
    n = query(dev);
    if (n <= 0) n = fallback;
    cache[dev][i].store(n, std::memory_order_relaxed);
  }
  return n;
}
static int device_cus() {
  static std::atomic<int> cus[64][1] = {};
  return device_cached(cus, 0, 256, [](int dev) {
    int n = 0;
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess ? n : 0;
  });
}
// workgroup slots of the dump-mode scan kernel on this device: CUs x the workgroups of it a CU holds -- from the occupancy
// query of the kernel's smallest instantiation (the "4 per CU" used to be an assumption)
static int dump_slots(const PackedUnit& u, int mode) {
  static std::atomic<int> per_cu[64][3 * 4] = {};  // [device][mode x m class]
  const int mi = mode == kDumpSel16 ? 0 : (mode == kDumpF32 ? 1 : 2), ci = u.m == 64 ? 0 : (u.m == 32 ? 1 : (u.m == 16 ? 2 : 3));
  return device_cached(per_cu, mi * 4 + ci, 4, [&](int) { return u.dump_occupancy(mode); }) * device_cus();
}
// The batch's last round of workgroups (ScanArgs::unsplit): the chip holds 4 dump-mode workgroups per CU; the
// nq mod slots queries left after the full rounds are dealt in 4 (or 2) parts each when those parts fit one round and
// the finish kernel can take their lists (<= 16 chunks of 64 keys per query) -- 1 250 queries: 1 024 whole + 226 x 4.
static void dump_tail(int nq, int nw, int RL, int slots, int* unsplit, int* parts) {
  *unsplit = nq;
  *parts = 1;
  if (slots <= 0) return;
  const int whole = (nq / slots) * slots, rest = nq - whole;
  if (rest == 0) return;
  for (int c = 4; c >= 2; c >>= 1) {
    if ((int64_t)rest * c <= slots && c * nw * RL <= 16) {
      *unsplit = whole;
      *parts = c;
      return;
    }
  }
}

// What a packed call runs, decided once per call by plan_scan -- a pure host function (no HIP call: the route query,
// tpq_ivfpq_scan_route, answers without a GPU) -- and executed by run_packed without re-deriving any of it.  How a dump
// route deals its workgroups -- the split tail and the dispatch order -- needs the device's workgroup slots and the size
// of the caller's buffer: plan_dump_dispatch adds it to the plan from those two numbers (pure as well: the executor asks
// the device, tpq_ivfpq_scan_ordered takes them as arguments).  It changes the parts a query is dealt in and the order
// the queries start in, never the route.
struct ScanPlan {
  int route = -1;            // TPQ_SCAN_ROUTE_*, -1 = the entry point rejects the call
  int R = 0;                 // registers of the merged list (list_regs_packed(k))
  int RL = 0;                // registers of the per-wave lists (pools: of the threshold lists)
  int Rf = 0;                // dump routes: registers of the finish kernel's exact list
  int mode = 0;              // dump routes: kDumpF32 / kDumpSel16 / kDumpSel16W8
  int waves = 0;             // waves per scan workgroup
  int n_split = 1;           // workgroups per query (the dump routes: 1 before the split tail)
  bool fuse = false;         // one-launch finish
  bool small_lists = false;  // per-wave lists shorter than k + kBandSlack
  // dump routes, by plan_dump_dispatch:
  int unsplit = 0;           // ScanArgs::unsplit (0: every query is dealt in `parts`)
  int parts = 1;             // workgroups per query of the split tail
  bool ordered = false;      // queries dispatched longest first (scan_order.hip)
};

static ScanPlan plan_scan(const ScanArgs& a, bool residual) {
  const int m = a.m, k = a.k;
  ScanPlan p;
  p.n_split = a.n_split;
  if (!packed_unit(m)) {
    // no scan-layout kernel at this m: the fused entry point scans the reference layout, the others reject the call
    if (!residual && !a.lut) p.route = TPQ_SCAN_ROUTE_REF;
    return p;
  }
  p.R = list_regs_packed(k);
  p.waves = packed_waves(m);
  const bool lds_fits =
      scan_lds_bytes_packed(m, p.R > 16 ? 16 : p.R, a.max_nprobe, fused_floats_of(a), residual) <= 160 * 1024;
  // k within kBandSlack of 1024 (no room for the candidate band), or a probe table that no longer
  // fits next to the LUT: scan exactly with the reference-layout kernel
  if (p.R > 16 || !lds_fits) {
    p.route = TPQ_SCAN_ROUTE_REF;
    if (residual) p.n_split = 1;
    return p;
  }
  // (measured against the sorted lists of the three-launch path, C2 shape, 10 000 queries: m = 64, k = 600 / 1000:
  // 6.1 / 6.9 ms against 7.1 / 8.3; m = 120 (1 000 queries), k = 1000: 2.0 against 3.4 -- and k = 600: 1.9 against 1.6;
  // m = 16, 32: within 2 %; k = 300, 500 at m = 64: 4.1 / 4.5 against 3.6 / 4.0)
  const bool pools = !residual && p.R >= pool_min_list_regs(m) && (p.waves < 16 || k > 768) && fuse_enabled();
  // large batches: dump_route.  (Where the pools apply as well -- k in (248, 504] of the short codes -- the pools keep the
  // call: dump_route's own k limit for m <= 32, kDumpShortMaxK, says so; variant builds move it for the A/B.)  A pair of
  // list registers without an instantiation (TPQ_DUMP_PAIRS) declines the route: ADVICE r5, a change of the list-size
  // heuristics must not fail a search.
  const int Rf = dump_finish_regs(k, a.slots_hint), mode = dump_route(a, residual, Rf);
  if (mode && !(is_sel16(mode) && pools)) {
    const int nw = scan_waves(m, mode), RL = list_regs_scan(k, m, a.max_nprobe, a.slots_hint, nw);
    if (dump_pair_built(mode, RL, Rf)) {
      p.route = mode == kDumpF32 ? TPQ_SCAN_ROUTE_DUMP_F32
                                 : (mode == kDumpSel16 ? TPQ_SCAN_ROUTE_DUMP_SEL16 : TPQ_SCAN_ROUTE_DUMP_SEL16_W8);
      p.mode = mode, p.waves = nw, p.RL = RL, p.Rf = Rf, p.n_split = 1;
      return p;
    }
  }
  // the largest k, plain PQ: pool mode (scan_packed_kernel.h) -- threshold lists of ceil(k / waves) entries, unsorted pools,
  // one ranking kernel per query; flagged queries (a pool or the ranking buffer overflowed) redone exactly
  // (the ranking kernel takes a query's lists into LDS: fewer workgroups per query when they would not fit)
  if (pools) {
    p.route = TPQ_SCAN_ROUTE_POOLS;
    p.RL = pool_list_regs(k, m);
    if (p.n_split > pool_max_split(m, k)) p.n_split = pool_max_split(m, k);
    return p;
  }
  p.RL = list_regs_scan(k, m, a.max_nprobe, a.slots_hint);
  p.small_lists = p.RL < p.R;
  // the scan workgroups finish the query themselves (merge, write, exact redo): one launch instead of three.
  // (k <= 248, plain PQ; a query split over several workgroups needs the caller's tickets)
  p.fuse = !residual && fuse_enabled() && fuse_fits(m, p.R) && p.waves * p.RL >= p.R && (a.n_split == 1 || a.tickets);
  p.route = p.fuse ? TPQ_SCAN_ROUTE_ONE_LAUNCH : TPQ_SCAN_ROUTE_LISTS;
  return p;
}

// The dump routes' dispatch, from the device's workgroup slots and the caller's workspace:
//  * the split tail (dump_tail; a workspace sized by an older rule keeps the tail whole);
//  * the order: on exactly when the batch needs more than one round of workgroup slots -- below that there is no ragged
//    end to shorten and the call costs what it did -- and is within the ranking's limit (kOrderMaxQueries), and the
//    workspace has room for the order behind the lists in use (tpq_ivfpq_scan_workspace_bytes covers 16 lists of two
//    registers per query, a call uses parts x waves x RL of them: the size the caller is told does not change; a
//    workspace without the room keeps index order).
static void plan_dump_dispatch(ScanPlan& p, int nq, int slots, size_t workspace_bytes) {
  int unsplit = nq, parts = 1;
  if (p.mode != kDumpSel16W8) dump_tail(nq, p.waves, p.RL, slots, &unsplit, &parts);
  if (parts > 1 && workspace_bytes < ws_bytes_for(nq, p.RL, parts * p.waves)) unsplit = nq, parts = 1;
  p.parts = parts;
  p.unsplit = parts > 1 ? unsplit : 0;  // (0 with one part per query: "all queries split 1 way")
  p.ordered = slots > 0 && nq > slots && nq <= kOrderMaxQueries &&
              workspace_bytes >= ws_bytes_for(nq, p.RL, parts * p.waves) + order_ws_bytes(nq);
}
static bool is_dump_route(int route) {
  return route == TPQ_SCAN_ROUTE_DUMP_F32 || route == TPQ_SCAN_ROUTE_DUMP_SEL16 || route == TPQ_SCAN_ROUTE_DUMP_SEL16_W8;
}

// the arguments a route query stands for (pointers are only tested against nullptr)
static ScanArgs route_query_args(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint,
                                 int has_lut, int has_tickets) {
  ScanArgs a{};
  static const float dummy_lut = 0.f;
  static int32_t dummy_tickets = 0;
  a.lut = has_lut ? &dummy_lut : nullptr;
  a.ds = has_lut ? 0 : ds;
  a.nq = nq; a.k = k; a.n_split = n_split; a.m = m; a.max_nprobe = max_nprobe;
  a.slots_hint = slots_hint;
  a.tickets = has_tickets ? &dummy_tickets : nullptr;
  return a;
}

extern "C" int tpq_ivfpq_scan_route(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint,
                                    int has_lut, int has_packed, int has_tickets, int residual) {
  if (nq <= 0 || k < 1 || k > 1024 || m < 4 || m % 4 != 0 || n_split < 1 || max_nprobe < 1) return -1;
  if (!has_packed) return TPQ_SCAN_ROUTE_REF;
  return plan_scan(route_query_args(nq, k, n_split, m, ds, max_nprobe, slots_hint, has_lut, has_tickets), residual != 0)
      .route;
}

extern "C" int tpq_ivfpq_scan_ordered(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint,
                                      int has_lut, int has_packed, int has_tickets, int residual, int slots,
                                      size_t workspace_bytes) {
  if (nq <= 0 || k < 1 || k > 1024 || m < 4 || m % 4 != 0 || n_split < 1 || max_nprobe < 1) return -1;
  if (!has_packed) return 0;
  ScanPlan p =
      plan_scan(route_query_args(nq, k, n_split, m, ds, max_nprobe, slots_hint, has_lut, has_tickets), residual != 0);
  if (!is_dump_route(p.route)) return 0;
  plan_dump_dispatch(p, nq, slots > 0 ? slots : dump_slots(*packed_unit(m), p.mode), workspace_bytes);
  return p.ordered ? 1 : 0;
}

// ---- the cell-major form of the m = 64 large-batch route (scan_cells.hip) ---------------------------
// The route stays TPQ_SCAN_ROUTE_DUMP_SEL16; the form is what a call that hands over its probed cells runs when
//  * the plan is the four-wave route (fused table, ds <= 2, >= 1 024 queries), k <= 128, more than kCellP0 probes;
//  * the batch is cell-dense: the mean code byte is read nq x slots_hint / n_slots >= kCellMinRereads times;
//  * the query's lists as 16 (or 8) chunks of 64 keys -- the finish kernel's forms -- and the inversion arrays fit the
//    workspace: behind the lists in use, as the order does; tpq_ivfpq_scan_workspace_bytes stays what it is.
// With room for one more array behind those -- an fp32 per slot (cell_norm_bytes) -- the slot norms are computed once
// per call (cell_norm_kernel) instead of in every candidate block: cell_major_norms, tpq_ivfpq_scan_cell_norms.
// Pure host arithmetic: tpq_ivfpq_scan_cell_major answers without a GPU.  Returns the chunks per query, 0 = today's path.
// The A/B switch of the threshold form's selection key (index.use_cell_single_product): process-wide, read once per call
// on the host; 1 (the default): one fp16 product per k-step and the per-query band of `The single-product key`
// (scan_cells.hip) where that kernel is built (ds = 2); 0: three products.  Same results either way -- every returned
// value is the finish kernel's --; the single product admits more candidates where many rows lie within 2 delta_q of the
// k-th best, and a query whose lists overflow is redone exactly: that is the data the switch is for.
// g_cell_products: the products per k-step the last packed scan call's candidate kernels ran, 0 when it did not take
// the cell-major form.
static std::atomic<int> g_cell_single_product{1};
static std::atomic<int> g_cell_products{0};
extern "C" int tpq_ivfpq_scan_use_cell_single_product(int on) { return g_cell_single_product.exchange(on ? 1 : 0); }
extern "C" int tpq_ivfpq_scan_last_cell_products(void) { return g_cell_products.load(); }

struct CellMajor {
  const int64_t* cells;  // [nq][max_nprobe]
  int n_cells;
  // the caller's kept state (scan_cells.hip: `The kept state`; nullptr: none) and whether it is valid for these codes,
  // codebook and tombstones; a call that takes the form with slot norms builds it first when it is not
  void* kept = nullptr;
  size_t kept_bytes = 0;
  int kept_valid = 0;
};
// a state too small for the index is not used (and not written)
static void cell_major_use_kept(CellArgs& c, const CellMajor& cm) {
  if (cm.kept && c.norm && cm.kept_bytes >= cell_kept_bytes(c.n_slots, c.ds)) cell_use_kept(c, cm.kept, cm.kept_valid);
}
static int cell_major_chunks(const ScanArgs& a, const ScanPlan& p, bool residual, int n_cells, size_t workspace_bytes) {
  if (residual || p.route != TPQ_SCAN_ROUTE_DUMP_SEL16 || a.lut || a.m != 64 || a.ds < 1 || a.ds > 2) return 0;
  if (a.k > 128 || a.max_nprobe <= kCellP0 || n_cells < 1 || a.n_slots <= 0 || a.slots_hint <= 0) return 0;
  if ((int64_t)a.nq * a.slots_hint < (int64_t)kCellMinRereads * a.n_slots) return 0;
  if ((int64_t)a.nq * a.max_nprobe >= 0x7fffffffLL) return 0;
  const size_t extra = cell_extra_bytes(a.nq, a.max_nprobe, n_cells, kCellP0);
  for (int chunks = 16; chunks >= 8; chunks >>= 1)
    if ((a.k + 63) / 64 < chunks && workspace_bytes >= ws_bytes_for(a.nq, 1, chunks) + extra) return chunks;
  return 0;
}
static bool cell_major_norms(const ScanArgs& a, int chunks, int n_cells, size_t workspace_bytes) {
  return chunks > 0 && workspace_bytes >= ws_bytes_for(a.nq, 1, chunks) +
                                              cell_extra_bytes(a.nq, a.max_nprobe, n_cells, kCellP0) +
                                              cell_norm_bytes(a.n_slots);
}

// stages 1-5 (the flag-gated redo over ALL probes is the caller's next line, as on every dump route)
static int run_cell_major(ScanArgs& a, ScanPlan p, const PackedUnit& u, const CellMajor& cm, int chunks, void* workspace,
                          size_t workspace_bytes, hipStream_t st) {
  const int nq = a.nq;
  // 1. the threshold pass: today's route -- order, split tail, scan, finish -- over each query's first kCellP0 probes;
  //    it leaves the exact top-k of those cells in out_vals / out_addr
  ScanArgs t = a;
  t.probe_cap = kCellP0;
  plan_dump_dispatch(p, nq, dump_slots(u, p.mode), workspace_bytes);
  t.n_split = p.parts;
  t.unsplit = p.unsplit;
  const size_t lists_bytes = ws_bytes_for(nq, p.RL, p.parts * p.waves);
  int rc = need_ws(workspace, workspace_bytes, lists_bytes, "ivfpq_scan_packed");
  if (rc) return rc;
  fill_ws(t, workspace, p.RL, p.parts * p.waves);
  if (p.ordered) {
    int* o = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + lists_bytes);
    const size_t stride = order_ws_bytes(nq) / 3 / sizeof(int);
    rc = launch_scan_order(a.cell_start, a.cell_size, a.n_probe_list, nq, a.max_nprobe, packed_tile_shift(a.m), o,
                           o + stride, o + 2 * stride, st, kCellP0);
    if (rc) return rc;
    t.order = o;
    t.rank = o + stride;
  }
  rc = u.dump(t, p.RL, p.Rf, p.mode, st);
  if (rc) return rc;
  // 2-4. seeds, inversion, candidates: the query's lists are `chunks` lists of one chunk each from here on
  a.n_split = 1;
  a.unsplit = 0;
  fill_ws(a, workspace, 1, chunks);
  CellArgs c{};
  c.codes = a.codes; c.query = a.query; c.codebook = a.codebook; c.is_empty = a.is_empty;
  c.cell_start = a.cell_start; c.cell_size = a.cell_size; c.n_probe_list = a.n_probe_list; c.cells = cm.cells;
  c.n_slots = a.n_slots; c.nq = nq; c.max_nprobe = a.max_nprobe; c.n_cells = cm.n_cells; c.ds = a.ds;
  c.euclid = a.euclid; c.p0 = kCellP0; c.p_hi = a.max_nprobe; c.k = a.k; c.chunks = chunks; c.epoch = a.epoch;
  c.rel = cell_delta_rel(a.ds);
  c.products = 3;
  g_cell_products.store(3);
  c.seed_vals = a.out_vals; c.seed_addr = a.out_addr;
  c.keys = reinterpret_cast<unsigned*>(a.ws_vals); c.idx = reinterpret_cast<unsigned*>(a.ws_idx);
  c.list_evict = a.list_evict; c.flags = a.flags; c.ws_delta = a.ws_delta;
  const size_t cm_lists = ws_bytes_for(nq, 1, chunks);  // (the gate saw to it: lists and extras fit)
  cell_fill_extras(c, reinterpret_cast<char*>(workspace) + cm_lists, workspace_bytes - cm_lists);
  cell_major_use_kept(c, cm);  // (with room for per-call norms only: tpq_ivfpq_scan_cell_norms is the rule for both)
  rc = launch_cell_candidates(c, st);
  if (rc) return rc;
  // 5. the finish kernel over the chunks that were filled (the seed chunks and ceil(cnt[q] / 64) behind them): F_k, the
  //    cut at F_k - 2 delta_q, the survivors among the candidates evaluated exactly; those among the seeds keep the
  //    values stage 1 gave them (scan_finish.h)
  return u.finish(a, chunks, p.Rf, (a.k + 63) / 64, c.cnt, st);
}

// The threshold form of the cell-major form (scan_cells.hip: `The threshold from group maxima`): no query-major pass and
// no seeds -- the threshold comes from the candidate kernel's own accumulators over each query's first kCellThrProbes
// probes.  Taken when
//  * the cell-major form and its per-call slot norms are taken (pass A reads the norm array);
//  * the form's arrays (cell_thr_bytes) fit behind the lists, the extras and the norms;
//  * there are more than kCellThrProbes probes;
//  * the mean probed cell is long: slots_hint / max_nprobe >= kCellThrMinCell;
//  * the maxima expected of the first kCellThrProbes cells outnumber k twice -- fewer than k maxima give no threshold at
//    all (-inf admits everything), and a threshold from just over k of them is loose.
// Pure host arithmetic: tpq_ivfpq_scan_cell_threshold answers without a GPU.
static bool cell_threshold_form(const ScanArgs& a, int chunks, int n_cells, size_t workspace_bytes) {
  if (!cell_major_norms(a, chunks, n_cells, workspace_bytes) || a.max_nprobe <= kCellThrProbes) return false;
  const size_t need = ws_bytes_for(a.nq, 1, chunks) + cell_extra_bytes(a.nq, a.max_nprobe, n_cells, kCellP0) +
                      cell_norm_bytes(a.n_slots) + cell_thr_bytes(a.nq, a.max_nprobe, n_cells);
  const int64_t mean_cell = a.slots_hint / a.max_nprobe;
  return workspace_bytes >= need && mean_cell >= kCellThrMinCell &&
         (int64_t)kCellThrProbes * mean_cell / kCellThrGroup >= 2 * (int64_t)a.k;
}

// the threshold form's stages (the flag-gated redo over ALL probes is the caller's next line)
static int run_cell_threshold(ScanArgs& a, const ScanPlan& p, const PackedUnit& u, const CellMajor& cm, int chunks,
                              void* workspace, hipStream_t st) {
  const int nq = a.nq;
  a.n_split = 1;
  a.unsplit = 0;
  fill_ws(a, workspace, 1, chunks);
  CellArgs c{};
  c.codes = a.codes; c.query = a.query; c.codebook = a.codebook; c.is_empty = a.is_empty;
  c.cell_start = a.cell_start; c.cell_size = a.cell_size; c.n_probe_list = a.n_probe_list; c.cells = cm.cells;
  c.n_slots = a.n_slots; c.nq = nq; c.max_nprobe = a.max_nprobe; c.n_cells = cm.n_cells; c.ds = a.ds;
  c.euclid = a.euclid; c.p0 = 0; c.p_hi = a.max_nprobe; c.k = 0; c.thr_k = a.k; c.chunks = chunks; c.epoch = a.epoch;
  // the selection key's arithmetic (scan_cells.hip: `The single-product key`): both passes on it, and its own band
  c.products = g_cell_single_product.load() && cell_single_product_built(a.ds) ? 1 : 3;
  c.rel = c.products == 1 ? cell_delta1_rel(a.ds) : cell_delta_rel(a.ds);
  g_cell_products.store(c.products);
  c.keys = reinterpret_cast<unsigned*>(a.ws_vals); c.idx = reinterpret_cast<unsigned*>(a.ws_idx);
  c.list_evict = a.list_evict; c.flags = a.flags; c.ws_delta = a.ws_delta;
  // the extras where the seeded form has them (its pairs array, max_nprobe - kCellP0 per query, stays unused: pass B's
  // pairs are the form's own), the norms behind them, the form's arrays behind the norms (the gate: all of it fits)
  char* at = reinterpret_cast<char*>(workspace) + ws_bytes_for(nq, 1, chunks);
  const size_t head = cell_extra_bytes(nq, a.max_nprobe, cm.n_cells, kCellP0) + cell_norm_bytes(a.n_slots);
  cell_fill_extras(c, at, head, kCellP0);
  cell_major_use_kept(c, cm);
  CellThrArrays t{};
  cell_fill_thr(t, at + head, nq, a.max_nprobe, cm.n_cells);
  int rc = launch_cell_threshold(c, t, st);
  if (rc) return rc;
  // stage 5 without seed chunks: every survivor of the cut is evaluated by the finish kernel's ascending-j chain; the
  // exact list sized for the band of the key the candidates were selected on
  const int Rf1 = c.products == 1 ? cell_single_finish_regs(a.k) : 0;
  return u.finish(a, chunks, Rf1 > p.Rf ? Rf1 : p.Rf, 0, c.cnt, st);
}

extern "C" int tpq_ivfpq_scan_cell_major(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint,
                                         int has_lut, int has_packed, int has_tickets, int residual, int n_cells,
                                         int64_t n_slots, size_t workspace_bytes) {
  if (nq <= 0 || k < 1 || k > 1024 || m < 4 || m % 4 != 0 || n_split < 1 || max_nprobe < 1) return -1;
  if (!has_packed) return 0;
  ScanArgs a = route_query_args(nq, k, n_split, m, ds, max_nprobe, slots_hint, has_lut, has_tickets);
  a.n_slots = n_slots;
  const ScanPlan p = plan_scan(a, residual != 0);
  return cell_major_chunks(a, p, residual != 0, n_cells, workspace_bytes) ? 1 : 0;
}

extern "C" int tpq_ivfpq_scan_cell_norms(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint,
                                         int has_lut, int has_packed, int has_tickets, int residual, int n_cells,
                                         int64_t n_slots, size_t workspace_bytes) {
  if (nq <= 0 || k < 1 || k > 1024 || m < 4 || m % 4 != 0 || n_split < 1 || max_nprobe < 1) return -1;
  if (!has_packed) return 0;
  ScanArgs a = route_query_args(nq, k, n_split, m, ds, max_nprobe, slots_hint, has_lut, has_tickets);
  a.n_slots = n_slots;
  const ScanPlan p = plan_scan(a, residual != 0);
  const int chunks = cell_major_chunks(a, p, residual != 0, n_cells, workspace_bytes);
  return cell_major_norms(a, chunks, n_cells, workspace_bytes) ? 1 : 0;
}

extern "C" int tpq_ivfpq_scan_cell_threshold(int nq, int k, int n_split, int m, int ds, int max_nprobe,
                                             int64_t slots_hint, int has_lut, int has_packed, int has_tickets,
                                             int residual, int n_cells, int64_t n_slots, size_t workspace_bytes) {
  if (nq <= 0 || k < 1 || k > 1024 || m < 4 || m % 4 != 0 || n_split < 1 || max_nprobe < 1) return -1;
  if (!has_packed) return 0;
  ScanArgs a = route_query_args(nq, k, n_split, m, ds, max_nprobe, slots_hint, has_lut, has_tickets);
  a.n_slots = n_slots;
  const ScanPlan p = plan_scan(a, residual != 0);
  const int chunks = cell_major_chunks(a, p, residual != 0, n_cells, workspace_bytes);
  return cell_threshold_form(a, chunks, n_cells, workspace_bytes) ? 1 : 0;
}

// the A/B switch of the two forms (index.use_cell_threshold): process-wide, read once per call on the host; 0 keeps
// every later call to the seeded form.  Returns the previous setting.  tpq_ivfpq_scan_cell_threshold does not look at it.
static std::atomic<int> g_cell_threshold{1};
extern "C" int tpq_ivfpq_scan_use_cell_threshold(int on) { return g_cell_threshold.exchange(on ? 1 : 0); }
extern "C" int tpq_ivfpq_scan_cell_threshold_probes(void) { return kCellThrProbes; }

static int run_packed(ScanArgs a, const ResidualArgs* ra, void* workspace, size_t workspace_bytes,
                      tpq_stream_t stream, const CellMajor* cm = nullptr) {
  int rc = validate(a);
  if (rc) return rc;
  TPQ_REQUIRE(a.packed != nullptr, "ivfpq_scan_packed: null packed pointer");
  g_cell_products.store(0);
  if (a.nq == 0) return TPQ_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ScanPlan p = plan_scan(a, ra != nullptr);
  if (p.route == TPQ_SCAN_ROUTE_REF) {
    a.n_split = p.n_split;
    return ra ? run_residual_ref(a, *ra, st) : run_ref(a, workspace, workspace_bytes, st);
  }
  if (p.route < 0) {
    set_error("ivfpq_scan_packed: no scan-layout kernel instantiated for n_subvectors=%d; use "
              "tpq_ivfpq_scan_topk", a.m);
    return TPQ_ERR_UNSUPPORTED;
  }
  const PackedUnit& u = *packed_unit(a.m);
  const int nq = a.nq;
  a.n_split = p.n_split;
  a.small_lists = p.small_lists;
  a.fuse = p.fuse;
  if (!p.fuse) a.tickets = nullptr;
  // flags: raised == equal to this call's epoch; no zeroing pass (it was a launch of its own)
  a.epoch = fresh_epoch();
#ifdef TPQ_SCAN_PROFILE
  a.prof = g_scan_prof;
#endif
  switch (p.route) {
    case TPQ_SCAN_ROUTE_POOLS: {
      const int n_lists = p.n_split * p.waves;
      rc = need_ws(workspace, workspace_bytes, pool_ws_bytes(nq, a.k, a.m, n_lists), "ivfpq_scan_packed");
      if (rc) return rc;
      fill_ws_pool(a, workspace, n_lists);
      rc = u.pool(a, p.RL, st);
      break;
    }
    // large batches of plain PQ, k <= 504: dump mode (scan_packed_kernel.h) -- the scan workgroups stream over the selection
    // table (m = 64: 16-bit, 32 KiB, four workgroups per CU; m = 8, 16, 32: the fp32 table) and end with their lists of
    // fast values, one wave per query finishes
    case TPQ_SCAN_ROUTE_DUMP_F32:
    case TPQ_SCAN_ROUTE_DUMP_SEL16:
    case TPQ_SCAN_ROUTE_DUMP_SEL16_W8: {
      if (const int chunks = cm ? cell_major_chunks(a, p, ra != nullptr, cm->n_cells, workspace ? workspace_bytes : 0) : 0) {
        rc = g_cell_threshold.load() && cell_threshold_form(a, chunks, cm->n_cells, workspace_bytes)
                 ? run_cell_threshold(a, p, u, *cm, chunks, workspace, st)
                 : run_cell_major(a, p, u, *cm, chunks, workspace, workspace_bytes, st);
        break;
      }
      plan_dump_dispatch(p, nq, dump_slots(u, p.mode), workspace ? workspace_bytes : 0);
      a.n_split = p.parts;
      a.unsplit = p.unsplit;
      const size_t lists_bytes = ws_bytes_for(nq, p.RL, p.parts * p.waves);
      rc = need_ws(workspace, workspace_bytes, lists_bytes, "ivfpq_scan_packed");
      if (rc) return rc;
      fill_ws(a, workspace, p.RL, p.parts * p.waves);
      if (p.ordered) {  // order, rank and the work they are ranked by: behind the lists in use
        int* o = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + lists_bytes);
        const size_t stride = order_ws_bytes(nq) / 3 / sizeof(int);
        rc = launch_scan_order(a.cell_start, a.cell_size, a.n_probe_list, nq, a.max_nprobe, packed_tile_shift(a.m), o,
                               o + stride, o + 2 * stride, st, 0);
        if (rc) return rc;
        a.order = o;
        a.rank = o + stride;
      }
      rc = u.dump(a, p.RL, p.Rf, p.mode, st);
      break;
    }
    default: {  // TPQ_SCAN_ROUTE_ONE_LAUNCH, TPQ_SCAN_ROUTE_LISTS
      const int n_lists = p.n_split * p.waves;
      rc = need_ws(workspace, workspace_bytes, ws_bytes_for(nq, p.RL, n_lists), "ivfpq_scan_packed");
      if (rc) return rc;
      fill_ws(a, workspace, p.RL, n_lists);
      rc = u.packed(a, ra, p.RL, p.R, st);
      if (p.fuse) return rc;  // (the fused finish redoes them itself)
    }
  }
  if (rc) return rc;
  return redo_flagged(a, ra, st);
}

// ---- entry points (their ScanArgs: scan_args, scan_list.h) ---------------------------------------------
extern "C" size_t tpq_ivfpq_scan_tickets_bytes(int nq) { return nq > 0 ? (size_t)nq * sizeof(int32_t) : 0; }

extern "C" size_t tpq_ivfpq_cell_kept_bytes(int64_t n_slots, int ds) {
  return n_slots > 0 && (ds == 1 || ds == 2) ? cell_kept_bytes(n_slots, ds) : 0;
}

extern "C" int tpq_ivfpq_search_fused_cells_kept(const uint8_t* packed, const uint8_t* codes,
                                                 const float* query, const float* codebook, int ds,
                                                 int metric, const uint8_t* is_empty,
                                                 const int64_t* cell_start, const int64_t* cell_size,
                                                 const int64_t* n_probe_list, float* out_vals,
                                                 int64_t* out_addr, const int64_t* address2id,
                                                 int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                                                 int m, int k, int n_split, void* workspace,
                                                 size_t workspace_bytes, int32_t* tickets,
                                                 int64_t slots_hint, const int64_t* cells, int n_cells,
                                                 void* kept, size_t kept_bytes, int kept_valid,
                                                 tpq_stream_t stream) {
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER,
              "ivfpq_search_fused: bad metric %d", metric);
  TPQ_REQUIRE(ds >= 1 && ds <= 1024, "ivfpq_search_fused: bad sub-vector length %d", ds);
  ScanArgs a = scan_args(codes, packed, nullptr, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         address2id, out_ids, n_slots, nq, max_nprobe, m, k, n_split);
  a.query = query; a.codebook = codebook; a.ds = ds; a.euclid = metric == TPQ_METRIC_NEG_SQ_L2 ? 1 : 0;
  a.tickets = tickets; a.slots_hint = slots_hint;
  TPQ_REQUIRE((reinterpret_cast<uintptr_t>(kept) & 15) == 0, "ivfpq_search_fused: the kept state must be 16-byte aligned");
  const CellMajor cm{cells, n_cells, kept, kept_bytes, kept_valid};
  return packed ? run_packed(a, nullptr, workspace, workspace_bytes, stream, cells ? &cm : nullptr)
                : run_ref(a, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int tpq_ivfpq_search_fused_cells(const uint8_t* packed, const uint8_t* codes,
                                            const float* query, const float* codebook, int ds,
                                            int metric, const uint8_t* is_empty,
                                            const int64_t* cell_start, const int64_t* cell_size,
                                            const int64_t* n_probe_list, float* out_vals,
                                            int64_t* out_addr, const int64_t* address2id,
                                            int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                                            int m, int k, int n_split, void* workspace,
                                            size_t workspace_bytes, int32_t* tickets,
                                            int64_t slots_hint, const int64_t* cells, int n_cells,
                                            tpq_stream_t stream) {
  return tpq_ivfpq_search_fused_cells_kept(packed, codes, query, codebook, ds, metric, is_empty, cell_start, cell_size,
                                           n_probe_list, out_vals, out_addr, address2id, out_ids, n_slots, nq,
                                           max_nprobe, m, k, n_split, workspace, workspace_bytes, tickets, slots_hint,
                                           cells, n_cells, nullptr, 0, 0, stream);
}

extern "C" int tpq_ivfpq_search_fused_tickets(const uint8_t* packed, const uint8_t* codes,
                                              const float* query, const float* codebook, int ds,
                                              int metric, const uint8_t* is_empty,
                                              const int64_t* cell_start, const int64_t* cell_size,
                                              const int64_t* n_probe_list, float* out_vals,
                                              int64_t* out_addr, const int64_t* address2id,
                                              int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                                              int m, int k, int n_split, void* workspace,
                                              size_t workspace_bytes, int32_t* tickets,
                                              int64_t slots_hint, tpq_stream_t stream) {
  return tpq_ivfpq_search_fused_cells(packed, codes, query, codebook, ds, metric, is_empty, cell_start, cell_size,
                                      n_probe_list, out_vals, out_addr, address2id, out_ids, n_slots, nq, max_nprobe, m,
                                      k, n_split, workspace, workspace_bytes, tickets, slots_hint, nullptr, 0, stream);
}

extern "C" int tpq_ivfpq_search_fused(const uint8_t* packed, const uint8_t* codes,
                                      const float* query, const float* codebook, int ds,
                                      int metric, const uint8_t* is_empty,
                                      const int64_t* cell_start, const int64_t* cell_size,
                                      const int64_t* n_probe_list, float* out_vals,
                                      int64_t* out_addr, const int64_t* address2id,
                                      int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                                      int m, int k, int n_split, void* workspace,
                                      size_t workspace_bytes, tpq_stream_t stream) {
  return tpq_ivfpq_search_fused_tickets(packed, codes, query, codebook, ds, metric, is_empty, cell_start,
                                        cell_size, n_probe_list, out_vals, out_addr, address2id, out_ids,
                                        n_slots, nq, max_nprobe, m, k, n_split, workspace, workspace_bytes,
                                        nullptr, 0, stream);
}

extern "C" int tpq_ivfpq_scan_topk(const uint8_t* codes, const float* lut, const uint8_t* is_empty,
                                   const int64_t* cell_start, const int64_t* cell_size,
                                   const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                   const int64_t* address2id, int64_t* out_ids, int64_t n_slots,
                                   int nq, int max_nprobe, int m, int k, int n_split,
                                   void* workspace, size_t workspace_bytes, tpq_stream_t stream) {
  const ScanArgs a = scan_args(codes, nullptr, lut, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                               address2id, out_ids, n_slots, nq, max_nprobe, m, k, n_split);
  return run_ref(a, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int tpq_ivfpq_scan_topk_packed_tickets(const uint8_t* packed, const uint8_t* codes,
                                                  const float* lut, const uint8_t* is_empty,
                                                  const int64_t* cell_start, const int64_t* cell_size,
                                                  const int64_t* n_probe_list, float* out_vals,
                                                  int64_t* out_addr, const int64_t* address2id,
                                                  int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                                                  int m, int k, int n_split, void* workspace,
                                                  size_t workspace_bytes, int32_t* tickets,
                                                  int64_t slots_hint, tpq_stream_t stream) {
  ScanArgs a = scan_args(codes, packed, lut, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         address2id, out_ids, n_slots, nq, max_nprobe, m, k, n_split);
  a.tickets = tickets; a.slots_hint = slots_hint;
  return run_packed(a, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int tpq_ivfpq_scan_topk_packed(const uint8_t* packed, const uint8_t* codes,
                                          const float* lut, const uint8_t* is_empty,
                                          const int64_t* cell_start, const int64_t* cell_size,
                                          const int64_t* n_probe_list, float* out_vals,
                                          int64_t* out_addr, const int64_t* address2id,
                                          int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                                          int m, int k, int n_split, void* workspace,
                                          size_t workspace_bytes, tpq_stream_t stream) {
  return tpq_ivfpq_scan_topk_packed_tickets(packed, codes, lut, is_empty, cell_start, cell_size, n_probe_list,
                                            out_vals, out_addr, address2id, out_ids, n_slots, nq, max_nprobe, m,
                                            k, n_split, workspace, workspace_bytes, nullptr, 0, stream);
}

extern "C" int tpq_ivfpq_scan_topk_residual(const uint8_t* codes, const float* part1,
                                            const float* part2, const float* full_lut,
                                            const int64_t* cells, const float* base_sims,
                                            const uint8_t* is_empty, const int64_t* cell_start,
                                            const int64_t* cell_size, const int64_t* n_probe_list,
                                            float* out_vals, int64_t* out_addr,
                                            const int64_t* address2id, int64_t* out_ids,
                                            int64_t n_slots, int nq, int max_nprobe, int m, int k,
                                            tpq_stream_t stream) {
  const ScanArgs a = scan_args(codes, nullptr, part1 ? part1 : full_lut, is_empty, cell_start, cell_size, n_probe_list,
                               out_vals, out_addr, address2id, out_ids, n_slots, nq, max_nprobe, m, k, 1);
  int rc = validate(a);
  if (rc) return rc;
  TPQ_REQUIRE(base_sims != nullptr, "ivfpq_scan_residual: base_sims is required");
  TPQ_REQUIRE(full_lut != nullptr || (part1 && part2 && cells),
              "ivfpq_scan_residual: need either full_lut or (part1, part2, cells)");
  if (nq == 0) return TPQ_OK;
  ResidualArgs ra{part1, part2, full_lut, cells, base_sims, nullptr, nullptr};
  return run_residual_ref(a, ra, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int tpq_ivfpq_scan_topk_residual_packed(
    const uint8_t* packed, const uint8_t* codes, const float* part1, const float* query,
    const float* codebook, int ds, const float* part2, const float* slot_term,
    const float* cell_bound, const int64_t* cells, const float* base_sims, const uint8_t* is_empty,
    const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
    float* out_vals, int64_t* out_addr, const int64_t* address2id, int64_t* out_ids,
    int64_t n_slots, int nq, int max_nprobe, int m, int k, int n_split, void* workspace,
    size_t workspace_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(part1 || (query && codebook && ds >= 1 && ds <= 1024),
              "ivfpq_scan_residual_packed: need part1 or (query, codebook, ds)");
  TPQ_REQUIRE(part2 && slot_term && cell_bound && cells && base_sims,
              "ivfpq_scan_residual_packed: null pointer argument");
  ScanArgs a = scan_args(codes, packed, part1, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr,
                         address2id, out_ids, n_slots, nq, max_nprobe, m, k, n_split);
  a.query = query; a.codebook = codebook; a.ds = ds;
  a.euclid = 2;  // the in-workgroup LUT is part1 = 2 q_j.r_jc
  ResidualArgs ra{part1, part2, nullptr, cells, base_sims, slot_term, cell_bound};
  return run_packed(a, &ra, workspace, workspace_bytes, stream);
}

// ---- per-slot / per-cell constants of the packed residual scan ----------------------------------
namespace tpq {
// slot_term[s] = sum_j part2[cell(s)][j][code_j(s)] (ascending j, fp32) for the slots inside
// [cell_start, cell_start + cell_size); cell_bound[c] = sum_j max_c' |part2[c][j][c']|
__global__ __launch_bounds__(256) void residual_slot_term_kernel(
    const uint32_t* __restrict__ codes32, const float* __restrict__ part2,
    const int64_t* __restrict__ cell_start, const int64_t* __restrict__ cell_size,
    float* __restrict__ slot_term, int64_t n_slots, int m) {
  const int cell = blockIdx.x;
  const float* __restrict__ p2 = part2 + (int64_t)cell * m * 256;
  const int64_t st = cell_start[cell], sz = cell_size[cell];
  const int G = m >> 2;
  for (int64_t o = (int64_t)blockIdx.y * 256 + threadIdx.x; o < sz; o += (int64_t)gridDim.y * 256) {
    const int64_t s = st + o;
    float v = 0.f;
    for (int g = 0; g < G; ++g) {
      const uint32_t w = codes32[(int64_t)g * n_slots + s];
      v = lut_word(v, p2 + g * 1024, w);
    }
    slot_term[s] = v;
  }
}

__global__ __launch_bounds__(64) void residual_cell_bound_kernel(const float* __restrict__ part2,
                                                                 float* __restrict__ cell_bound,
                                                                 int m) {
  const int cell = blockIdx.x, lane = threadIdx.x;
  const float4* __restrict__ p2 = reinterpret_cast<const float4*>(part2 + (int64_t)cell * m * 256);
  float sum = 0.f;
  for (int j = 0; j < m; ++j) {
    const float4 x = p2[j * 64 + lane];
    float mx = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    sum += mx;
  }
  if (lane == 0) cell_bound[cell] = sum;
}
}  // namespace tpq

extern "C" int tpq_ivfpq_residual_slot_terms(const uint8_t* codes, const float* part2,
                                             const int64_t* cell_start, const int64_t* cell_size,
                                             float* slot_term, float* cell_bound, int64_t n_slots,
                                             int n_cells, int m, tpq_stream_t stream) {
  TPQ_REQUIRE(codes && part2 && cell_start && cell_size && slot_term && cell_bound,
              "ivfpq_residual_slot_terms: null pointer argument");
  TPQ_REQUIRE(m >= 4 && m % 4 == 0 && n_cells >= 1 && n_slots >= 0 && n_slots < 0x7fffffffLL,
              "ivfpq_residual_slot_terms: bad shape (m=%d, n_cells=%d, n_slots=%lld)", m, n_cells,
              (long long)n_slots);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc = check_hip(hipMemsetAsync(slot_term, 0, (size_t)n_slots * 4, st), "slot_terms memset");
  if (rc) return rc;
  hipLaunchKernelGGL(residual_cell_bound_kernel, dim3(n_cells), dim3(64), 0, st, part2, cell_bound, m);
  TPQ_LAUNCH_CHECK("residual_cell_bound_kernel");
  if (n_slots == 0) return TPQ_OK;
  const int per_cell = (int)((n_slots / n_cells + 255) / 256);
  const int by = per_cell < 1 ? 1 : (per_cell > 64 ? 64 : per_cell);
  hipLaunchKernelGGL(residual_slot_term_kernel, dim3(n_cells, by), dim3(256), 0, st,
                     reinterpret_cast<const uint32_t*>(codes), part2, cell_start, cell_size,
                     slot_term, n_slots, m);
  TPQ_LAUNCH_CHECK("residual_slot_term_kernel");
  return TPQ_OK;
}

extern "C" int tpq_residual_part1(const float* query, const float* codebook, float* part1, int m,
                                  int ds, int nq, tpq_stream_t stream) {
  TPQ_REQUIRE(query && codebook && part1, "residual_part1: null pointer");
  TPQ_REQUIRE(m >= 1 && m <= 65535 && ds >= 1 && nq >= 0, "residual_part1: bad shape");
  if (nq == 0) return TPQ_OK;
  hipLaunchKernelGGL(residual_part1_kernel, dim3(nq, m), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), query, codebook, part1, m, ds, nq);
  TPQ_LAUNCH_CHECK("residual_part1_kernel");
  return TPQ_OK;
}
