// IVF list scan: the kernels' arguments, the modes of scan_packed_kernel and the constants every stage shares.
#pragma once
#include "common.h"
#include "scan_layout.h"
#include "wave_topk.h"

namespace tpq {

#ifndef TPQ_LUT_U
#define TPQ_LUT_U 4  // fused LUT build, ds <= 2: entries (float4 groups) per thread whose codebook loads are issued together
#endif
// pool mode: the counting rounds that tighten the cut before the exact evaluation pay beyond this k (same box, m = 64, ms
// per 10 000 queries, 0 / 1 / 3 rounds COMPILED IN: k = 600: 4.79 / 5.14 / 5.27, k = 800: 5.19 / 5.50 / 5.68, k = 1000:
// 6.66 / 6.70 / 6.08; three rounds compiled in and none executed: 5.48 at k = 600 -- hence a kernel of its own, RM = -3)
constexpr int kPoolRoundsFromK = 900;
// pool mode from list_regs_packed(k) = 16 on, i.e. k > 504 (eight waves, from k > 248 with pools of 1 024 and no rounds,
// same box, ms per 10 000 queries, lists -> pool: m = 64, k = 300 / 400 / 500: 3.57 / 3.79 / 3.96 -> 3.76 / 3.95 / 4.09)
constexpr int kPoolMinListRegs = 16;
// ... and, with four waves per workgroup (m <= 32), from list_regs_packed(k) = 8 on (k > 248, where the fused finish of the
// sorted lists ends): lists -> pools of 2 048 without rounds, same box, ms per 10 000 queries: m = 32, k = 300 / 400 / 500:
// 3.49 / 3.72 / 3.96 -> 2.67 / 2.83 / 2.97; m = 16, k = 300 / 500: 2.27 / 2.55 -> 1.65 / 1.82; m = 8, k = 400: 2.32 -> 1.45;
// IVF4096 cells, m = 32, k = 400: 3.33 -> 1.99.  (k <= 248 stays with the lists: m = 32, k = 248: 2.04 against 2.40.)
static int pool_min_list_regs(int m) { return m <= 32 ? 8 : kPoolMinListRegs; }
constexpr int kScanWaves = 8;
constexpr int kScanThreads = kScanWaves * 64;

// ws_delta[q] after a call: the value scan_ref_kernel / scan_residual_kernel leave when they redo a FLAGGED query (a
// selection band is >= 0 and the one-launch finisher writes 1.f / 0.f: -1 is neither) -- IVFPQTopkHip.last_redone
constexpr float kRedoneMark = -1.f;

struct ScanArgs {
  const uint8_t* codes;    // reference layout [m/4][n_slots][4]
  const uint8_t* packed;   // scan layout (packed kernel only)
  const float* lut;        // [m][nq][256]; nullptr = build the LUT in the workgroup ("fused")
  const float* query;      // fused: [m*ds][nq]
  const float* codebook;   // fused: [m][ds][256]
  int ds, euclid;          // fused: sub-vector length, 1 = 2ab-a^2-b^2 / 0 = dot / 2 = 2ab
  const uint8_t* is_empty; // nullable
  const int64_t* cell_start;
  const int64_t* cell_size;
  const int64_t* n_probe_list;
  float* out_vals;
  int64_t* out_addr;
  const int64_t* address2id;
  int64_t* out_ids;
  float* ws_vals;  // [nq][n_split][64R]
  int* ws_idx;
  int* flags;             // [nq] packed path: == epoch: candidate band overflowed, redo exactly.  Never zeroed:
                          // "raised" is equality with this call's epoch (the workspace arrives as garbage; a
                          // word that happens to equal the epoch costs one needless exact redo, never a wrong result)
  float* ws_delta;        // [nq] packed path: fast-vs-exact error bound of the query
  const int* only_flagged;  // reference kernel: when set, only queries with a non-zero flag run
  int64_t n_slots;
  int nq, max_nprobe, m, k, n_split;
  unsigned long long* prof;  // -DTPQ_SCAN_PROFILE builds: [nq][16] phase timestamps (10 ns ticks)
  int small_lists;           // packed path, large k: per-wave lists hold fewer than k + 8 entries
  int epoch;                 // value that marks a raised flag in this call (non-zero)
  int* tickets;              // fused finish, n_split > 1: the CALLER's [nq] int32, zero on entry, zero on exit
  int fuse;                  // fused finish (scan_packed_kernel RM > 0): the scan workgroups write the result
  int64_t slots_hint;        // host only: expected slots scanned per query (0 = unknown), sizes the per-wave lists
  // pool mode (k > 248, scan_packed_kernel RM < 0): per (query, split, wave) an append-only pool of pool_cap
  // admitted candidates (keys: value image, ~address), later overwritten in place by the exact candidates
  unsigned* pool_hi;
  unsigned* pool_lo;
  int* pool_cnt;             // [nq][n_lists] exact candidates the list holds after the scan kernel
  int pool_cap;
  // dump mode (scan_packed_kernel RM <= kDumpF32): [nq][n_lists] 1 = the wave's list may have evicted a candidate
  int* list_evict;
  // dump mode, "tail split": queries [0, unsplit) run as ONE workgroup each, queries [unsplit, nq) as n_split
  // workgroups each (0 = every query is split n_split ways, the meaning of n_split everywhere else).  A batch that is
  // not a multiple of the chip's workgroup slots ends with a round of few workgroups, each as long as a whole query
  // (1 250 queries on 1 024 slots: two rounds for 1.22 rounds of work); the queries of that last round are dealt
  // as short workgroups instead -- they start last (workgroups are dispatched in blockIdx order) and fill the slots
  // the long ones leave.  The lists keep the stride of n_split parts for every query.
  int unsplit;
  // dump mode, dispatch order (scan_order.hip): order[i] = the query the i-th workgroup (the i-th group of n_split
  // workgroups, past `unsplit`) scans -- the batch's queries longest first, so that the batch ends on its shortest --,
  // rank = its inverse: a query runs unsplit when rank[q] < unsplit.  nullptr = index order.  Everything else is
  // indexed by the query, as before: the results do not depend on the order.
  const int* order;
  const int* rank;
  // probe cap (the cell-major form's threshold pass, scan_cells.h): every kernel that walks a query's probes takes
  // min(n_probe_list[q], probe_cap) of them -- clamped_n_probe (scan_list.h), scan_work_kernel.  0 = no cap.
  int probe_cap;
};

// scan_packed_kernel modes beyond the fused finish (RM > 0) and the pools (RM = -1, -2, -3): "dump" -- the scan
// workgroup ends with its waves' lists of FAST values; scan_finish_exact_kernel (one wave per query, full occupancy)
// merges them, evaluates the band's survivors exactly from global memory and writes the result.
constexpr int kDumpF32 = -8;     // fp32 table in LDS (m KiB), the permuted-order fp32 sum as the selection key
constexpr int kDumpSel16 = -16;  // 16-bit fixed-point table (m / 2 KiB), an exact integer sum as the selection key
constexpr int kDumpSel16W8 = -17;  // the same with the eight waves of the other paths (k in (248, 504]: lists of <= 2 registers)
constexpr bool is_sel16(int RM) { return RM == kDumpSel16 || RM == kDumpSel16W8; }
// the mode, from the kernel's RM: > 0 fused finish (RM = registers of the merged list), 0 three launches, -1 / -2 / -3 pools
// (1 024 entries per wave; 2 048; 2 048 without the counting rounds: kPoolRoundsFromK), <= kDumpF32 the dump modes
constexpr bool is_dump(int RM) { return RM <= kDumpF32; }
constexpr bool is_pool(int RM) { return RM < 0 && !is_dump(RM); }
constexpr bool is_fused(int RM) { return RM > 0; }
constexpr int pool_regs(int RM) { return RM == -1 ? 16 : 32; }   // pool registers at read-back: pool_cap = 64 x this
constexpr int pool_rounds(int RM) { return RM == -3 ? 0 : 3; }   // counting rounds over the pools
// which m take which dump mode: m = 64 the 16-bit table (both forms), m = 8, 16, 32 (round 6) the fp32 table
constexpr bool dump_built(int m, int mode) {
  return is_sel16(mode) ? m == 64 : (mode == kDumpF32 && (m == 8 || m == 16 || m == 32));
}
// the (RL = registers of the scan's per-wave lists, Rf = of the finish kernel's exact list) pairs instantiated per dump
// mode -- what list_regs_scan / dump_finish_regs produce today; plan_scan (scan.hip) declines the route for any other
#define TPQ_DUMP_PAIRS(X)                                                                                     \
  X(kDumpSel16W8, 1, 8) X(kDumpSel16W8, 2, 8) X(kDumpSel16W8, 2, 16)                                          \
  X(kDumpF32, 1, 1) X(kDumpF32, 1, 2) X(kDumpF32, 2, 2) X(kDumpF32, 1, 4) X(kDumpF32, 2, 4) X(kDumpF32, 4, 4) \
  X(kDumpF32, 2, 8) X(kDumpF32, 4, 8) X(kDumpF32, 4, 16)                                                      \
  X(kDumpSel16, 1, 1) X(kDumpSel16, 1, 2) X(kDumpSel16, 2, 2) X(kDumpSel16, 1, 4) X(kDumpSel16, 2, 4)         \
  X(kDumpSel16, 2, 8) X(kDumpSel16, 4, 8)
constexpr bool dump_pair_built(int mode, int RL, int Rf) {
#define TPQ_IS_PAIR(MODE, A, B) if (mode == MODE && RL == A && Rf == B) return true;
  TPQ_DUMP_PAIRS(TPQ_IS_PAIR)
#undef TPQ_IS_PAIR
  return false;
}
constexpr int kDumpMinQueries = 1024;  // batches that fill the chip's 4 x 256 workgroup slots at least once
constexpr int kDumpShortMaxK = 248;    // m = 8, 16, 32 (kDumpF32): the pools take the larger k
constexpr int kDumpLutMinSlots = 24576;  // ... with a caller's table: from this many expected slots per query on

#ifdef TPQ_SCAN_PROFILE
#define TPQ_PROF(a, q, i)                                                        \
  do {                                                                           \
    if ((a).prof && threadIdx.x == 0) (a).prof[(int64_t)(q) * 16 + (i)] = wall_clock64(); \
  } while (0)
#else
#define TPQ_PROF(a, q, i) ((void)0)
#endif

// Volatile accesses to LDS words other waves update (the shared admission threshold, the waves' quantiles) go through an
// LDS-ADDRESS-SPACE pointer.  A `volatile T*` cast of a generic pointer compiles to FLAT loads, and FLAT counts on vmcnt:
// the `s_waitcnt vmcnt(0)` hipcc put behind the per-tile threshold poll made every wave wait, once per tile, until the NEXT
// tile's code loads -- the software pipeline's prefetch, issued a few hundred cycles earlier -- had landed (round 6, read
// off the ISA of the tile loop: `flat_load_dword ... sc0 sc1` + `s_waitcnt vmcnt(0)`).  ds_read_b32 counts on lgkmcnt only.
__device__ __forceinline__ unsigned lds_poll_u32(const unsigned* p) {
  typedef const volatile __attribute__((address_space(3))) unsigned* lds_ptr;
  return *(lds_ptr)p;
}
__device__ __forceinline__ float lds_poll_f32(const float* p) {
  typedef const volatile __attribute__((address_space(3))) float* lds_ptr;
  return *(lds_ptr)p;
}
__device__ __forceinline__ void lds_post_f32(float* p, float v) {
  typedef volatile __attribute__((address_space(3))) float* lds_ptr;
  *(lds_ptr)p = v;
}

// residual PQ: the tables and per-probe terms of scan_residual_kernel (scan_ref.h) and of the packed kernel (RES)
struct ResidualArgs {
  const float* part1;       // [nq][m][256]        (mode A; nullptr = 2 q_j.r_jc built from query/codebook)
  const float* part2;       // [n_cells][m][256]   (mode A)
  const float* full;        // [nq][max_nprobe][m][256] (mode B) or nullptr
  const int64_t* cells;     // [nq][max_nprobe]    (mode A)
  const float* base_sims;   // [nq][max_nprobe]
  const float* slot_term;   // packed kernel: [n_slots] sum_j part2[cell(s)][j][code_j(s)]
  const float* cell_bound;  // packed kernel: [n_cells] sum_j max_c |part2[cell][j][c]|
};

}  // namespace tpq
