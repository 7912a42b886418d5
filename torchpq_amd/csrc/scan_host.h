// IVF list scan, host side: list sizing, LDS and workspace sizes, argument checks.  Needs TPQ_PACKED_M_LIST (scan_device.h).
// (check_lds, need_ws and what the list entry points share: scan_list.h, which scan_packed_kernel.h brings in)
#pragma once
#include "scan_args.h"
#include "scan_packed_kernel.h"
#include "scan_finish.h"

namespace tpq {

// splits per query the ranking kernel's LDS (64 KiB) can take
static int pool_max_split(int m, int k) {
  const int nw = packed_waves(m), len = 64 * (nw == 4 ? 8 : 4);
  const int kcap = (k + 63) / 64 * 64;
  int s = (int)((65536 - (size_t)kcap * 8) / ((size_t)nw * len * 8));
  return s < 1 ? 1 : s;
}

constexpr int kBandSlack = 8;  // spare list entries the packed path wants beyond k
static int list_regs_packed(int k) { return pow2_ceil((k + kBandSlack + 63) / 64); }
// ... and of the finish kernel's exact list on the dump routes: the band of the 16-bit table is ~70 table units wide
// whatever the values, and what lies within it below the k-th best grows with the slots scanned (k = 500 over 31 000
// slots: 504-520 survivors -- beyond 512 the query is redone by the exact kernel, 0.47 ms per 10 000 queries)
static int dump_finish_regs(int k, int64_t slots_hint) {
  // (up to 16 384 slots per query the extras stay within the 8 entries every packed path allows: k = 504 over 7 800
  // slots ran 2.58 ms against the lists' 3.36)
  const int slack = (slots_hint > 0 && slots_hint <= 16384) ? kBandSlack : 16 + k / 8;
  return pow2_ceil((k + slack + 63) / 64);
}
// ... and on the cell-major threshold form's single-product key (scan_cells.hip): its band is three to six times that of
// three products (SIFT-like data 3.3, Gaussian codebooks 5.8: the bound takes the LARGEST entry of a sub-quantizer), and
// what lies within it below the k-th best grows with it -- four times the slack above, whatever the slots (k = 100: 256
// entries instead of 128; k <= 128 stays within the 4 registers the finish kernel is built for beside 8)
static int cell_single_finish_regs(int k) { return pow2_ceil((k + 4 * (16 + k / 8) + 63) / 64); }
// Registers of the per-wave lists of the packed scan.  Tiles are dealt round-robin, so a wave's share
// of the top-k is ~k/NW: the lists are sized for at least 2k entries over the workgroup (64 RL per
// wave) instead of k + 8 per wave.  Folding 64 candidates into a 512- or 1024-entry sorted list used
// to dominate large k (k = 1000: 12.8 ms against 3.1 ms at k = 100, C2).  A wave that fills its list
// with candidates that still matter flags the query for the exact kernel (scan_packed_kernel).
#ifndef TPQ_SCAN_MIN_RL_K
#define TPQ_SCAN_MIN_RL_K 1  // experiment knob: below this k the lists keep the full k + 8
#endif
// The 2k budget counts on a cell's tiles being dealt to ALL the waves of the workgroup: the nearest cell alone
// can hold half of the top-k.  A cell much shorter than one round of tiles (waves x slots per tile: 512 slots at
// m = 64, 1024 at m = 32) lands in few waves -- on the reference's own benchmark grid (IVF4096 over 1 M vectors:
// 244 slots, ONE 256-slot tile at m <= 32) the 2k budget sent 1-2 % of the queries (93 % at n_probe = 1) through
// the exact redo at k = 100 (profiles/r04_reference_grid.json, "queries_redone_exactly") -- and gets 4k; so does
// a caller that gives no hint.  (Full-size lists everywhere would cost the long cells 10 % at k = 100, m <= 32.)
static int list_regs_scan(int k, int m, int max_nprobe, int64_t slots_hint, int waves = 0) {
  const int nw = waves ? waves : packed_waves(m);
  const int rp = list_regs_packed(k);
  if (k < TPQ_SCAN_MIN_RL_K) return rp;
  const int64_t round_slots = (int64_t)nw * 64 * packed_slots(m);
  // ("spread": the mean probed cell fills at least three quarters of a round of tiles)
  const bool spread = slots_hint > 0 && 4 * slots_hint >= 3 * round_slots * (max_nprobe > 0 ? max_nprobe : 1);
  const int budget = (spread ? 2 : 4) * k;
  int rl = 1;
  while (rl < rp && nw * 64 * rl < budget) rl <<= 1;
  return rl;
}

// pool mode (k > 248): registers of the threshold list (the wave's ceil(k / NW) best) and entries per pool
static int pool_list_regs(int k, int m) {
  const int nw = packed_waves(m);
  return pow2_ceil(((k + nw - 1) / nw + 63) / 64);
}
static int pool_capacity(int k, int m) {  // (16 / 32 registers per lane at read-back; four waves share a query's admissions)
  return (k <= 512 && m > 32) ? 1024 : 2048;
}  // (16 / 32 registers per lane at read-back)

// (the reference-layout kernels: list_scan_lds_bytes, scan_list.h)
static size_t scan_lds_bytes_packed(int m, int R, int max_nprobe, int fused_floats, bool res) {
  const int nw = packed_waves(m);
  size_t b = (size_t)m * 1024 + packed_aux_bytes(R, m) + nw * 512 +
             (size_t)(3 * max_nprobe + 1) * 4 + 8 + 3 * nw * 4 + (res ? 8 * (size_t)max_nprobe : 0) +
             (size_t)fused_floats * 4;
  return (b + 15) & ~(size_t)15;
}
// dump modes: no un-permute rows; the 16-bit table is half the size and runs four waves per workgroup
static size_t scan_lds_bytes_dump(int m, bool sel16, int nw, int max_nprobe, int fused_floats) {
  size_t b = (size_t)m * (sel16 ? 512 : 1024) + nw * 512 + (size_t)(3 * max_nprobe + 1) * 4 + 8 + 3 * nw * 4 +
             (size_t)fused_floats * 4;
  return (b + 15) & ~(size_t)15;
}
static int fused_floats_of(const ScanArgs& a) { return a.lut ? 0 : a.m * a.ds + a.m; }
// fused finish (scan_packed_kernel RM > 0): instantiated for merged lists of up to kFuseMaxR registers
// (k <= 248); its merge buffers -- waves x 64 RM keys -- lie over the LUT, the un-permute rows and the queues
constexpr int kFuseMaxR = 4;
static bool fuse_fits(int m, int RM) {
  const int nw = packed_waves(m);
  return RM <= kFuseMaxR &&
         (size_t)(nw + 1) * RM * 64 * 8 <= (size_t)m * 1024 + packed_aux_bytes(RM, m) + (size_t)nw * 512;
}

// the per-M units' entry points (the list of M: TPQ_PACKED_M_LIST, scan_device.h)
#ifndef TPQ_PACKED_M_LIST
#error "scan_host.h is included through scan_device.h, which defines TPQ_PACKED_M_LIST"
#endif
#define TPQ_DECLARE_PACKED(M) \
  int dispatch_packed_##M(const ScanArgs& a, const ResidualArgs* ra, int RL, int R, hipStream_t st); \
  int dispatch_pool_##M(const ScanArgs& a, int RL, hipStream_t st);                                  \
  int dispatch_dump_##M(const ScanArgs& a, int RL, int R, int mode, hipStream_t st);                 \
  int dump_occupancy_##M(int mode);                                                                  \
  int dispatch_finish_##M(const ScanArgs& a, int chunks, int R, int seed_chunks, const int* cnt, hipStream_t st);
TPQ_PACKED_M_LIST(TPQ_DECLARE_PACKED)
#undef TPQ_DECLARE_PACKED

template <class K>
static int set_lds(K kernel, size_t bytes, const char* name) {
  if (int rc = check_lds(name, bytes)) return rc;
  return check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes),
                   name);
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: [flags nq*4][delta nq*4][lists nq*n_lists*64R*8]; n_lists = n_split (reference
// kernel, only when n_split > 1) or n_split * waves-per-workgroup (packed kernel, always)
static size_t ws_bytes_for(int nq, int R, int n_lists) {
  return 2 * align256((size_t)nq * 4) + (size_t)nq * n_lists * R * 64 * 8 + align256((size_t)nq * n_lists * 4);
}

// pool mode workspace: [flags][delta][pool hi nq*n_lists*cap][pool lo ...][counts nq*n_lists]
static size_t pool_ws_bytes(int nq, int k, int m, int n_lists) {
  return 2 * align256((size_t)nq * 4) + (size_t)nq * n_lists * pool_capacity(k, m) * 8 +
         align256((size_t)nq * n_lists * 4);
}
static void fill_ws_pool(ScanArgs& a, void* workspace, int n_lists) {
  char* p = reinterpret_cast<char*>(workspace);
  a.flags = reinterpret_cast<int*>(p);
  a.ws_delta = reinterpret_cast<float*>(p + align256((size_t)a.nq * 4));
  char* pools = p + 2 * align256((size_t)a.nq * 4);
  a.pool_cap = pool_capacity(a.k, a.m);
  const size_t n = (size_t)a.nq * n_lists * a.pool_cap;
  a.pool_hi = reinterpret_cast<unsigned*>(pools);
  a.pool_lo = reinterpret_cast<unsigned*>(pools + n * 4);
  a.pool_cnt = reinterpret_cast<int*>(pools + n * 8);
}

static void fill_ws(ScanArgs& a, void* workspace, int R, int n_lists) {
  char* p = reinterpret_cast<char*>(workspace);
  a.flags = reinterpret_cast<int*>(p);
  a.ws_delta = reinterpret_cast<float*>(p + align256((size_t)a.nq * 4));
  char* lists = p + 2 * align256((size_t)a.nq * 4);
  a.ws_vals = reinterpret_cast<float*>(lists);
  a.ws_idx = reinterpret_cast<int*>(lists + (size_t)a.nq * n_lists * R * 64 * 4);
  a.list_evict = reinterpret_cast<int*>(lists + (size_t)a.nq * n_lists * R * 64 * 8);  // (dump modes)
}

static int validate(const ScanArgs& a) {
  TPQ_REQUIRE(a.codes && (a.lut || (a.query && a.codebook)) && a.cell_start && a.cell_size &&
                  a.n_probe_list && a.out_vals && a.out_addr,
              "ivfpq_scan: null pointer argument");
  TPQ_REQUIRE(a.lut || a.ds >= 1, "ivfpq_scan: bad sub-vector length %d", a.ds);
  TPQ_REQUIRE(a.nq >= 0 && a.max_nprobe >= 1, "ivfpq_scan: bad nq/max_nprobe (%d, %d)", a.nq,
              a.max_nprobe);
  TPQ_REQUIRE(a.m >= 4 && a.m % 4 == 0, "ivfpq_scan: n_subvectors=%d must be a positive multiple of 4", a.m);
  TPQ_REQUIRE(a.k >= 1 && a.k <= 1024, "ivfpq_scan: k=%d out of range (0, 1024]", a.k);
  TPQ_REQUIRE(a.n_slots >= 0 && a.n_slots < 0x7fffffffLL, "ivfpq_scan: n_slots=%lld out of range",
              (long long)a.n_slots);
  TPQ_REQUIRE(a.n_split >= 1 && a.n_split <= 1024, "ivfpq_scan: n_split=%d out of range", a.n_split);
  TPQ_REQUIRE((a.out_ids == nullptr) || (a.address2id != nullptr),
              "ivfpq_scan: out_ids given without address2id");
  return TPQ_OK;
}

}  // namespace tpq
