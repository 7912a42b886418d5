// IVF list scan, cell-major form of the m = 64 large-batch route (scan_cells.hip): what scan.hip and the unit share.
#pragma once
#include "common.h"

namespace tpq {

// probes per query the threshold pass scans with the query-major route (profiles/cell_major_bench.json)
#ifndef TPQ_CELL_P0
#define TPQ_CELL_P0 4  // (variant builds: the A/B of 3, 4 and 6)
#endif
constexpr int kCellP0 = TPQ_CELL_P0;
// The threshold form (scan_cells.hip: `The threshold from group maxima`): no query-major pass at all.  The candidate
// kernel's pass A runs over each query's first kCellThrProbes probes and keeps, per lane and tile, the maximum of every
// kCellThrGroup of its 16 rows; the k-th largest of a query's maxima bounds its k-th best value from below.
#ifndef TPQ_CELL_THR_PROBES
#define TPQ_CELL_THR_PROBES 6  // (variant builds: the A/B of 4, 6 and 8 -- profiles/cell_threshold_bench.json)
#endif
#ifndef TPQ_CELL_THR_GROUP
#define TPQ_CELL_THR_GROUP 16  // (variant builds: the A/B of 8 and 16)
#endif
constexpr int kCellThrProbes = TPQ_CELL_THR_PROBES;
constexpr int kCellThrGroup = TPQ_CELL_THR_GROUP;
static_assert(kCellThrGroup == 8 || kCellThrGroup == 16, "a group is half or all of a lane's 16 rows of a tile");
// the threshold form is taken from this mean length of a probed cell on: the maxima of short cells are few, and the
// existing form's tests pin its behaviour at mean cells of 50 - 381 slots
constexpr int kCellThrMinCell = 512;
// the form applies from this many re-reads of the mean code byte on (nq x slots_hint / n_slots)
constexpr int kCellMinRereads = 96;
constexpr int kCellQSplit = 256;  // halfs per query of the split copy: [hi, lo][128 components]
constexpr int kCellGroup = 32;   // queries per candidate block: the 32 MFMA columns of a wave
// A candidate block -- (cell, group) over the cell's whole length -- is dealt in this many pieces of whole tiles: piece i
// of S covers tiles [i nt / S, (i + 1) nt / S) of the cell's nt = ceil(size / 32).  The launch ends a block's length
// after its last draw at the latest; pieces shorten that unit (profiles/cell_pieces_bench.json).  1: the block undivided
#ifndef TPQ_CELL_PIECES_A
#define TPQ_CELL_PIECES_A 2  // pass A of the threshold form (variant builds: the A/B of 1, 2 and 4)
#endif
#ifndef TPQ_CELL_PIECES_B
#define TPQ_CELL_PIECES_B 1  // the candidates proper, either form: 2 stayed inside the trace-to-trace variation
#endif
constexpr int kCellPiecesA = TPQ_CELL_PIECES_A, kCellPiecesB = TPQ_CELL_PIECES_B;
static_assert(kCellPiecesA >= 1 && kCellPiecesA <= 8 && kCellPiecesB >= 1 && kCellPiecesB <= 8, "pieces per block");
constexpr int cell_pieces(bool maxima) { return maxima ? kCellPiecesA : kCellPiecesB; }
// the inversion counts and scatters per workgroup, over a slice of this many consecutive queries, in an LDS histogram of
// one int per cell (profiles/cell_inversion_bench.json)
#ifndef TPQ_CELL_SLICE
#define TPQ_CELL_SLICE 128  // (variant builds: the A/B of 128, 256 and 512)
#endif
constexpr int kCellSlice = TPQ_CELL_SLICE;
// cells the LDS histogram takes: 64 KiB, two workgroups per CU.  Beyond it the inversion issues one global atomic per
// listed pair (a slice's pairs hardly share a cell there, and every workgroup would walk the whole histogram twice)
constexpr int kCellLdsCells = 16384;

// one view of the inversion: the pairs of a range of probes grouped by cell (the fields of that name in CellArgs)
struct CellView {
  int *hist, *cell_off, *blk_off, *cell_st, *cell_sz, *pairs;
};

struct CellArgs {
  const uint8_t* codes;          // reference layout [16][n_slots][4]
  const float* query;            // [64 ds][nq]
  const float* codebook;         // [64][ds][256]
  const uint8_t* is_empty;       // nullable
  const int64_t* cell_start;     // [nq][max_nprobe]
  const int64_t* cell_size;
  const int64_t* n_probe_list;   // [nq]
  const int64_t* cells;          // [nq][max_nprobe]
  int64_t n_slots;
  int nq, max_nprobe, n_cells, ds, euclid;
  int p0;                        // the pairs listed are (q, p), p0 <= p < min(n_probe_list[q], p_hi)
  int p_hi;                      // (max_nprobe: every probe from p0 on)
  int k;                         // seeds per query (0: none)
  int thr_k;                     // the threshold form: the call's k (k == 0 there; 0 everywhere else)
  int work;                      // the candidate kernel's block counter: params + 8 + work (0 or 1)
  int chunks;                    // capacity of a query's lists in chunks of 64 keys, seed chunks included
  int epoch;                     // flags[q] == epoch: the query takes no part / overflowed
  float rel;                     // delta_q = rel (|q| + |x|max)^2
  const float* seed_vals;        // [nq][k]: the threshold pass's result, tau_q = its k-th value ...
  const int64_t* seed_addr;
  const float* thr_in;           // ... or (k == 0) the caller's thresholds [nq]
  unsigned* keys;                // [nq][chunks * 64] value images
  unsigned* idx;                 // [nq][chunks * 64] ~address
  int* list_evict;               // [nq][chunks], zeroed (nullable)
  int* flags;                    // [nq]
  float* ws_delta;               // [nq] <- 2 delta_q
  // behind the lists (cell_extra_bytes): every array rounded up to 256 bytes
  float* params;                 // [4] max |codebook|, sum_j max_c |c_jc|^2, 0 / 1: the codebook can be scaled
  float* thr;                    // [nq] tau_q - delta_q; euclidean: folded over |q|^2 (cell_fold_threshold)
  float* qscale;                 // [nq] the query's power-of-two scale
  float* qnorm;                  // [nq] |q|^2
  int* cnt;                      // [nq] candidates admitted (beyond the capacity: counted, not stored)
  int* hist;                     // [n_cells] pairs per cell, then the scatter's cursor
  int* cell_off;                 // [n_cells + 1]
  int* blk_off;                  // [n_cells + 1] exclusive prefix of ceil(pairs / kCellGroup)
  int* cell_st;                  // [n_cells] start and size of a listed cell
  int* cell_sz;
  int* pairs;                    // [nq (max_nprobe - p0)] the queries, grouped by cell
  _Float16* qsplit;              // [nq][2][128] the fp16 pieces of s_q q (hi, lo)
  // behind the extras, when the workspace has the room (cell_norm_bytes); nullptr: the candidate kernel's own chain
  float* norm;                   // [n_slots] |x'|^2 / s_x^2 of every slot of a listed cell, by address (NaN: tombstone)
  // the threshold form (behind the norms, cell_thr_bytes): the second inversion's histogram, which cell_prep_kernel
  // zeroes with the first (nullptr: none), and where cell_kth_kernel leaves the number of maxima pass A reserved
  // (nullptr: nowhere)
  int* hist2;                    // [n_cells]: the one walk's second histogram and cursor (pass A's view) as well
  int* n_max;                    // [nq]
  // the threshold form's one walk (launch_cell_threshold, n_cells <= kCellLdsCells / 2: two LDS histograms): the count,
  // scan and scatter launches of the view above also count (into hist2) and place the pairs with p < p_a -- pass A's
  // view -- into this one (va.hist == hist2); p_a == 0: one view
  int p_a;
  CellView va;
  // what depends on the index alone (`The kept state`, scan_cells.hip).  kparams: the four numbers of cell_prep_kernel --
  // params itself, or the head of a caller-owned kept state; the block counters stay at params + 8.  book: the split
  // codebook as the candidate kernels stage it (CellBook<DS>), copied into LDS instead of converted; nullptr: no kept
  // state, every workgroup converts.  With a kept state `norm` points into it and covers every slot address.
  // kept_build: the state is not valid yet -- this call writes it first, on its stream
  float* kparams;
  unsigned* book;
  int kept_build;
  // the MFMA products per k-step of the candidate kernels (scan_cells.hip: `The single-product key`): 3, or 1 -- the
  // threshold form at ds = 2 when the switch is on; `rel` is then cell_delta1_rel and the seed kernel adds the query's
  // own term from the piece maxima at kparams + kCellPieceMaxAt
  int products;
};
// the piece maxima of cell_prep_kernel in the 256-byte parameter block: 64 numbers of 16 bits from this byte on -- per
// pair i of sub-quantizers (2 i, 2 i + 1) the larger max_c |hi piece of s_x c_jc| (32 numbers), then the same of the lo
// pieces --, each the upper half of an fp32 rounded UP.  Bytes [0, 16) and the block counters at ints 8 and 9 stay
constexpr int kCellPieceMaxAt = 64;
// the kept state: [256 bytes: the parameters][the codebook image, 64 x 256 x 4 ds bytes][an fp32 norm per slot address]
inline size_t cell_book_bytes(int ds) { return (size_t)64 * 256 * 4 * ds; }
inline size_t cell_kept_bytes(int64_t n_slots, int ds) {
  return 256 + cell_book_bytes(ds) + ((((size_t)(n_slots > 0 ? n_slots : 0) * 4) + 255) & ~(size_t)255);
}
// points a.kparams, a.book and a.norm into the kept state at `kept` (cell_kept_bytes of it)
inline void cell_use_kept(CellArgs& a, void* kept, int valid) {
  char* p = reinterpret_cast<char*>(kept);
  a.kparams = reinterpret_cast<float*>(p);
  a.book = reinterpret_cast<unsigned*>(p + 256);
  a.norm = reinterpret_cast<float*>(p + 256 + cell_book_bytes(a.ds));
  a.kept_build = valid ? 0 : 1;
}
// the arrays of the threshold form: pass B's pairs (all probes: the extras hold max_nprobe - kCellP0 per query), then
// pass A's inversion -- hist, cell_off, blk_off, cell_st, cell_sz, pairs --, then the maxima counts [nq]
struct CellThrArrays {
  int* pairs_b;
  int *hist, *cell_off, *blk_off, *cell_st, *cell_sz, *pairs, *n_max;
};

// the view the loose fields of `a` describe
__host__ __device__ inline CellView cell_view(const CellArgs& a) {
  return CellView{a.hist, a.cell_off, a.blk_off, a.cell_st, a.cell_sz, a.pairs};
}
inline size_t cell_align(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t cell_extra_bytes(int nq, int max_nprobe, int n_cells, int p0) {
  const int np = max_nprobe > p0 ? max_nprobe - p0 : 0;
  return 256 + 4 * cell_align((size_t)nq * 4) + cell_align((size_t)n_cells * 4) +
         2 * cell_align(((size_t)n_cells + 1) * 4) + 2 * cell_align((size_t)n_cells * 4) +
         cell_align((size_t)nq * np * 4) + cell_align((size_t)nq * kCellQSplit * 2);
}
// the slot norms of a call (cell_norm_kernel): one fp32 per slot address
inline size_t cell_norm_bytes(int64_t n_slots) { return cell_align((size_t)(n_slots > 0 ? n_slots : 0) * 4); }
// the threshold form's arrays (CellThrArrays), behind the extras and the norms
inline size_t cell_thr_bytes(int nq, int max_nprobe, int n_cells) {
  const int t = max_nprobe < kCellThrProbes ? max_nprobe : kCellThrProbes;
  return cell_align((size_t)nq * max_nprobe * 4) + 3 * cell_align((size_t)n_cells * 4) +
         2 * cell_align(((size_t)n_cells + 1) * 4) + cell_align((size_t)nq * t * 4) + cell_align((size_t)nq * 4);
}
// The candidate kernel's folded threshold.  A row is admitted when fl(a - q2) >= thr (a = fl(2 dot - |x|^2), q2 = |q|^2
// finite); rounding is monotone, so the rows admitted are those with a >= thr2 for ONE float thr2 = the smallest a that
// passes, and the subtraction leaves the tile loop.  -inf stays -inf, +inf stays +inf, NaN stays NaN (nothing passes).
// fl(thr + q2) is only where the search starts: where thr + q2 cancels (thr = -1 + 2^-24, q2 = 1) it is millions of
// floats away from thr2, so the search doubles its step until it brackets thr2 and bisects -- two or three evaluations
// in the common case.  Floats are walked by their order-preserving integer image (both zeros -> 0).
__host__ __device__ inline int cell_float_ord(float f) {
  const unsigned b = __builtin_bit_cast(unsigned, f);
  return (b & 0x80000000u) ? (int)(0x80000000u - b) : (int)b;
}
__host__ __device__ inline float cell_ord_float(int o) {
  return __builtin_bit_cast(float, o >= 0 ? (unsigned)o : 0x80000000u - (unsigned)o);
}
__host__ __device__ inline float cell_fold_threshold(float thr, float q2) {
  constexpr long long kTop = 0x7f800000;  // the image of +inf
  if (!(thr == thr) || thr == __builtin_inff() || thr == -__builtin_inff()) return thr;
  auto pass = [&](long long o) { return (cell_ord_float((int)o) - q2) >= thr; };
  const float t0 = thr + q2;
  if (!(t0 == t0)) return t0;  // (q2 not finite: nothing passes)
  long long lo, hi, step = 1;  // !pass(lo), pass(hi); -inf never passes a finite threshold, +inf always does
  if (pass(cell_float_ord(t0))) {
    hi = cell_float_ord(t0);
    for (;; step *= 2) {
      lo = hi - step > -kTop ? hi - step : -kTop;
      if (lo == -kTop || !pass(lo)) break;
      hi = lo;
    }
  } else {
    lo = cell_float_ord(t0);
    for (;; step *= 2) {
      hi = lo + step < kTop ? lo + step : kTop;
      if (hi == kTop || pass(hi)) break;
      lo = hi;
    }
  }
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (pass(mid)) hi = mid; else lo = mid;
  }
  return cell_ord_float((int)hi);
}

// points the extras of `a` into `at` (cell_extra_bytes of it); `room` bytes are the caller's from `at` on: the slot
// norms follow the extras when they fit, else a.norm = nullptr.  layout_p0 >= 0: the extras are laid out as for that first
// probe whatever a.p0 is (the threshold form keeps the seeded form's layout, whose pairs array it leaves unused)
void cell_fill_extras(CellArgs& a, void* at, size_t room, int layout_p0 = -1);
// delta_q / (|q| + |x|max)^2 (derivation: scan_cells.hip)
float cell_delta_rel(int ds);
// the single-product key's delta_q is 1.25 x the query's own term (the seed kernel's) + this x (|q| + |x|max)^2
float cell_delta1_rel(int ds);
// whether the single-product candidate kernels are built for this ds (ds = 1 stays on three products)
inline bool cell_single_product_built(int ds) { return ds == 2; }
// stages 2-4 on `st`: seed (or the caller's thresholds), inversion, candidates
int launch_cell_candidates(const CellArgs& a, hipStream_t st);
// points `t` into `at` (cell_thr_bytes of it)
void cell_fill_thr(CellThrArrays& t, void* at, int nq, int max_nprobe, int n_cells);
// the threshold form on `st`, a.k == 0, a.thr_k = the call's k, a.norm set, a.p0 == 0: per-query part, inversion of all
// probes and slot norms, inversion of the first kCellThrProbes, pass A (group maxima into a.keys), cell_kth_kernel (thr,
// zero counts) and the candidates of all probes
int launch_cell_threshold(const CellArgs& a, const CellThrArrays& t, hipStream_t st);

}  // namespace tpq
