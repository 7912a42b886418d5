// IVF list scan, m = 64, large fused batches: the candidates of a batch taken CELL BY CELL on the fp16 matrix cores.
//
// The query-major scan (scan_packed_kernel) decodes every code byte once per query that probes its cell: ~300 times
// per launch on a cell-dense batch.  Here a probed cell is decoded once per group of 32 of its queries -- a look-up of
// ready-made fp16 pieces, no table address arithmetic per query -- and the values of the group come from one small GEMM,
// (decoded slots x 64 ds) . (64 ds x queries), on v_mfma_f32_32x32x16_f16.
// The values are a SELECTION key only: scan.hip seeds each query's lists with the exact top-k of its first kCellP0
// probes (the query-major route with a probe cap), this unit appends every slot of the other probes that may reach that
// top-k, and scan_finish_exact_kernel evaluates the lists exactly.  Nothing here selects, merges or redoes.
//
// Kernels (all on the caller's stream; no host read, no allocation):
//   cell_prep_kernel     one block: the codebook's max |entry| (-> the power-of-two scale s_x) and X^2 = sum_j max_c
//                        |c_jc|^2 >= |x|^2 of every decodable slot.  Not launched by a call that reads a kept state.
//   cell_seed_kernel     one wave per query: tau_q (the k-th seed, or the caller's threshold), the query's scale s_q and
//                        |q|^2, delta_q, the admission threshold tau_q - delta_q (euclidean: folded over |q|^2, see `The
//                        admission test`) and ws_delta = 2 delta_q; the seeds into the
//                        first ceil(k / 64) chunks of the query's lists in the finish kernel's format (value image,
//                        ~address), pads (~kPadIdx) behind them; zero counter and eviction words.  Over its whole grid
//                        it also zeroes what the later stages count in: the histogram(s) of the inversion and the
//                        candidate kernel's two block counters.
//                        A query that was flagged before, has a non-finite component, norm or
//                        threshold (NaN, +inf), cannot be scaled or lists a cell outside [0, n_cells) is flagged and takes
//                        no further part (tau = -inf is a threshold like any other: everything is admitted, and what
//                        does not fit flags the query below).
//   cell_count_kernel    the histogram of the listed (query, probe) pairs.  One workgroup per slice of kCellSlice
//                        consecutive queries: the slice's pairs, flattened over the threads (the rows of cells, cell_start
//                        and cell_size read coalesced), are counted with LDS atomics in a histogram of n_cells ints, and
//                        every cell the slice lists takes ONE global atomic with the slice's count.  (One global atomic
//                        per pair, from one wave per query, put ~270 atomics on each of the headline's 1 024 addresses
//                        and several times that on a popular cell; same-address atomics execute one after the other.
//                        Measured there, profiles/cell_inversion_bench.json: the seed kernel with that loop 89 us, without
//                        it 22; the scatter 81 us; count + scatter now 8 + 12 us at 128 queries per slice, the shortest
//                        of the three lengths measured -- 128, 256 and 512.)
//   cell_scan_kernel     one block: exclusive prefixes of the histogram (pairs) and of ceil(pairs / 32) (blocks).
//   cell_scatter_kernel  the same slices and the same LDS count; one RETURNING global atomic per listed cell reserves the
//                        slice's consecutive positions in the cell's range and leaves the first in LDS, and a second walk
//                        places the pairs: pairs[lds_cursor[cell]++] = q; the pair that takes a cell's first position
//                        writes the cell's extent.  The order inside a cell varies from run to run; nothing downstream
//                        depends on it.
//                        <true>, with a second block of cell_scan_kernel: the threshold form's ONE walk -- a second LDS
//                        histogram and cursor per cell for the pairs with p < kCellThrProbes, so that the three launches
//                        fill pass A's view beside pass B's (n_cells <= kCellLdsCells / 2; launch_cell_threshold).
//   cell_count_wide_kernel, cell_scatter_wide_kernel   n_cells > kCellLdsCells: one wave per query, one global atomic
//                        per pair -- the form both stages had before; a slice's pairs hardly share a cell there.
//   cell_norm_kernel     when the workspace has room for an fp32 per slot behind the other arrays (CellArgs::norm):
//                        |x'|^2 / s_x^2 of every slot of a listed cell, NaN for a tombstone, once per call -- the bits
//                        the candidate kernel's own chain forms in every (cell, block).  A thread per slot over a
//                        codebook of fp32 sums (hi piece + lo piece) in LDS, cells dealt over one workgroup per CU.
//   cell_cand_kernel     one block of work per (cell, group of <= 32 listed queries), taken by ONE WAVE, query per MFMA
//                        column: a lane owns one query, threshold and scales in registers, its B operand read as 16-byte
//                        pieces of the seed kernel's split copy.  One workgroup of eight waves per CU stages the codebook in
//                        LDS once -- already scaled and split into its two fp16 pieces, 128 KiB at ds = 2 -- and its waves
//                        take blocks from a counter, independently: no barrier after the staging.  Per tile of 32 slots,
//                        lane (row, half) reads the 8 code dwords of its half of every k-step from the reference layout
//                        [16][n_slots][4] (coalesced over slots, one tile ahead, unconditionally: rows past the size
//                        are clamped into the cell and masked afterwards) and gathers its A operand straight from
//                        the codebook in LDS; |x'|^2 is cell_norm_kernel's, loaded with the codes (NORMS), or rides
//                        along (an fma chain over the same pieces, the two half-waves added), and reaches the
//                        accumulator's rows through 128 bytes of LDS per wave.  A lane's admitted rows are staged in
//                        its own segment of LDS and take consecutive entries of its query's list from ONE counter
//                        update per flush -- at the end of the block, or when a segment is full (a returning atomic
//                        per row was four or five dependent round trips per tile, one per lane and tile still one).
//                        A probe listed twice in a row is skipped as the scan skips it (fetch_probes, scan_shared.h).
//                        A block is dealt in S pieces of whole tiles (scan_cells.h: kCellPiecesA for pass A, kCellPiecesB
//                        otherwise; 1: undivided): draw w is piece w % S of block w / S, its flush or its reservation
//                        of maxima the piece's own.  Whole tiles: the groups of pass A are the same sets of rows.
//                        <.., MAXIMA>: pass A of the threshold form -- group maxima instead of admitted rows.
//   cell_kth_kernel      the threshold form, one wave per query: the k-th largest of pass A's maxima -> thr[q]; zeroes
//                        cnt[q] (`The threshold from group maxima`, below).
//                        (Measured on the headline batch, 10 000 queries x 28 listed probes: sub-vectors gathered from
//                        the fp32 codebook in global memory into a staged 128-slot tile, 2.66 ms; this form with the
//                        queries read from [d][nq] per block, 1.06 ms; with the split copy, 0.91 ms; with the norms of a
//                        tile read in four 16-byte LDS reads and the codes loaded a tile ahead, 0.81 ms (0.78 in the
//                        later record, profiles/cell_norms_bench.json); with the norms of cell_norm_kernel, 0.68 +
//                        0.03 ms; with one counter update per lane and tile, 0.53 + 0.03 ms (0.55 in the later
//                        record, profiles/cell_pipeline_bench.json); with the tile's loads unconditional, so that they
//                        really run a tile ahead, 0.50 + 0.03 ms; with the admitted rows staged in LDS, 0.43 + 0.03 ms.
//                        Two 32-column query sets per decode -- 64 queries per block, 252 registers -- ran 0.55 ms
//                        and are not built: tools/experiments/cell_two_sets.patch; twelve waves per workgroup ran
//                        0.40 ms with four registers of <2, true> spilled, and are not built either.)
//
// Arithmetic.  q' = s_q q = qh + ql + rq,  x' = s_x x = xh + xl + rx  (h = fp16(.), l = fp16(. - h); s_q, s_x powers of
// two with max |q'_i|, max |s_x c| in [2^12, 2^13): no piece overflows, and the scaling is exact).  Per component
//   |r| <= 2^-22 |.| + eta,  eta = 2^-14   (a piece below the fp16 normal range, flushed or not).
// S = sum over the k-steps of (xl qh + xh ql + xh qh) on the MFMA, the small products of a step first, fp32 accumulation;
//   fast = 2 S / (s_q s_x) - |x|^2 - |q|^2   (euclidean; |x|^2 an fp32 fma chain of the decoding thread over (xh + xl)^2, unscaled; |q|^2
//   an fp32 sum of the seed kernel)         or   S / (s_q s_x)   (inner product).
// Against g = 2 q.x - |x|^2 - |q|^2 in real numbers, with Q = |q'|, X = |x'| and B = |q| + |x|max (|x|max^2 = X^2 above;
// 2 |q| |x| <= B^2 / 2; D = 64 ds components, N = 3 D MFMA terms):
//   dropped product and piece residues  |ql.xl + rq.x' + (qh + ql).rx| <= 3.03 2^-22 Q X + 1.01 eta sqrt(D) (Q + X)
//   fp32 accumulation, any order        N roundings of at most 2^-23 sum |terms| <= 1.003 N 2^-23 Q X
//     -> in value units (x 2 / (s_q s_x)):  (3.03 2^-22 + 1.003 N 2^-23) B^2 / 2  +  1.01 sqrt(D) 2^-26 B^2
//        (1 / s_x <= 2^-12 |x|max and 1 / s_q <= 2^-12 |q|, so eta (Q + X) / (s_q s_x) <= eta 2^-12 B^2 / 2)
//   the norm chains                     (D + 1) 2^-24 (|x|^2 + |q|^2) <= (D + 1) 2^-24 B^2
//   |x|^2 taken from the pieces         sum_i (xh + xl)_i^2 / s_x^2: 2^-21 |x|^2 + 2 eta sqrt(D) |x| / s_x <= 14 2^-24 B^2
//   the two subtractions, tau - delta   2^-22 B^2
//   the exact chain's own rounding      the reference's value is sum_j fl(fl(2 dot_j - |q_j|^2) - |c_j|^2), ascending j:
//                                       (ds + 3) 2^-24 sum_j (|q_j| + |c_j|)^2 + (m - 1) 2^-24 sum_j |val_j|
//                                       <= 1.001 (m + ds + 2) 2^-24 B^2
// delta_q = 1.25 x the sum (cell_delta_rel) x B^2, B evaluated upwards.  The inner product's errors are a subset.
// Every slot whose exact value is >= tau_q has fast >= tau_q - delta_q and is admitted; every admitted slot has an exact
// value >= tau_q - 2 delta_q.  Rows past the cell's size and tombstones never pass.  A candidate beyond the capacity of
// the query's lists is not written: the query is flagged for the exact kernel.
//
// The admission test.  `fast >= tau_q - delta_q` is not evaluated row by row.  With u = 1 / (s_q s_x), a power of two, and
// thr = fl(tau_q - delta_q):
//   euclidean      a = fma(S, 2u, -|x|^2) >= thr2,  thr2 = cell_fold_threshold(thr, |q|^2) (scan_cells.h), formed once per
//                  query by the seed kernel: the smallest float with  a >= thr2  <=>  fl(a - |q|^2) >= thr  for every a
//                  (rounding is monotone; -inf and +inf fold to themselves).  While S u is a normal number, S u and its
//                  doubling are exact, a has the bits of fl(2 fl(S u) - |x|^2), and the rows admitted are exactly those
//                  with fast >= thr.  A NaN norm (tombstone, row past the size) makes a NaN: no separate compare.
//   inner product  fma(S, u, z) >= thr with z = 0 for a live row and NaN otherwise: fl(S u) >= thr, and NaN rejects.
// Where S u is subnormal -- |S u| < 2^-126, possible only when the scales multiply to more than 2^78, i.e. the largest
// components of query and codebook multiply to less than 2^-54 -- fl(S u) rounds and the fma does not: a is then the
// rounding of the exact 2 S u - |x|^2, the old value that of a number up to 2^-149 away from it, and the two can differ
// in the last bit.  The containment above is argued for the tested value: it is the line `the two subtractions` with
// one rounding less before them, so exact >= tau_q still implies admitted; the stored key of an admitted row is
// formed in the order given under Arithmetic and may then differ from the tested value by 2^-148 at most, against
// delta_q >= 2^-17 B^2 >= 2^-97 (|q| >= 2^-40): the second statement (exact >= tau_q - 2 delta_q) keeps its slack of 1.25.
// Only the rows that passed form `fast` (mul, add, two subtractions, the key image): the stored bits are what they were.
//
// Staging.  A row's compare leaves the answers of the 64 lanes in a scalar register pair; all 16 compares of a tile are
// issued first, and the walk over the rows tests the pairs with scalar instructions: a row nobody admitted costs its fma
// and compare and nothing else.  A row somebody admitted is staged under its mask as exec: one 8-byte LDS store into the
// lane's segment, fill + 1.  Before it, if any admitting lane's segment is full (one scalar AND of the row's mask with
// the ballot of fill >= depth), the wave flushes: one counter update per lane that holds entries, its entries copied
// to the query's lists up to the capacity, the flag set beyond it -- the rule as before; the flush no longer carries
// rows of the tile at hand in registers.
// (Measured on the headline batch, profiles/cell_epilogue_bench.json: 427 us before; one-fma test, metric as a template
// parameter and the mask walk, 366 us; the fold moved from the block prologue to the seed kernel and the compares
// batched ahead of the walk with the staging blocks out of line, 340 us.  Not built: the codebook as two planes of
// dwords -- hipcc pairs the two reads into ds_read2st64_b32, the operand moves stay and the half-rate dword reads cost
// 30 us, tools/experiments/cell_planes.patch --; the gathers of the next k-step issued ahead of a k-step's products,
// 335 us against 340 and one register over the budget without the slot norms; twelve waves per workgroup, which now fit
// 168 registers without a spill: 321-331 us, 0.65 % of the step, under five times the step's run-to-run spread.)
//
// The threshold from group maxima (the threshold form: launch_cell_threshold; the gate: scan.hip, cell_threshold_form).
// The seeded form pays the query-major scan for ONE number per query -- tau_q, a lower bound on the k-th best value --
// and for k seeds.  A bound needs no selection.  Pass A is cell_cand_kernel<.., MAXIMA> over the pairs (q, p), p < T =
// kCellThrProbes: the same staging, tile loop, loads and MFMAs; lane (query column, half) holds 16 rows of its query's
// column per tile and keeps, per group of G = kCellThrGroup of them, the MAXIMUM of their tested values.
//   The tested value against the stored value.  Of a row r the lane forms a_r = fma(S_r, um, -|x_r|^2) (euclidean; inner
//   product: fma(S_r, u, z_r)) -- the operand of the admission test, see `The admission test`; t_r = fl(a_r - |q|^2)
//   (inner product: a_r) is the TESTED value, the one that statement's containment is argued for: |t_r - exact_r| <=
//   delta_q for every live row, and t_r is NaN for a row past the size or a tombstone.  What is stored for a group g is
//   f2key(fl(max_{r in g} a_r - |q|^2)): rounding is monotone, so this is max_{r in g} t_r -- the tested value of the
//   group's best row, not a new quantity with an error of its own.  The maximum is taken with fmaxf from -inf: a NaN
//   never wins, and -inf comes out exactly when the group has no live row (a_r is finite for a live row: |S| < 2^36,
//   norms <= 3e38 / 4); such a group stores the key image 0, which no search over key images counts.
//   Why M_k bounds.  Groups are disjoint sets of rows of the multiset the reference scans (a probe listed twice, not in
//   a row, is scanned twice by the reference too, and its rows are two entries of that multiset in both).  Let M_k be
//   the k-th largest stored maximum of a query.  k groups have a maximum >= M_k, so k DISTINCT entries have t >= M_k,
//   hence exact >= M_k - delta_q: the exact k-th best value E_k over ALL listed probes is >= M_k - delta_q.
//   Why M_k - 2 delta_q admits every member, ties included.  Pass B admits a row when t >= thr = fl(M_k - 2 delta_q)
//   (tested as a >= cell_fold_threshold(thr, |q|^2)).  A member of the exact top-k -- any entry with exact >= E_k, so
//   every entry tied at the k-th place -- has t >= exact - delta_q >= E_k - delta_q >= M_k - 2 delta_q.  delta_q is
//   1.25 x the sum of the error terms, so the two uses of it leave 0.4 delta_q >= 2^-19 B^2 of slack, against one more
//   rounding of a number below 4 B^2 in thr (2^-22 B^2, the line `the two subtractions`); 2 delta_q is ws_delta, exact.
//   Stage 5 then works as in the seeded form, without seed chunks: F_k over the candidates' stored keys, the cut at F_k -
//   2 delta_q, all survivors evaluated exactly by the finish kernel's ascending-j chain -- the same bits.
//   Why dropped maxima, repeated probes and -inf are harmless.  A subset of the maxima has a k-th largest element that is
//   no larger: M_k only moves down, the bound stays a bound and more is admitted.  So entries at or beyond the capacity
//   of the query's key area are simply not written (the lane reserves its tiles x 16 / G entries with one returning
//   atomic before the tile loop, and cnt[q] counts them all; cell_kth_kernel reads min(cnt, capacity) of them -- every one
//   of those positions was written, since a lane stores to each position it reserved below the capacity).  Repeated
//   probes: above.  Fewer than k maxima: M_k = -inf, thr = -inf, pass B admits every live row; what does not fit flags the
//   query for the exact kernel, as -inf does in the seeded form.
//   The list is the query's own key area (chunks x 64 entries of ws_vals), unused until pass B, filled from its END
//   downwards: entry e of the list is position capacity - 1 - e.  Pass B appends from position 0 upwards, so what it does
//   not reach of the maxima is still there after the call, with cell_kth_kernel's count of them (n_max) -- which is what
//   the diagnostics and the float64 test of pass A read from a kept workspace.  Pass A writes KEYS only;
//   the seed kernel has written the pad index into every entry of the index area, pass B writes key and index of each
//   entry it appends from position 0 on, and the finish kernel zeroes the key of every entry whose index is pad: stage 5
//   never sees a maximum.  The two candidate launches draw their blocks from two counters (params + 8, + 9).
// (Measured on the headline batch: profiles/cell_threshold_bench.json.)
//
// The single-product key (CellArgs::products == 1: the threshold form at ds = 2 with tpq_ivfpq_scan_use_cell_single_product
// on, both passes, always together; cell_cand_kernel<.., PRODUCTS = 1>).  The candidate launches produce a selection key
// only -- every returned value is the finish kernel's --, so the result depends on the key's error being inside a proven
// band, not on its size.  S1 = sum over the k-steps of xh qh: ONE MFMA per k-step, the A operand four dword gathers from
// the hi plane of the book (64 KiB at ds = 2, [j][c] -> h0 h1) straight into its register quad, the B operand the hi half
// of qsplit.  The kept |x|^2 (still from both pieces), |q|^2, the fold, the one-fma test and the group maxima are as above.
// Against g, with the notation of `Arithmetic`, N = D MFMA terms, per sub-quantizer j: XH_j = max_c |xh_jc|, XL_j =
// max_c |xl_jc| over the scaled, split codebook, qh_j, ql_j the query's pieces:
//   dropped products                    |xh.ql + xl.qh + xl.ql| <= sum_j (XH_j |ql_j| + XL_j |qh_j| + XL_j |ql_j|)
//                                       (Cauchy-Schwarz per sub-quantizer) -> x 2 / (s_q s_x) in value units: the QUERY'S
//                                       OWN TERM, evaluated by cell_seed_kernel, upwards (x 1.0001)
//   piece residues                      |rq.x' + (qh + ql).rx| <= 2.03 2^-22 Q X + 1.01 eta sqrt(D) (Q + X)
//   fp32 accumulation, any order        1.003 N 2^-23 Q X, N = D
//     -> (2.03 2^-22 + 1.003 N 2^-23) B^2 / 2  +  1.01 sqrt(D) 2^-26 B^2
//   the norm chains, |x|^2 from the pieces, the two subtractions, the exact chain's own rounding: as under `Arithmetic`
// delta1_q = 1.25 x (the query's own term + the other lines' sum x B^2) -- cell_delta1_rel is 1.25 x that sum, and the seed
// kernel applies 1.25 to its term.  ws_delta = 2 delta1_q and thr = M_k - 2 delta1_q in both passes, so `Why M_k bounds`
// and `Why M_k - 2 delta_q admits every member` hold word for word with delta1_q for delta_q; the inner product's errors
// are a subset (its term is taken with the same factor 2).
// XH_j and XL_j depend on the index alone: cell_prep_kernel computes them behind its four numbers and leaves them in the
// 256-byte parameter block -- of the workspace, or of the kept state -- from byte kCellPieceMaxAt on, per PAIR of
// sub-quantizers (the larger of the two, 32 + 32 numbers) as the upper 16 bits of an fp32 rounded up: a pair's maximum
// bounds either member, rounding up only loosens.  The first 16 bytes, the counters at ints 8 and 9, the image, the norms
// and cell_kept_bytes are what they were.
// The band is 3.35 x that of three products on the headline's SIFT-like index (2 delta: 2 309 against 689 value units) and
// 5.8 x on Gaussian codebooks, whose largest entry per sub-quantizer is far from the typical one: 11 % more candidates on
// the headline (253 against 227 per query).  More rows then survive the finish kernel's cut at F_k - 2 delta1_q, and its
// exact list is sized for that: cell_single_finish_regs (scan_host.h) -- 256 entries instead of 128 at k = 100; with 128
// a batch of the existing tests (7 probes, k = 100, inner product) had 20 of 1 025 queries redone exactly.
// ds = 1 stays on three products: its single-product form (2-byte entries, pairs packed into the operand) was not built
// or measured.  The seeded form, tpq_ivfpq_cell_candidates and the query-major routes keep three products.
// (Measured on the headline batch, profiles/cell_single_product_bench.json: the candidates proper 416 -> 294 us, pass A
// 132 -> 141 us, the finish kernel 115 -> 139 us, the scan's kernels together 741 -> 652-657 us, the step 0.821 -> 0.741
// ms; twelve waves per workgroup (126 registers, no spill) against eight and sixteen: 0.732 / 0.754 / 0.750 ms.)
//
// The kept state (tpq_ivfpq_search_fused_cells_kept; CellArgs::kparams, book, norm; cell_use_kept, scan_cells.h).  Three
// things a call of the form with slot norms computes are functions of the codebook, the codes and the tombstones alone --
// no query enters: cell_prep_kernel's four numbers, the split fp16 codebook every candidate workgroup (and the norm
// kernel) derives from the fp32 one before its first tile, and cell_norm_kernel's norms.  An index is searched many times
// between two changes, so a caller that owns the index may own them too: a device buffer of cell_kept_bytes(n_slots, ds),
//   [256 bytes: max |entry|, X^2, scalable, s_x][the codebook image: [j][c] -> DS hi pieces, DS lo pieces, what
//   CellBook<DS> holds in LDS][an fp32 norm per slot ADDRESS in [0, n_slots), NaN for a tombstone]
// The norms cover every address, not the listed cells: the chain of a slot reads that slot's 64 code bytes and its
// tombstone byte only, so no cell structure is needed, and the bytes of a slot outside any cell decode to some value
// that nobody reads.  Per slot the chain, and so the bits, are cell_norm_kernel's (the same kernel, ALL).
//   kept_valid == 0   the call writes the state first, on its stream: cell_prep_kernel (into the state), cell_book_kernel
//                     (the image, book_entry -- the one definition the per-call staging uses too), cell_norm_kernel<DS,
//                     true>; then it runs as below.  The caller then hands the state to later calls as valid, for as long
//                     as codes, codebook and tombstones are what they were, and orders other streams behind this call.
//   kept_valid == 1   neither cell_prep_kernel nor cell_norm_kernel is launched; the candidate kernels copy the image into
//                     LDS with 16-byte loads instead of converting 16 384 entries per workgroup; the seed kernel reads
//                     `scalable` and X^2, the candidate kernels s_x, through kparams.  The zeroing cell_prep_kernel used
//                     to do is the seed kernel's, so no single-block launch is left.
// The block counters and everything per call stay in the workspace, whose size and layout are what they were (its norm
// region is simply unused).  Only a call that takes the form WITH slot norms (scan.hip: cell_major_norms, either form)
// uses a state; every other call ignores the pointer and writes nothing to it.  Same bits on every path: the state holds
// exactly what the per-call kernels would have produced.
#include <atomic>
#include <cmath>

#include "mfma_util.h"
#include "scan_cells.h"
#include "scan_fk.h"
#include "wave_topk.h"

namespace tpq {

float cell_delta_rel(int ds) {
  const double D = 64.0 * ds, N = 3.0 * D, u = 1.0 / 16777216.0;  // u = 2^-24
  const double sum = 0.5 * (3.03 * 4 * u + 1.003 * N * 2 * u) + 1.01 * std::sqrt(D) * u / 4 + (D + 1) * u + 14 * u + 4 * u +
                     1.001 * (64 + ds + 2) * u;
  return (float)(1.25 * sum * (1.0 + 1.0 / 1024));  // (+ 2^-10: B^2 and the product are evaluated in fp32)
}

// `The single-product key`: every line of the budget but the dropped products, which are the query's own term
float cell_delta1_rel(int ds) {
  const double D = 64.0 * ds, N = D, u = 1.0 / 16777216.0;  // u = 2^-24
  const double sum = 0.5 * (2.03 * 4 * u + 1.003 * N * 2 * u) + 1.01 * std::sqrt(D) * u / 4 + (D + 1) * u + 14 * u + 4 * u +
                     1.001 * (64 + ds + 2) * u;
  return (float)(1.25 * sum * (1.0 + 1.0 / 1024));
}

void cell_fill_extras(CellArgs& a, void* at, size_t room, int layout_p0) {
  char* p = reinterpret_cast<char*>(at);
  const int p0 = layout_p0 >= 0 ? layout_p0 : a.p0;
  const size_t extras = cell_extra_bytes(a.nq, a.max_nprobe, a.n_cells, p0);
  a.norm = room >= extras && room - extras >= cell_norm_bytes(a.n_slots) ? reinterpret_cast<float*>(p + extras) : nullptr;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += cell_align(bytes);
    return r;
  };
  const int np = a.max_nprobe > p0 ? a.max_nprobe - p0 : 0;
  a.params = reinterpret_cast<float*>(take(256));
  a.thr = reinterpret_cast<float*>(take((size_t)a.nq * 4));
  a.qscale = reinterpret_cast<float*>(take((size_t)a.nq * 4));
  a.qnorm = reinterpret_cast<float*>(take((size_t)a.nq * 4));
  a.cnt = reinterpret_cast<int*>(take((size_t)a.nq * 4));
  a.hist = reinterpret_cast<int*>(take((size_t)a.n_cells * 4));
  a.cell_off = reinterpret_cast<int*>(take(((size_t)a.n_cells + 1) * 4));
  a.blk_off = reinterpret_cast<int*>(take(((size_t)a.n_cells + 1) * 4));
  a.cell_st = reinterpret_cast<int*>(take((size_t)a.n_cells * 4));
  a.cell_sz = reinterpret_cast<int*>(take((size_t)a.n_cells * 4));
  a.pairs = reinterpret_cast<int*>(take((size_t)a.nq * np * 4));
  a.qsplit = reinterpret_cast<_Float16*>(take((size_t)a.nq * kCellQSplit * 2));
  a.kparams = a.params;  // (no kept state: cell_use_kept, scan_cells.h, points these elsewhere)
  a.book = nullptr;
  a.kept_build = 0;
}

constexpr int kCellScaleExp = 12;   // the largest scaled component lies in [2^12, 2^13)
constexpr int kCellMaxExp = 40;     // data whose largest component is outside 2^+-40 goes to the exact kernel
constexpr unsigned kMaxFiniteBits = 0x7f7fffffu;

// 2^e, |e| <= 126
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }
__device__ __forceinline__ int exp_of_bits(unsigned bits) { return (int)((bits >> 23) & 255u) - 127; }

// a wave's share of the codebook's maxima: sub-quantizers wave, wave + 16, ...; per sub-quantizer the largest |c_jc|^2 into
// c2max_s[j], and the largest |entry| bits of all it read.  DS is a constant so that the thread's 16 DS loads are issued
// together, ahead of the arithmetic: with the length read from the arguments they went out one by one, each waited for
// where it was issued, and the one block took 17 us over 128 KiB (profiles/cell_pieces_bench.json).  The chains and the
// maxima are what they were: fma over e ascending per entry, maxima of non-negative numbers in any order
template <int DS>
__device__ __forceinline__ unsigned prep_maxima(const float* __restrict__ codebook, int lane, int wave, float* c2max_s) {
  float y[4][4][DS];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
#pragma unroll
      for (int e = 0; e < DS; ++e) y[jj][cc][e] = codebook[((wave + 16 * jj) * DS + e) * 256 + lane + 64 * cc];
  unsigned mb = 0u;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    float c2m = 0.f;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      float c2 = 0.f;
#pragma unroll
      for (int e = 0; e < DS; ++e) {
        const unsigned b = __float_as_uint(y[jj][cc][e]) & 0x7fffffffu;
        mb = b > mb ? b : mb;
        c2 = fmaf(y[jj][cc][e], y[jj][cc][e], c2);
      }
      c2m = fmaxf(c2m, c2);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c2m = fmaxf(c2m, __shfl_xor(c2m, d, 64));
    if (lane == 0) c2max_s[wave + 16 * jj] = c2m;
  }
  return mb;
}

// the same share of the piece maxima (`The single-product key`): per sub-quantizer the largest |hi piece|^2 and |lo piece|^2
// of s_x c_jc over its 256 entries, the pieces as book_entry forms them
template <int DS>
__device__ __forceinline__ void prep_piece_maxima(const float* __restrict__ codebook, float sx, int lane, int wave,
                                                  float* xh2_s, float* xl2_s) {
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    float hm = 0.f, lm = 0.f;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      float h2 = 0.f, l2 = 0.f;
#pragma unroll
      for (int e = 0; e < DS; ++e) {
        const float ys = codebook[((wave + 16 * jj) * DS + e) * 256 + lane + 64 * cc] * sx;
        const _Float16 h = (_Float16)ys;
        const float hf = (float)h, lf = (float)(_Float16)(ys - hf);
        h2 = fmaf(hf, hf, h2);
        l2 = fmaf(lf, lf, l2);
      }
      hm = fmaxf(hm, h2);
      lm = fmaxf(lm, l2);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      hm = fmaxf(hm, __shfl_xor(hm, d, 64));
      lm = fmaxf(lm, __shfl_xor(lm, d, 64));
    }
    if (lane == 0) {
      xh2_s[wave + 16 * jj] = hm;
      xl2_s[wave + 16 * jj] = lm;
    }
  }
}
// a positive float's upper 16 bits, rounded UP (the value first raised past the roundings of its chain and root)
__device__ __forceinline__ unsigned short piece_max16(float sq_norm) {
  return (unsigned short)((__float_as_uint(sqrtf(sq_norm) * 1.0001f) + 0xffffu) >> 16);
}
__device__ __forceinline__ float piece_max_of(unsigned short w) { return __uint_as_float((unsigned)w << 16); }

__global__ __launch_bounds__(1024) void cell_prep_kernel(CellArgs a) {
  __shared__ unsigned maxbits_s;
  __shared__ float c2max_s[64], xh2_s[64], xl2_s[64], sx_s;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) maxbits_s = 0u;
  __syncthreads();
  // (ds is 1 or 2: the entry points of the form)
  const unsigned mb = a.ds == 1 ? prep_maxima<1>(a.codebook, lane, wave, c2max_s)
                                : prep_maxima<2>(a.codebook, lane, wave, c2max_s);
  atomicMax(&maxbits_s, mb);
  __syncthreads();
  if (tid == 0) {
    float x2 = 0.f;
    for (int j = 0; j < 64; ++j) x2 += c2max_s[j];
    x2 *= 1.0001f;  // (upwards: 64 + ds roundings of 2^-24 each)
    const unsigned bits = maxbits_s;
    const int e = exp_of_bits(bits);
    const bool ok = bits != 0u && bits <= kMaxFiniteBits && e >= -kCellMaxExp && e <= kCellMaxExp && x2 <= 3e38f;
    a.kparams[0] = __uint_as_float(bits);
    a.kparams[1] = x2;
    a.kparams[2] = ok ? 1.f : 0.f;
    a.kparams[3] = ok ? pow2i(kCellScaleExp - e) : 0.f;  // s_x
    sx_s = ok ? pow2i(kCellScaleExp - e) : 0.f;
  }
  __syncthreads();
  // the piece maxima per pair of sub-quantizers (kCellPieceMaxAt, scan_cells.h); a codebook that cannot be scaled leaves
  // numbers nobody reads: every query is flagged
  if (a.ds == 1)
    prep_piece_maxima<1>(a.codebook, sx_s, lane, wave, xh2_s, xl2_s);
  else
    prep_piece_maxima<2>(a.codebook, sx_s, lane, wave, xh2_s, xl2_s);
  __syncthreads();
  if (tid < 64) {
    const float* s = tid < 32 ? xh2_s : xl2_s;
    const int i = tid & 31;
    unsigned short* out = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(a.kparams) + kCellPieceMaxAt);
    out[tid] = piece_max16(fmaxf(s[2 * i], s[2 * i + 1]));
  }
}

// the listed probes of query q: p0 <= p < min(n_probe_list[q], p_hi) (clamped), the cell not empty and not the previous
// probe's again
struct ListedProbe {
  bool listed;
  int cell;
};
__device__ __forceinline__ int cell_n_probe(const CellArgs& a, int q) {
  const int n = (int)a.n_probe_list[q];
  return n < 0 ? 0 : (n > a.p_hi ? a.p_hi : n);
}
__device__ __forceinline__ ListedProbe listed_probe(const CellArgs& a, int q, int p) {
  const int64_t o = (int64_t)q * a.max_nprobe + p;
  const int64_t st = a.cell_start[o], sz = a.cell_size[o];
  const bool again = p > 0 && a.cell_start[o - 1] == st;
  return ListedProbe{sz > 0 && !again, (int)a.cells[o]};
}

__global__ __launch_bounds__(256) void cell_seed_kernel(CellArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  // what the call's later stages count in: the histograms of the inversion and cell_cand_kernel's block counters
  // (CellArgs::work).  Here, over the whole grid, so that a call with a kept state launches no block of its own for it
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < a.n_cells; i += (int)gridDim.x * 256) {
    a.hist[i] = 0;
    if (a.hist2) a.hist2[i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) reinterpret_cast<int*>(a.params)[8 + threadIdx.x] = 0;
  if (q >= a.nq) return;  // (wave-uniform)
  const int D = 64 * a.ds;
  const float x0 = lane < D ? a.query[(int64_t)lane * a.nq + q] : 0.f;
  const float x1 = 64 + lane < D ? a.query[(int64_t)(64 + lane) * a.nq + q] : 0.f;
  unsigned mb = __float_as_uint(x0) & 0x7fffffffu;
  const unsigned mb1 = __float_as_uint(x1) & 0x7fffffffu;
  mb = mb1 > mb ? mb1 : mb;
  float q2 = fmaf(x1, x1, x0 * x0);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)mb, d, 64);
    mb = o > mb ? o : mb;
    q2 += __shfl_xor(q2, d, 64);
  }
  const int n_probe = cell_n_probe(a, q);
  bool bad_cell = false;
  for (int p = a.p0 + lane; p < n_probe; p += 64) {
    const int64_t c = a.cells[(int64_t)q * a.max_nprobe + p];
    bad_cell = bad_cell || c < 0 || c >= (int64_t)a.n_cells;
  }
  bad_cell = __ballot(bad_cell) != 0ull;
  // (the threshold form: no threshold yet -- cell_kth_kernel writes thr[q] of every query that is not flagged here)
  const float tau = a.k > 0 ? a.seed_vals[(int64_t)q * a.k + a.k - 1] : (a.thr_k > 0 ? 0.f : a.thr_in[q]);
  const int eq = exp_of_bits(mb);
  const bool flagged = a.k > 0 && a.flags[q] == a.epoch;
  const bool scalable = a.kparams[2] != 0.f && mb != 0u && mb <= kMaxFiniteBits && eq >= -kCellMaxExp &&
                        eq <= kCellMaxExp && q2 <= 3e38f;
  const bool tau_ok = tau == tau && tau != INFINITY;  // (-inf: fewer than k seeds -- everything is admitted)
  const bool active = !flagged && scalable && tau_ok && !bad_cell;
  if (!active) {
    if (lane == 0) {
      a.flags[q] = a.epoch;
      a.cnt[q] = 0;
      a.thr[q] = INFINITY;
    }
    return;
  }
  // the pieces of s_q q: this lane's two components
  const float sq = pow2i(kCellScaleExp - eq);
  const float y0 = x0 * sq, y1 = x1 * sq;
  const _Float16 h0 = (_Float16)y0, h1 = (_Float16)y1;
  const _Float16 l0 = (_Float16)(y0 - (float)h0), l1 = (_Float16)(y1 - (float)h1);
  const float B = sqrtf(q2) * 1.000001f + sqrtf(a.kparams[1]) * 1.000001f;
  float delta = a.rel * (B * B);
  if (a.products == 1) {
    // the single-product key: the dropped products, bounded per sub-quantizer from cell_prep_kernel's piece maxima (per
    // pair of sub-quantizers) and the norms of this query's pieces per sub-quantizer -- component i belongs to
    // sub-quantizer i / ds, a lane's neighbour holds the other component at ds = 2 --, in value units, upwards
    const unsigned short* pm =
        reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(a.kparams) + kCellPieceMaxAt);
    auto subq_norm = [&](_Float16 v) {
      float s = (float)v * (float)v;
      if (a.ds == 2) s += __shfl_xor(s, 1, 64);
      return sqrtf(s) * 1.000001f;
    };
    const float nh0 = subq_norm(h0), nl0 = subq_norm(l0), nh1 = subq_norm(h1), nl1 = subq_norm(l1);
    const int i0 = lane / (2 * a.ds), i1 = a.ds == 2 ? 16 + (lane >> 2) : 0;  // (ds = 1: the second component is 0)
    float t = fmaf(piece_max_of(pm[i0]), nl0, piece_max_of(pm[32 + i0]) * (nh0 + nl0)) +
              fmaf(piece_max_of(pm[i1]), nl1, piece_max_of(pm[32 + i1]) * (nh1 + nl1));
    if (a.ds == 2 && (lane & 1)) t = 0.f;  // (one lane per sub-quantizer)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d, 64);
    delta = fmaf(1.25f * 1.0001f * t, 2.f / (sq * a.kparams[3]), delta);
  }
  if (lane == 0) {
    // the candidate kernel's threshold: a row passes when fl(a - |q|^2) >= tau - delta, tested as a >= the fold
    if (a.thr_k == 0) a.thr[q] = a.euclid ? cell_fold_threshold(tau - delta, q2) : tau - delta;
    a.ws_delta[q] = 2.f * delta;
    a.qscale[q] = pow2i(kCellScaleExp - eq);
    a.qnorm[q] = q2;
    a.cnt[q] = 0;
    if (a.k == 0) a.flags[q] = 0;
  }
  if (a.list_evict && lane < a.chunks) a.list_evict[(int64_t)q * a.chunks + lane] = 0;
  {
    // the pieces of s_q q, component-major per query: the candidate kernel's B operand is 16 contiguous bytes of it
    _Float16* qs = a.qsplit + (int64_t)q * kCellQSplit;
    if (lane < D) {
      qs[lane] = h0;
      qs[128 + lane] = l0;
    }
    if (64 + lane < D) {
      qs[64 + lane] = h1;
      qs[192 + lane] = l1;
    }
  }
  const int64_t base = (int64_t)q * a.chunks * 64;
  const int seed_chunks = (a.k + 63) / 64;
  for (int t = 0; t < a.chunks; ++t) {
    const int e = t * 64 + lane;
    Key key = pad_key();
    if (e < a.k) {
      const int64_t ad = a.seed_addr[(int64_t)q * a.k + e];
      if (ad >= 0) key = make_key(a.seed_vals[(int64_t)q * a.k + e], (int)ad);
    }
    if (t < seed_chunks) a.keys[base + e] = key.hi;
    a.idx[base + e] = key.lo;
  }
}

// The inversion's walk: the listed pairs of the slice of kCellSlice consecutive queries from q0, flattened over the
// workgroup -- pair i is (q0 + i / np, p0 + i % np), so the rows of cells, cell_start and cell_size are read coalesced.
// A query the seed kernel flagged lists nothing; every other query's cells lie in [0, n_cells) (the seed kernel's check).
constexpr int kCellSliceThreads = 1024;
template <class F>
__device__ __forceinline__ void for_slice_pairs(const CellArgs& a, int q0, F&& f) {
  const int np = a.p_hi - a.p0;  // (> 0: the launch)
  const int nqs = a.nq - q0 < kCellSlice ? a.nq - q0 : kCellSlice;
  for (int i = (int)threadIdx.x; i < nqs * np; i += kCellSliceThreads) {
    const int dq = i / np;
    const int q = q0 + dq, p = a.p0 + (i - dq * np);
    if (p >= cell_n_probe(a, q) || a.flags[q] == a.epoch) continue;
    const ListedProbe lp = listed_probe(a, q, p);
    if (lp.listed) f(q, p, lp.cell);
  }
}
// the slice's pairs per cell, in the workgroup's LDS histogram (n_cells ints, n_cells <= kCellLdsCells).
// TWO: the threshold form's one walk -- a second histogram behind the first counts the pairs with p < a.p_a, pass A's
// (2 n_cells ints, n_cells <= kCellLdsCells / 2)
template <bool TWO>
__device__ __forceinline__ void count_slice(const CellArgs& a, int q0, int* cell_h) {
  for (int c = (int)threadIdx.x; c < (TWO ? 2 : 1) * a.n_cells; c += kCellSliceThreads) cell_h[c] = 0;
  __syncthreads();
  for_slice_pairs(a, q0, [&](int, int p, int c) {
    atomicAdd(&cell_h[c], 1);
    if (TWO && p < a.p_a) atomicAdd(&cell_h[a.n_cells + c], 1);
  });
  __syncthreads();
}

template <bool TWO>
__global__ __launch_bounds__(kCellSliceThreads) void cell_count_kernel(CellArgs a) {
  extern __shared__ int cell_h[];
  count_slice<TWO>(a, (int)blockIdx.x * kCellSlice, cell_h);
  for (int c = (int)threadIdx.x; c < a.n_cells; c += kCellSliceThreads) {
    const int h = cell_h[c];
    if (h) atomicAdd(&a.hist[c], h);
    if constexpr (TWO) {
      const int ha = cell_h[a.n_cells + c];
      if (ha) atomicAdd(&a.hist2[c], ha);
    }
  }
}

// n_cells > kCellLdsCells: one wave per query, one global atomic per listed pair
__global__ __launch_bounds__(256) void cell_count_wide_kernel(CellArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (q >= a.nq) return;
  if (a.flags[q] == a.epoch) return;
  const int n_probe = cell_n_probe(a, q);
  for (int p = a.p0 + lane; p < n_probe; p += 64) {
    const ListedProbe lp = listed_probe(a, q, p);
    if (lp.listed) atomicAdd(&a.hist[lp.cell], 1);
  }
}

// (the one walk: a second block does the same for pass A's view)
__global__ __launch_bounds__(1024) void cell_scan_kernel(CellArgs a) {
  __shared__ int sp[2][1024], sb[2][1024];
  const int tid = (int)threadIdx.x;
  if (blockIdx.x == 1) {
    a.hist = a.va.hist;
    a.cell_off = a.va.cell_off;
    a.blk_off = a.va.blk_off;
  }
  const int per = (a.n_cells + 1023) / 1024;
  const int lo = tid * per < a.n_cells ? tid * per : a.n_cells;
  const int hi = lo + per < a.n_cells ? lo + per : a.n_cells;
  int np = 0, nb = 0;
  for (int c = lo; c < hi; ++c) {
    const int h = a.hist[c];
    np += h;
    nb += (h + kCellGroup - 1) / kCellGroup;
  }
  sp[0][tid] = np;
  sb[0][tid] = nb;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan, double-buffered
    const int vp = sp[cur][tid] + (tid >= d ? sp[cur][tid - d] : 0);
    const int vb = sb[cur][tid] + (tid >= d ? sb[cur][tid - d] : 0);
    sp[cur ^ 1][tid] = vp;
    sb[cur ^ 1][tid] = vb;
    cur ^= 1;
    __syncthreads();
  }
  int op = sp[cur][tid] - np, ob = sb[cur][tid] - nb;  // exclusive
  for (int c = lo; c < hi; ++c) {
    const int h = a.hist[c];
    a.cell_off[c] = op;
    a.blk_off[c] = ob;
    a.hist[c] = op;  // the scatter's cursor
    op += h;
    ob += (h + kCellGroup - 1) / kCellGroup;
  }
  if (tid == 1023) {
    a.cell_off[a.n_cells] = sp[cur][1023];
    a.blk_off[a.n_cells] = sb[cur][1023];
  }
}

// the pair that takes a cell's first position writes the cell's extent (every query lists it with the same)
__device__ __forceinline__ void place_pair(const CellArgs& a, const CellView& v, int q, int p, int c, int pos) {
  v.pairs[pos] = q;
  if (pos == v.cell_off[c]) {
    const int64_t o = (int64_t)q * a.max_nprobe + p;
    v.cell_st[c] = (int)a.cell_start[o];
    v.cell_sz[c] = (int)a.cell_size[o];
  }
}

template <bool TWO>
__global__ __launch_bounds__(kCellSliceThreads) void cell_scatter_kernel(CellArgs a) {
  extern __shared__ int cell_h[];
  const int q0 = (int)blockIdx.x * kCellSlice;
  count_slice<TWO>(a, q0, cell_h);
  // one returning atomic per cell the slice lists: its h consecutive positions, the first of them left in LDS
  for (int c = (int)threadIdx.x; c < a.n_cells; c += kCellSliceThreads) {
    const int h = cell_h[c];
    if (h) cell_h[c] = atomicAdd(&a.hist[c], h);
    if constexpr (TWO) {
      const int ha = cell_h[a.n_cells + c];
      if (ha) cell_h[a.n_cells + c] = atomicAdd(&a.hist2[c], ha);
    }
  }
  __syncthreads();
  for_slice_pairs(a, q0, [&](int q, int p, int c) {
    place_pair(a, cell_view(a), q, p, c, atomicAdd(&cell_h[c], 1));
    if (TWO && p < a.p_a) place_pair(a, a.va, q, p, c, atomicAdd(&cell_h[a.n_cells + c], 1));  // (pass A's view)
  });
}

__global__ __launch_bounds__(256) void cell_scatter_wide_kernel(CellArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (q >= a.nq) return;
  if (a.flags[q] == a.epoch) return;
  const int n_probe = cell_n_probe(a, q);
  for (int p = a.p0 + lane; p < n_probe; p += 64) {
    const ListedProbe lp = listed_probe(a, q, p);
    if (lp.listed) place_pair(a, cell_view(a), q, p, lp.cell, atomicAdd(&a.hist[lp.cell], 1));
  }
}

// A candidate workgroup's LDS: the split codebook, per wave the 32 row norms of its tile, and per wave a staging area for
// admitted rows -- kDepth entries of 8 bytes per lane, entry-major ([entry][lane]: a wave's store of one entry level is
// contiguous).  kDepth is what the CU's 160 KiB leave behind the ds = 2 book, for either ds: 7 at eight waves.
#ifndef TPQ_CELL_WAVES
#define TPQ_CELL_WAVES 8  // (variant builds: the A/B of 12)
#endif
constexpr int kCellWaves = TPQ_CELL_WAVES;
// the single-product kernels (`The single-product key`): half the book and fewer registers leave room for more waves
#ifndef TPQ_CELL_WAVES1
#define TPQ_CELL_WAVES1 12  // (variant builds: the A/B of 8, 12 and 16 -- profiles/cell_single_product_bench.json)
#endif
constexpr int kCellWaves1 = TPQ_CELL_WAVES1;
constexpr int cell_waves(int products) { return products == 1 ? kCellWaves1 : kCellWaves; }
constexpr size_t kCellLdsBytes = 160 * 1024;
// PRODUCTS = 1: the hi plane alone, [j][c] -> DS hi pieces (ds = 2: 64 KiB), and the staging depth from what that leaves
template <int DS, int PRODUCTS = 3>
struct CellBook {
  static constexpr int KS = 4 * DS;                            // MFMA k-steps of 16 components
  static constexpr size_t kBook = (size_t)64 * 256 * (PRODUCTS == 1 ? 2 : 4) * DS;  // [j][c] -> DS hi pieces, DS lo pieces
  static constexpr int kWaves = cell_waves(PRODUCTS);
  static constexpr int kThreads = 64 * kWaves;
  static constexpr size_t kNorms = (size_t)kWaves * 32 * 4;    // per wave: |x|^2 of the tile's 32 rows (NaN: not live)
  static constexpr int kDepth = (int)((kCellLdsBytes - (PRODUCTS == 1 ? kBook : (size_t)64 * 256 * 8) - kNorms) /
                                      ((size_t)kWaves * 64 * 8));
  static constexpr size_t kBytes = kBook + kNorms + (size_t)kWaves * 64 * kDepth * 8;
  static_assert(kDepth >= 1 && kBytes <= kCellLdsBytes, "the staging area does not fit the CU's LDS");
};

__device__ __forceinline__ unsigned pack_f16x2(_Float16 lo, _Float16 hi) {
  return (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
}
__device__ __forceinline__ float f16_lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float f16_hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }

// The split codebook as a candidate workgroup keeps it in LDS: entry (j, c) -> the fp16 pieces of s_x c_jc.  DS = 2:
// two dwords (h0 h1, l0 l1); DS = 1: one (h l).  One definition for the per-call staging and the kept image
template <int DS>
__device__ __forceinline__ void book_entry(const float* __restrict__ codebook, float sx, int i, unsigned* book) {
  const int j = i >> 8, c = i & 255;
  _Float16 h[DS], l[DS];
#pragma unroll
  for (int e = 0; e < DS; ++e) {
    const float ys = codebook[(j * DS + e) * 256 + c] * sx;
    h[e] = (_Float16)ys;
    l[e] = (_Float16)(ys - (float)h[e]);
  }
  if constexpr (DS == 2) {
    book[2 * i] = pack_f16x2(h[0], h[1]);
    book[2 * i + 1] = pack_f16x2(l[0], l[1]);
  } else {
    book[i] = pack_f16x2(h[0], l[0]);
  }
}
// the kept state's codebook image: a.book in global memory, what book_entry leaves in LDS
template <int DS>
__global__ __launch_bounds__(256) void cell_book_kernel(CellArgs a) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);  // (the launch: 64 blocks, one thread per entry)
  book_entry<DS>(a.codebook, a.kparams[3], i, a.book);
}

// The slot norms of a call: norm[slot] = |x'|^2 / s_x^2 of every slot of a listed cell, NaN for a tombstone -- the value
// cell_cand_kernel<DS, false> forms per (cell, block) in its tile loop, here once per slot, with the same bits: per half
// (components [16 s + 8 half, + 8), s ascending) the chain x2 = fma(v, v, x2) over v = fp32(hi piece) + fp32(lo piece),
// then half 0 + half 1, then x inv_sx2.  The sums v do not depend on the slot, so the staging forms them once per entry:
// the book in LDS is [j][c] -> DS fp32 sums (128 KiB at ds = 2).  One workgroup per CU at most, cells dealt round robin,
// a thread per slot: its 16 code dwords are coalesced over the slots of the cell.
// ALL: the kept state's norms -- every slot address in [0, n_slots), no cell structure: the bytes of a slot outside any
// cell decode to some value nobody reads.  The same chain per slot, so the same bits for every slot of a cell.
template <int DS, bool ALL = false>
__global__ __launch_bounds__(512) void cell_norm_kernel(CellArgs a) {
  constexpr int KS = 4 * DS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sums = reinterpret_cast<float*>(smem);  // [j][c][DS]
  const int tid = (int)threadIdx.x;
  const float sx = a.kparams[3];
  const float inv_sx = 1.f / sx;
  const float inv_sx2 = inv_sx * inv_sx;
  for (int i = tid; i < 64 * 256; i += 512) {  // entry (j, c)
    const int j = i >> 8, c = i & 255;
#pragma unroll
    for (int e = 0; e < DS; ++e) {
      const float ys = a.codebook[(j * DS + e) * 256 + c] * sx;
      const _Float16 h = (_Float16)ys;
      const _Float16 l = (_Float16)(ys - (float)h);
      sums[i * DS + e] = (float)h + (float)l;
    }
  }
  __syncthreads();
  // ALL: one round of "cells" of 512 consecutive slot addresses per workgroup, n_slots < 2^31 (the entry points)
  const int n_units = ALL ? (int)((a.n_slots + 511) / 512) : a.n_cells;
  for (int c = (int)blockIdx.x; c < n_units; c += (int)gridDim.x) {
    int64_t st;
    int sz;
    if constexpr (ALL) {
      st = (int64_t)c * 512;
      sz = a.n_slots - st < 512 ? (int)(a.n_slots - st) : 512;
    } else {
      if (a.cell_off[c + 1] == a.cell_off[c]) continue;  // not listed: its extent was never written
      st = a.cell_st[c];
      sz = a.cell_sz[c];
      if (st < 0 || sz < 0 || st + sz > a.n_slots) sz = 0;  // (the candidate kernel's check)
    }
    for (int r = tid; r < sz; r += 512) {
      const int64_t slot = st + r;
      const uint32_t* __restrict__ cw = reinterpret_cast<const uint32_t*>(a.codes) + slot;
      uint32_t w[16];  // dword g: the codes of sub-quantizers [4 g, + 4)
#pragma unroll
      for (int g = 0; g < 16; ++g) w[g] = cw[(int64_t)g * a.n_slots];
      const bool empty = a.is_empty && a.is_empty[slot];
      float x2h[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float x2 = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
          for (int bb = 0; bb < 8 / DS; ++bb) {
            const int j = (16 * s + 8 * half) / DS + bb;
            const int code = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
            if constexpr (DS == 2) {
              const float2 v = reinterpret_cast<const float2*>(sums)[j * 256 + code];
              x2 = fmaf(v.x, v.x, x2);
              x2 = fmaf(v.y, v.y, x2);
            } else {
              const float v = sums[j * 256 + code];
              x2 = fmaf(v, v, x2);
            }
          }
        }
        x2h[half] = x2;
      }
      a.norm[slot] = empty ? __builtin_nanf("") : (x2h[0] + x2h[1]) * inv_sx2;
    }
  }
}

// One workgroup of eight waves per CU stages the split codebook once; every WAVE then takes blocks -- (cell, group of
// <= 32 listed queries) -- from a counter (cell_prep_kernel zeroes it) and never meets the others again.  Per tile of 32
// slots, lane (row, half) loads the 8 code dwords that hold its half of every k-step and gathers its A operand -- the
// pieces of 8 components -- straight from the codebook in LDS: no staged tile, no barrier.
// NORMS: the norm of a row is cell_norm_kernel's (a.norm, loaded with the codes, NaN for a row that is not live) instead
// of the chain over the gathered pieces; the same bits either way.
//
// The tile loop's pipeline.  The loads of tile i + 1 -- 8 code dwords and the norm (NORMS) or the tombstone byte -- are
// issued at the head of tile i's body, unconditionally and straight-line: a row at or past the cell's size reads the
// cell's last row (in range: the extent was checked, and a.norm is written for the whole of a listed cell), the last tile
// prefetches that row again, and rv / the tombstone are applied to the loaded values as selects.  (A load under `rv ? :`
// is a branch around the load to hipcc, and a full vmcnt(0) behind it: the loads were issued a tile ahead and waited for
// at once.)  The loop head waits for tile i's own dwords -- the previous prefetch -- BEFORE the new loads go out, and no
// wait on the new loads stands between their issue and the tile's last MFMA.  A block with nothing to read (extent
// rejected) is skipped before any load.
// Admitted rows do not go to the query's list from the loop: a returning atomic there is a second exposed round trip per
// tile, and its vmcnt(0) drains the prefetch.  Lane (query column, half) appends (f2key(fast), ~address) to its private
// segment of the wave's staging area.  The wave flushes at the end of its block, and before a ROW that some admitting
// lane's segment cannot take (the row's mask AND one ballot, scalar): a flush is ONE counter update per lane that holds
// entries, followed by the capacity rule as before (entries at or beyond cap are not written, the query is flagged, cnt
// counts them all).  EUCLID: the metric, so that the tile loop selects nothing on it (the header: `The admission test`).
// MAXIMA: pass A of the threshold form (the header: `The threshold from group maxima`).  Nothing is tested or staged:
// the lane reserves tiles x 16 / kCellThrGroup entries of its query's key area with ONE returning atomic before the tile
// loop and stores, per tile, the key image of the largest tested value of every group of kCellThrGroup of its 16 rows --
// 0, which counts for nothing in a search over key images, for a group without a live row.  Entries at or beyond the
// capacity are dropped.  NORMS only: the form requires the norm array.
// PRODUCTS = 1: `The single-product key` -- the hi plane of the book alone in LDS (one dword per entry at ds = 2), a
// k-step's four entries gathered straight into the A operand's register quad, one MFMA per k-step against the hi half
// of the split query.  NORMS only, ds = 2 only (ds = 1 stays on three products); everything behind the MFMAs as it was.
template <int DS, bool NORMS, bool EUCLID, bool MAXIMA = false, int PRODUCTS = 3>
__global__ __launch_bounds__(64 * cell_waves(PRODUCTS)) void cell_cand_kernel(CellArgs a) {
  static_assert(!MAXIMA || NORMS, "pass A reads the slot norms");
  static_assert(PRODUCTS == 3 || (PRODUCTS == 1 && DS == 2 && NORMS), "the single-product key: ds = 2 with slot norms");
  using T = CellBook<DS, PRODUCTS>;
  constexpr int S = cell_pieces(MAXIMA);
  constexpr int KS = T::KS;
  constexpr int kDepth = T::kDepth;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* book = reinterpret_cast<unsigned*>(smem);  // DS = 2: [j][c] (h0 h1, l0 l1); DS = 1: [j][c] (h l)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* x2w = reinterpret_cast<float*>(smem + T::kBook) + wave * 32;
  uint2* stage = reinterpret_cast<uint2*>(smem + T::kBook + T::kNorms) + wave * (64 * kDepth) + lane;  // [entry][lane]
  int* work = reinterpret_cast<int*>(a.params) + 8 + a.work;
  const int n_blocks = a.blk_off[a.n_cells];
  const int col = lane & 31, half = lane >> 5;
  const float sx = a.kparams[3];
  const float inv_sx = 1.f / sx;  // (a power of two: exact)
  const float inv_sx2 = inv_sx * inv_sx;
  // the tombstone bytes, or any readable bytes of one per slot when the index keeps none (the value is not used then)
  const uint8_t* __restrict__ emp = a.is_empty ? a.is_empty : a.codes;
  if constexpr (PRODUCTS == 1) {
    if (a.book) {  // the hi dwords of two entries of the kept image per 16-byte load
      const u32x4* __restrict__ img = reinterpret_cast<const u32x4*>(a.book);
      for (int i = tid; i < 64 * 256 / 2; i += T::kThreads) {
        const u32x4 v = img[i];
        reinterpret_cast<uint2*>(book)[i] = make_uint2(v[0], v[2]);
      }
    } else {  // (book_entry's hi pieces)
      for (int i = tid; i < 64 * 256; i += T::kThreads) {
        const int j = i >> 8, c = i & 255;
        book[i] = pack_f16x2((_Float16)(a.codebook[(j * 2) * 256 + c] * sx), (_Float16)(a.codebook[(j * 2 + 1) * 256 + c] * sx));
      }
    }
  } else if (a.book) {  // the kept image: 16 bytes per thread and round, no conversion
    const u32x4* __restrict__ img = reinterpret_cast<const u32x4*>(a.book);
    for (int i = tid; i < (int)(T::kBook / 16); i += T::kThreads) reinterpret_cast<u32x4*>(book)[i] = img[i];
  } else {
    for (int i = tid; i < 64 * 256; i += T::kThreads) book_entry<DS>(a.codebook, sx, i, book);  // entry (j, c)
  }
  __syncthreads();
  const int64_t cap = (int64_t)a.chunks * 64;
  const int seed_entries = ((a.k + 63) / 64) * 64;
  for (;;) {
    int b = 0;
    if (lane == 0) b = atomicAdd(work, 1);
    b = __builtin_amdgcn_readfirstlane(b);
    // draw w is piece w % S of block w / S (S = 1: the block)
    const int piece = S > 1 ? b % S : 0;
    if constexpr (S > 1) b /= S;
    if (b >= n_blocks) break;
    // the block's cell: blk_off[c] <= b < blk_off[c + 1]
    int lo = 0, hi = a.n_cells;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.blk_off[mid] <= b) lo = mid; else hi = mid;
    }
    const int c = lo, g = b - a.blk_off[c];
    const int first = a.cell_off[c] + g * kCellGroup;
    const int n_listed = a.cell_off[c + 1] - first;
    const int nqs = n_listed < kCellGroup ? n_listed : kCellGroup;
    const int64_t st = a.cell_st[c];
    int sz = a.cell_sz[c];
    if (st < 0 || sz < 0 || st + sz > a.n_slots) sz = 0;  // (an extent outside the storage is never read)
    if (sz == 0) continue;
    // the piece's rows [r_lo, r_hi): whole tiles of the cell's ceil(sz / 32), the last one cut at the size.  A cell of
    // fewer tiles than pieces leaves some of them empty: the draw, and nothing else
    int r_lo = 0, r_hi = sz;
    if constexpr (S > 1) {
      const int nt = (sz + 31) >> 5;
      r_lo = (piece * nt / S) << 5;
      r_hi = ((piece + 1) * nt / S) << 5;
      if (r_lo == r_hi) continue;
      if (r_hi > sz) r_hi = sz;
    }
    // this lane's query: pieces of s_q q for the B operand, threshold and scales
    const bool qvalid = col < nqs;
    const int q = qvalid ? a.pairs[first + col] : 0;
    const float sq = qvalid ? a.qscale[q] : 0.f;
    const float thr2 = qvalid ? a.thr[q] : INFINITY;  // (the seed kernel's: folded over |q|^2 when euclidean)
    const float q2 = qvalid ? a.qnorm[q] : 0.f;
    const float unscale = qvalid ? (1.f / sq) * inv_sx : 0.f;
    // the admission test of a row is ONE fma and ONE compare (see the header): test = fma(acc, um, -|x|^2) >= thr2.
    // A lane without a query has um = 0 and thr2 = +inf: its test value is -|x|^2, 0 or NaN, and never passes
    const float um = EUCLID ? 2.f * unscale : unscale;
    f16x8 qh[KS], ql[PRODUCTS == 3 ? KS : 1];
    const _Float16* __restrict__ qs = a.qsplit + (int64_t)q * kCellQSplit + 8 * half;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      qh[s] = __builtin_bit_cast(f16x8, qvalid ? *reinterpret_cast<const u32x4*>(qs + 16 * s) : z);
      if constexpr (PRODUCTS == 3)
        ql[s] = __builtin_bit_cast(f16x8, qvalid ? *reinterpret_cast<const u32x4*>(qs + 128 + 16 * s) : z);
    }
    // the code dwords of this lane's components: k-step s holds components [16 s + 8 half, + 8), i.e. sub-quantizers
    // [(16 s + 8 half) / DS, + 8 / DS): one dword at ds = 2, two at ds = 1; aux: the norm's bits (NORMS) or the tombstone
    // byte.  Every load is unconditional: a row past the size reads the cell's last row (0 < sz, st + sz <= n_slots)
    auto load_tile = [&](int r0, uint32_t (&w)[8], unsigned& aux) {
      const int row = r0 + col < sz ? r0 + col : sz - 1;
      const int64_t slot = st + row;
      const uint32_t* __restrict__ cw = reinterpret_cast<const uint32_t*>(a.codes) + slot;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int gq = DS == 2 ? 2 * i + half : 4 * (i >> 1) + 2 * half + (i & 1);
        w[i] = cw[(int64_t)gq * a.n_slots];
      }
      if constexpr (NORMS)
        aux = __float_as_uint(a.norm[slot]);
      else
        aux = emp[slot];
    };
    // a flush: one counter update for the lane's staged entries; those at or beyond cap are counted and not written.
    // (A loop, not unrolled: the flush stands in front of every row of the tile, and runs before few.)
    int fill = 0;
    auto flush = [&]() {
      if (fill > 0) {
        const int64_t e0 = (int64_t)seed_entries + atomicAdd(&a.cnt[q], fill);
        if (e0 + fill > cap) a.flags[q] = a.epoch;
        unsigned* __restrict__ qkeys = a.keys + (int64_t)q * cap + e0;
        unsigned* __restrict__ qidx = a.idx + (int64_t)q * cap + e0;
        const int fits = e0 + fill <= cap ? fill : (e0 < cap ? (int)(cap - e0) : 0);
#pragma unroll 1
        for (int i = 0; i < fits; ++i) {
          const uint2 v = stage[i * 64];
          qkeys[i] = v.x;
          qidx[i] = v.y;
        }
      }
      fill = 0;
    };
    // MAXIMA: the lane's entries of its query's key area, reserved here once; a lane without a query stores nothing
    int me = (int)cap;
    unsigned* __restrict__ mkeys = a.keys + (int64_t)q * cap;
    if constexpr (MAXIMA) {
      if (qvalid) me = atomicAdd(&a.cnt[q], ((r_hi - r_lo + 31) >> 5) * (16 / kCellThrGroup));
    }
    uint32_t w[8], wn[8];
    unsigned aux = 0u, aux_n = 0u;
    load_tile(r_lo, w, aux);
    for (int r0 = r_lo; r0 < r_hi; r0 += 32) {
      load_tile(r0 + 32, wn, aux_n);  // (a piece's last tile: the next piece's first; the cell's: its last row again)
      const bool rv = r0 + col < sz;
      // (opaque: a load whose only use is a select is sunk under the select's condition, and waited for there)
      asm volatile("" : "+v"(aux));
      float nrm = 0.f;
      bool live = false;
      if constexpr (NORMS)
        nrm = rv ? __uint_as_float(aux) : __builtin_nanf("");
      else
        live = rv & ((a.is_empty == nullptr) | (aux == 0u));
      f32x16 acc = zero_f32x16();
      float x2 = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        u32x4 vh, vl;
        if constexpr (PRODUCTS == 1) {
          const int j0 = 8 * s + 4 * half;
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) vh[bb] = book[(j0 + bb) * 256 + (int)((w[s] >> (8 * bb)) & 255u)];
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vh), qh[s], acc, 0, 0, 0);
          continue;
        } else if constexpr (DS == 2) {
          const int j0 = 8 * s + 4 * half;
          uint2 en[4];
#pragma unroll
          for (int bb = 0; bb < 4; ++bb)
            en[bb] = reinterpret_cast<const uint2*>(book)[(j0 + bb) * 256 + (int)((w[s] >> (8 * bb)) & 255u)];
#pragma unroll
          for (int bb = 0; bb < 4 && !NORMS; ++bb) {
            const float v0 = f16_lo(en[bb].x) + f16_lo(en[bb].y), v1 = f16_hi(en[bb].x) + f16_hi(en[bb].y);
            x2 = fmaf(v0, v0, x2);
            x2 = fmaf(v1, v1, x2);
          }
          vh = u32x4{en[0].x, en[1].x, en[2].x, en[3].x};
          vl = u32x4{en[0].y, en[1].y, en[2].y, en[3].y};
        } else {
          const int j0 = 16 * s + 8 * half;
          unsigned en[8];
#pragma unroll
          for (int bb = 0; bb < 8; ++bb)
            en[bb] = book[(j0 + bb) * 256 + (int)((w[2 * s + (bb >> 2)] >> (8 * (bb & 3))) & 255u)];
#pragma unroll
          for (int bb = 0; bb < 8 && !NORMS; ++bb) {
            const float v0 = f16_lo(en[bb]) + f16_hi(en[bb]);
            x2 = fmaf(v0, v0, x2);
          }
          vh = u32x4{(en[0] & 0xffffu) | (en[1] << 16), (en[2] & 0xffffu) | (en[3] << 16),
                        (en[4] & 0xffffu) | (en[5] << 16), (en[6] & 0xffffu) | (en[7] << 16)};
          vl = u32x4{(en[0] >> 16) | (en[1] & 0xffff0000u), (en[2] >> 16) | (en[3] & 0xffff0000u),
                     (en[4] >> 16) | (en[5] & 0xffff0000u), (en[6] >> 16) | (en[7] & 0xffff0000u)};
        }
        // the three products of the k-step, the small ones first (the bound holds for any order of accumulation)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vl), qh[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vh), ql[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vh), qh[s], acc, 0, 0, 0);
      }
      // (a row past the cell's size or a tombstone: NaN, which no comparison passes; the inner product's test needs
      // only that: its rows carry 0 or NaN)
      if constexpr (NORMS) {
        if (half == 0) x2w[col] = EUCLID ? nrm : nrm * 0.f;
      } else {
        // |x'|^2 of the row: this lane's half of the components and the other half-wave's
        x2 += __shfl_xor(x2, 32, 64);
        const float v = live ? x2 * inv_sx2 : __builtin_nanf("");
        if (half == 0) x2w[col] = EUCLID ? v : v * 0.f;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      // accumulator register 4 g + i holds row 8 g + 4 half + i of the tile: four 16-byte reads bring the 16 norms.
      // A row's compare leaves its 64 lanes' answers in a scalar register pair: whether anybody admitted the row is
      // scalar work, and a row nobody admitted costs no vector instruction beyond its fma and compare
      if constexpr (MAXIMA) {
        // the tested values of the lane's 16 rows, reduced per group: fmaxf takes the other operand over a NaN (a row
        // past the size, a tombstone), so a group's maximum is -inf exactly when none of its rows is live
        float gm[16 / kCellThrGroup];
#pragma unroll
        for (int g = 0; g < 16 / kCellThrGroup; ++g) gm[g] = -INFINITY;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const f32x4 x4 = *reinterpret_cast<const f32x4*>(x2w + 8 * gq + 4 * half);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * gq + i;
            gm[r / kCellThrGroup] = fmaxf(gm[r / kCellThrGroup], fmaf(acc[r], um, -x4[i]));
          }
        }
#pragma unroll
        for (int g = 0; g < 16 / kCellThrGroup; ++g) {
          const unsigned key = gm[g] == -INFINITY ? 0u : f2key(EUCLID ? gm[g] - q2 : gm[g]);
          if (me < (int)cap) mkeys[(int)cap - 1 - me] = key;  // (from the end of the area downwards: the header)
          ++me;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = wn[i];
        aux = aux_n;
        continue;
      }
      float xr[16];
      bool adm[16];
      unsigned long long any[16];  // (the compare's scalar register pair)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(x2w + 8 * gq + 4 * half);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * gq + i;
          xr[r] = x4[i];
          adm[r] = fmaf(acc[r], um, -xr[r]) >= thr2;
          any[r] = __ballot(adm[r]);
        }
      }
      // (all 16 compares ahead of the walk: sunk to its rows, each is a compare, a wait for its scalar result and a
      // taken branch, one after the other)
#pragma unroll
      for (int r = 0; r < 16; ++r) asm volatile("" ::"s"(any[r]));
      // an admitted row goes to its lanes' segments, under the compare's mask -- the key formed as ever, for these
      // lanes only; a row that some admitting lane's segment cannot take flushes the wave first
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (__builtin_expect(any[r] != 0ull, 0)) {
          if ((any[r] & __ballot(fill >= kDepth)) != 0ull) flush();
          if (adm[r]) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            float s = acc[r];
            asm volatile("" : "+v"(s));  // (opaque: the keys of all 16 rows are otherwise formed ahead of the walk)
            const float dot = s * unscale;
            const float fast = EUCLID ? (2.f * dot - xr[r]) - q2 : dot;
            stage[fill * 64] = make_uint2(f2key(fast), ~(unsigned)(st + r0 + row));
            ++fill;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = wn[i];
      aux = aux_n;
    }
    flush();
  }
}

// The threshold form's step between its two passes, one wave per query: M_k, the k-th largest of the min(cnt, capacity)
// group maxima pass A left in the query's key area -- the finish kernel's search over key images (scan_fk.h), the chunks
// in registers; fewer than k maxima: -inf --, then thr[q] = M_k - 2 delta_q, folded over |q|^2 when euclidean, where the
// candidate kernel reads it.  cnt[q] is zeroed for pass B.  Pass A wrote keys only: the pad indices and the eviction
// words of the seed kernel stand as they were, so nothing else is restored.  A flagged query keeps thr = +inf.
template <int NCH>
__global__ __launch_bounds__(256) void cell_kth_kernel(CellArgs a) {
  const int lane = (int)(threadIdx.x & 63);
  const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (q >= a.nq) return;  // (wave-uniform)
  const int n_all = __builtin_amdgcn_readfirstlane(a.cnt[q]);
  if (lane == 0) {
    a.cnt[q] = 0;
    if (a.n_max) a.n_max[q] = n_all;  // (diagnostics: what pass A reserved)
  }
  if (a.flags[q] == a.epoch) return;
  const int cap = a.chunks * 64;  // (the launch: chunks <= NCH)
  const int n = n_all < cap ? n_all : cap;
  const unsigned* __restrict__ keys = a.keys + (int64_t)q * cap;
  unsigned hi[NCH];
#pragma unroll
  for (int t = 0; t < NCH; ++t) hi[t] = t * 64 + lane < n ? keys[cap - 1 - (t * 64 + lane)] : 0u;  // (0: counts for nothing)
  const unsigned fk = finish_fk_upto<2, NCH>(hi, (n + 63) / 64, a.thr_k);
  if (lane == 0) {
    const float t = (fk ? key2f(fk) : -INFINITY) - a.ws_delta[q];
    a.thr[q] = a.euclid ? cell_fold_threshold(t, a.qnorm[q]) : t;
  }
}

// the metric is the kernel's: no select on it in the tile loop
template <int DS, bool NORMS, bool MAXIMA = false, int PRODUCTS = 3>
static int launch_cand(const CellArgs& a, dim3 grid, hipStream_t st) {
  using T = CellBook<DS, PRODUCTS>;
  const dim3 wg(T::kThreads);
  return a.euclid ? launch_with_lds(cell_cand_kernel<DS, NORMS, true, MAXIMA, PRODUCTS>, "cell_cand_kernel", grid, wg, T::kBytes, st, a)
                  : launch_with_lds(cell_cand_kernel<DS, NORMS, false, MAXIMA, PRODUCTS>, "cell_cand_kernel", grid, wg, T::kBytes, st, a);
}

static int cell_cus() {
  int dev = 0, n_cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cus <= 0)
    n_cus = 256;
  return n_cus;
}

// the kept state (a.kparams, a.book, a.norm of cell_use_kept): parameters, codebook image, a norm per slot address
static int launch_cell_kept_build(const CellArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(cell_prep_kernel, dim3(1), dim3(1024), 0, st, a);
  TPQ_LAUNCH_CHECK("cell_prep_kernel");
  if (a.ds == 1)
    hipLaunchKernelGGL(cell_book_kernel<1>, dim3(64), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(cell_book_kernel<2>, dim3(64), dim3(256), 0, st, a);
  TPQ_LAUNCH_CHECK("cell_book_kernel");
  const int64_t units = (a.n_slots + 511) / 512;
  if (units < 1) return TPQ_OK;
  const int n_cus = cell_cus();
  const dim3 grid((unsigned)(units < n_cus ? units : n_cus)), wg(512);
  return a.ds == 1 ? launch_with_lds(cell_norm_kernel<1, true>, "cell_norm_kernel", grid, wg, 64 * 256 * 4, st, a)
                   : launch_with_lds(cell_norm_kernel<2, true>, "cell_norm_kernel", grid, wg, 64 * 256 * 8, st, a);
}

// the head of a call: what depends on the index alone -- per call (cell_prep_kernel), or the kept state, built here when
// it is not valid yet and otherwise left alone --, then the seed kernel
static int launch_cell_head(const CellArgs& a, hipStream_t st) {
  if (!a.book) {
    hipLaunchKernelGGL(cell_prep_kernel, dim3(1), dim3(1024), 0, st, a);
    TPQ_LAUNCH_CHECK("cell_prep_kernel");
  } else if (a.kept_build) {
    if (int rc = launch_cell_kept_build(a, st)) return rc;
  }
  hipLaunchKernelGGL(cell_seed_kernel, dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, st, a);
  TPQ_LAUNCH_CHECK("cell_seed_kernel");
  return TPQ_OK;
}

// the inversion of the pairs (q, p), p0 <= p < p_hi, into a's hist / cell_off / blk_off / cell_st / cell_sz / pairs:
// a workgroup per slice of kCellSlice queries over an LDS histogram, while one fits
// a.p_a > 0 (n_cells <= kCellLdsCells / 2: the caller's): the one walk, both views from these three launches
static std::atomic<long long> g_cell_inversions{0};  // diagnostics: count / scan / scatter chains launched so far
static int launch_cell_inversion(const CellArgs& a, hipStream_t st) {
  g_cell_inversions.fetch_add(1);
  const dim3 per_query((unsigned)((a.nq + 3) / 4));
  const bool lds_hist = a.n_cells <= kCellLdsCells;
  const dim3 per_slice((unsigned)((a.nq + kCellSlice - 1) / kCellSlice)), slice_wg(kCellSliceThreads);
  const size_t hist_lds = (size_t)a.n_cells * sizeof(int);  // (<= 64 KiB: no attribute to raise)
  if (a.p_a > 0) {
    hipLaunchKernelGGL(cell_count_kernel<true>, per_slice, slice_wg, 2 * hist_lds, st, a);
    TPQ_LAUNCH_CHECK("cell_count_kernel");
    hipLaunchKernelGGL(cell_scan_kernel, dim3(2), dim3(1024), 0, st, a);
    TPQ_LAUNCH_CHECK("cell_scan_kernel");
    hipLaunchKernelGGL(cell_scatter_kernel<true>, per_slice, slice_wg, 2 * hist_lds, st, a);
    TPQ_LAUNCH_CHECK("cell_scatter_kernel");
    return TPQ_OK;
  }
  if (lds_hist) {
    hipLaunchKernelGGL(cell_count_kernel<false>, per_slice, slice_wg, hist_lds, st, a);
    TPQ_LAUNCH_CHECK("cell_count_kernel");
  } else {
    hipLaunchKernelGGL(cell_count_wide_kernel, per_query, dim3(256), 0, st, a);
    TPQ_LAUNCH_CHECK("cell_count_wide_kernel");
  }
  hipLaunchKernelGGL(cell_scan_kernel, dim3(1), dim3(1024), 0, st, a);
  TPQ_LAUNCH_CHECK("cell_scan_kernel");
  if (lds_hist) {
    hipLaunchKernelGGL(cell_scatter_kernel<false>, per_slice, slice_wg, hist_lds, st, a);
    TPQ_LAUNCH_CHECK("cell_scatter_kernel");
  } else {
    hipLaunchKernelGGL(cell_scatter_wide_kernel, per_query, dim3(256), 0, st, a);
    TPQ_LAUNCH_CHECK("cell_scatter_wide_kernel");
  }
  return TPQ_OK;
}

// the norms of the listed cells, once per call: cells dealt over at most one workgroup per CU
static int launch_cell_norms(const CellArgs& a, int n_cus, hipStream_t st) {
  const dim3 norm_grid((unsigned)(a.n_cells < n_cus ? a.n_cells : n_cus)), wg(512);
  return a.ds == 1 ? launch_with_lds(cell_norm_kernel<1>, "cell_norm_kernel", norm_grid, wg, 64 * 256 * 4, st, a)
                   : launch_with_lds(cell_norm_kernel<2>, "cell_norm_kernel", norm_grid, wg, 64 * 256 * 8, st, a);
}

// one workgroup of eight waves per CU, fewer when the call cannot list that many pieces of (cell, group) blocks: at
// most one block per listed cell plus one per full group of pairs; 0: nothing can be listed
static unsigned cell_cand_grid(const CellArgs& a, int n_cus, bool maxima = false) {
  const int64_t np = (int64_t)a.nq * (a.p_hi > a.p0 ? a.p_hi - a.p0 : 0);
  int64_t blocks = (int64_t)a.n_cells + np / kCellGroup;
  if (blocks > np) blocks = np;
  if (blocks < 1) return 0;
  const int waves = cell_waves(a.products);
  blocks = (blocks * cell_pieces(maxima) + waves - 1) / waves;
  return (unsigned)(blocks > n_cus ? n_cus : blocks);
}

// the candidate kernel's draw counter is an int: blocks x pieces, plus one failed draw per wave of the launch
static bool cell_draws_fit(const CellArgs& a) {
  const int64_t blocks = (int64_t)a.n_cells + (int64_t)a.nq * a.max_nprobe / kCellGroup;
  const int s = kCellPiecesA > kCellPiecesB ? kCellPiecesA : kCellPiecesB;
  return blocks * s + 65536 < 0x7fffffffLL;
}

int launch_cell_candidates(const CellArgs& a, hipStream_t st) {
  if (a.nq <= 0) return TPQ_OK;
  TPQ_REQUIRE(cell_draws_fit(a), "ivfpq_scan (cell-major): more pieces of blocks than the draw counter holds");
  if (int rc = launch_cell_head(a, st)) return rc;
  if (a.p_hi <= a.p0) return TPQ_OK;
  if (int rc = launch_cell_inversion(a, st)) return rc;
  const int n_cus = cell_cus();
  TPQ_REQUIRE(a.products == 3, "ivfpq_scan (cell-major): the seeded form runs three products");
  const dim3 grid(cell_cand_grid(a, n_cus));
  if (a.norm) {
    if (!a.book)  // (a kept state holds the norms of every slot)
      if (int rc = launch_cell_norms(a, n_cus, st)) return rc;
    return a.ds == 1 ? launch_cand<1, true>(a, grid, st) : launch_cand<2, true>(a, grid, st);
  }
  return a.ds == 1 ? launch_cand<1, false>(a, grid, st) : launch_cand<2, false>(a, grid, st);
}

void cell_fill_thr(CellThrArrays& t, void* at, int nq, int max_nprobe, int n_cells) {
  char* p = reinterpret_cast<char*>(at);
  auto take = [&](size_t bytes) {
    int* r = reinterpret_cast<int*>(p);
    p += cell_align(bytes);
    return r;
  };
  const int tp = max_nprobe < kCellThrProbes ? max_nprobe : kCellThrProbes;
  t.pairs_b = take((size_t)nq * max_nprobe * 4);
  t.hist = take((size_t)n_cells * 4);
  t.cell_off = take(((size_t)n_cells + 1) * 4);
  t.blk_off = take(((size_t)n_cells + 1) * 4);
  t.cell_st = take((size_t)n_cells * 4);
  t.cell_sz = take((size_t)n_cells * 4);
  t.pairs = take((size_t)nq * tp * 4);
  t.n_max = take((size_t)nq * 4);
}

int launch_cell_threshold(const CellArgs& a, const CellThrArrays& t, hipStream_t st) {
  if (a.nq <= 0) return TPQ_OK;
  TPQ_REQUIRE(a.norm && a.k == 0 && a.thr_k >= 1 && a.p0 == 0 && a.p_hi == a.max_nprobe && a.chunks <= 16,
              "ivfpq_scan (cell threshold): arguments outside the form");
  TPQ_REQUIRE(cell_draws_fit(a), "ivfpq_scan (cell threshold): more pieces of blocks than the draw counter holds");
  // pass B's view: every probe, its pairs in the form's own array; pass A's: the first kCellThrProbes, its own inversion
  // arrays and block counter.  The cells A lists are among B's (the same rule over a prefix of the same probes), so
  // the slot norms of B's cells cover them
  CellArgs b = a;
  b.n_max = t.n_max;
  b.pairs = t.pairs_b;
  b.hist2 = t.hist;
  b.work = 0;
  CellArgs pa = b;
  pa.p_hi = a.max_nprobe < kCellThrProbes ? a.max_nprobe : kCellThrProbes;
  pa.hist = t.hist; pa.cell_off = t.cell_off; pa.blk_off = t.blk_off; pa.cell_st = t.cell_st; pa.cell_sz = t.cell_sz;
  pa.pairs = t.pairs;
  pa.hist2 = nullptr;
  pa.work = 1;
  if (int rc = launch_cell_head(b, st)) return rc;
  // one walk for both views while two LDS histograms fit; beyond, pass A's own count / scan / scatter as before
  const bool one_walk = a.n_cells <= kCellLdsCells / 2;
  if (one_walk) {
    b.p_a = pa.p_hi;
    b.va = CellView{t.hist, t.cell_off, t.blk_off, t.cell_st, t.cell_sz, t.pairs};
  }
  if (int rc = launch_cell_inversion(b, st)) return rc;
  b.p_a = 0;
  const int n_cus = cell_cus();
  if (!b.book)  // (a kept state holds the norms of every slot)
    if (int rc = launch_cell_norms(b, n_cus, st)) return rc;
  if (!one_walk)
    if (int rc = launch_cell_inversion(pa, st)) return rc;
  // both passes on the same arithmetic, always: they share delta_q
  const bool single = a.products == 1;
  const dim3 grid_a(cell_cand_grid(pa, n_cus, true));
  if (int rc = a.ds == 1 ? launch_cand<1, true, true>(pa, grid_a, st)
               : single  ? launch_cand<2, true, true, 1>(pa, grid_a, st)
                         : launch_cand<2, true, true>(pa, grid_a, st))
    return rc;
  const dim3 per_query((unsigned)((a.nq + 3) / 4));
  if (a.chunks <= 8)
    hipLaunchKernelGGL(cell_kth_kernel<8>, per_query, dim3(256), 0, st, b);
  else
    hipLaunchKernelGGL(cell_kth_kernel<16>, per_query, dim3(256), 0, st, b);
  TPQ_LAUNCH_CHECK("cell_kth_kernel");
  const dim3 grid(cell_cand_grid(b, n_cus));
  return a.ds == 1 ? launch_cand<1, true>(b, grid, st)
         : single  ? launch_cand<2, true, false, 1>(b, grid, st)
                   : launch_cand<2, true>(b, grid, st);
}

}  // namespace tpq

using namespace tpq;

extern "C" int tpq_ivfpq_cell_candidates(const uint8_t* codes, const float* query, const float* codebook, int ds,
                                         int metric, const uint8_t* is_empty, const int64_t* cell_start,
                                         const int64_t* cell_size, const int64_t* n_probe_list, const int64_t* cells,
                                         int n_cells, int first_probe, const float* threshold, int64_t n_slots, int nq,
                                         int max_nprobe, int m, int capacity, int32_t* out_count, uint32_t* out_keys,
                                         uint32_t* out_addr, float* out_delta, int32_t* out_flags, void* workspace,
                                         size_t workspace_bytes, tpq_stream_t stream) {
  TPQ_REQUIRE(codes && query && codebook && cell_start && cell_size && n_probe_list && cells && threshold &&
                  out_count && out_keys && out_addr && out_delta && out_flags,
              "ivfpq_cell_candidates: null pointer argument");
  TPQ_REQUIRE(m == 64 && (ds == 1 || ds == 2), "ivfpq_cell_candidates: m = 64 and ds <= 2 only (m=%d, ds=%d)", m, ds);
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "ivfpq_cell_candidates: bad metric %d",
              metric);
  TPQ_REQUIRE(nq >= 0 && max_nprobe >= 1 && n_cells >= 1 && first_probe >= 0 && n_slots >= 0 &&
                  n_slots < 0x7fffffffLL && (int64_t)nq * max_nprobe < 0x7fffffffLL,
              "ivfpq_cell_candidates: bad shape (nq=%d, max_nprobe=%d, n_cells=%d, first_probe=%d)", nq, max_nprobe,
              n_cells, first_probe);
  TPQ_REQUIRE(capacity >= 64 && capacity % 64 == 0 && capacity <= 65536,
              "ivfpq_cell_candidates: capacity=%d must be a multiple of 64 in [64, 65536]", capacity);
  const size_t need = cell_extra_bytes(nq, max_nprobe, n_cells, first_probe);
  if (!workspace || workspace_bytes < need) {
    set_error("ivfpq_cell_candidates: workspace too small (%zu < %zu)", workspace_bytes, need);
    return TPQ_ERR_WORKSPACE;
  }
  CellArgs a{};
  a.codes = codes; a.query = query; a.codebook = codebook; a.is_empty = is_empty;
  a.cell_start = cell_start; a.cell_size = cell_size; a.n_probe_list = n_probe_list; a.cells = cells;
  a.n_slots = n_slots; a.nq = nq; a.max_nprobe = max_nprobe; a.n_cells = n_cells; a.ds = ds;
  a.euclid = metric == TPQ_METRIC_NEG_SQ_L2 ? 1 : 0;
  a.p0 = first_probe; a.p_hi = max_nprobe; a.k = 0; a.chunks = capacity / 64; a.epoch = 1; a.rel = cell_delta_rel(ds);
  a.thr_in = threshold;
  a.products = 3;
  a.keys = out_keys; a.idx = out_addr; a.flags = out_flags; a.ws_delta = out_delta;
  cell_fill_extras(a, workspace, workspace_bytes);  // (with room behind the extras: the slot norms, once per call)
  a.cnt = out_count;
  return launch_cell_candidates(a, reinterpret_cast<hipStream_t>(stream));
}

extern "C" long long tpq_ivfpq_scan_cell_inversions(void) { return g_cell_inversions.load(); }

extern "C" float tpq_ivfpq_cell_fold_threshold(float threshold, float q2) { return cell_fold_threshold(threshold, q2); }

extern "C" size_t tpq_ivfpq_cell_candidates_workspace_bytes(int nq, int max_nprobe, int n_cells, int first_probe) {
  if (nq <= 0 || max_nprobe < 1 || n_cells < 1 || first_probe < 0) return 0;
  return cell_extra_bytes(nq, max_nprobe, n_cells, first_probe);
}

extern "C" size_t tpq_ivfpq_cell_candidates_norms_workspace_bytes(int nq, int max_nprobe, int n_cells, int first_probe,
                                                                  int64_t n_slots) {
  if (nq <= 0 || max_nprobe < 1 || n_cells < 1 || first_probe < 0 || n_slots < 0) return 0;
  return cell_extra_bytes(nq, max_nprobe, n_cells, first_probe) + cell_norm_bytes(n_slots);
}
