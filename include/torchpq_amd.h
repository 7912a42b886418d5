/* torchpq_amd.h -- C ABI of libtorchpq_amd.so: the MI355X (gfx950) IVFPQ hot path.
 *
 * Drop-in boundary for DeMoriarty/TorchPQ's kernel-wrapper layer
 * (the torchpq/kernels/ xxxCuda.py wrappers).  Every entry point replaces one CuPy RawKernel
 * wrapper of the reference; the reference file:line each one stands in for is
 * cited at its declaration (paths relative to the reference repository root).
 *
 * Conventions (same contract as the reference wrappers):
 *   - all pointers are DEVICE pointers owned by the caller (torch's caching
 *     allocator in the Python host); the library never allocates, frees or
 *     keeps device memory between calls, holds no state between calls and
 *     reads no environment variable (every entry point is re-entrant; the one
 *     third-party exception: tpq_get_ioa sorts with rocPRIM's radix sort, which
 *     consults ROCPRIM_USE_ATOMIC_BLOCK_ID and caches the device architecture);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the null stream) and never synchronises;
 *   - tensors are dense, row-major, in the reference's layouts;
 *   - return value: TPQ_OK (0) or a negative TPQ_ERR_* code; the message is
 *     available from tpq_last_error() (thread-local).
 */
#ifndef TORCHPQ_AMD_H_
#define TORCHPQ_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPQ_VERSION 500 /* 0.5.0 */

#define TPQ_OK 0
#define TPQ_ERR_INVALID_ARGUMENT (-1)
#define TPQ_ERR_HIP (-2)
#define TPQ_ERR_WORKSPACE (-3)
#define TPQ_ERR_UNSUPPORTED (-4)

/* similarity metrics (values are "larger = closer", as in the reference) */
#define TPQ_METRIC_NEG_SQ_L2 0 /* "euclidean": -|a-b|^2 */
#define TPQ_METRIC_INNER 1     /* "cosine"/"inner": a.b (inputs pre-normalised by the host) */

typedef void* tpq_stream_t; /* hipStream_t */

int tpq_version(void);
const char* tpq_last_error(void);

/* ---------------------------------------------------------------------------
 * a-1 / a-2  IVF list scan + top-k
 * replaces IVFPQTopkCuda.topk      torchpq/kernels/IVFPQTopkCuda.py:81-142
 *          IVFPQTop1Cuda.topk      torchpq/kernels/IVFPQTop1Cuda.py:86-140
 * kernels  ivfpq_topk              torchpq/kernels/cuda/ivfpq_topk.cu:822-971
 *          ivfpq_top1              torchpq/kernels/cuda/ivfpq_top1.cu:385-455
 *
 * codes        u8  [m/4][n_slots][4]   CellContainer._storage (contiguous_size=4)
 * lut          f32 [m][nq][256]        PQCodec.precompute_adc output
 * is_empty     u8  [n_slots] or NULL   1 = free/tombstone (NULL: no slot is skipped)
 * cell_start   i64 [nq][max_nprobe]    _cell_start[cells]
 * cell_size    i64 [nq][max_nprobe]    _cell_size[cells]
 * n_probe_list i64 [nq]                cells actually scanned per query (<= max_nprobe)
 * out_vals     f32 [nq][k]             descending; unfilled = -inf
 * out_addr     i64 [nq][k]             slot addresses; unfilled = -1
 * address2id   i64 [n_slots] or NULL   when given, out_ids (i64 [nq][k]) receives
 * out_ids                               BaseContainer.get_id_by_address(out_addr)
 *                                       (torchpq/container/BaseContainer.py:58-65)
 * n_split      workgroups per query (>=1); >1 needs workspace of
 *              tpq_ivfpq_scan_workspace_bytes(nq, k, n_split, m) (the packed variant always
 *              needs it: per-wave candidate lists are merged by a second kernel)
 *
 * value(slot) = 0.f; for j = 0..m-1 ascending: value += lut[j][q][code_j]  (fp32,
 * the order of consume_data, ivfpq_topk.cu:662-679).  Ordering: value descending,
 * exact ties by ascending address.  1 <= k <= 1024, m % 4 == 0, m <= 156.
 * ------------------------------------------------------------------------- */
/* The workspace need not be zeroed (or hold anything): flags are compared with a per-call epoch, every list, pool, count and
 * order array a call reads was written by that call's own kernels. */
size_t tpq_ivfpq_scan_workspace_bytes(int nq, int k, int n_split, int m);

int tpq_ivfpq_scan_topk(const uint8_t* codes, const float* lut, const uint8_t* is_empty,
                        const int64_t* cell_start, const int64_t* cell_size,
                        const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                        const int64_t* address2id, int64_t* out_ids, int64_t n_slots, int nq,
                        int max_nprobe, int m, int k, int n_split, void* workspace,
                        size_t workspace_bytes, tpq_stream_t stream);

/* MI355X scan layout ("packed"): same bytes as `codes`, permuted per slot so that
 * the 32 lanes of a half-wave always hit 32 distinct LDS banks.
 *   packed u8 [m/W][n_slots][W], W = 16 if m%16==0, else 8 if m%8==0, else 4.
 * tpq_ivfpq_pack_codes (re)builds slots [slot_begin, slot_end) of `packed` from `codes`.
 * tpq_ivfpq_scan_topk_packed has the contract of tpq_ivfpq_scan_topk (bit-identical
 * results) but streams `packed`; `codes` is still needed for the exact re-evaluation of
 * the few candidates that pass the threshold filter.
 * Launches: ONE for plain PQ with k <= 248 when the query is not split (n_split == 1) or the caller
 * passes tickets (the *_tickets entry points) -- the scan workgroups merge their lists, a query split over
 * n_split workgroups is written by the last of them to finish (a ticket per query), and a candidate
 * band that overflowed is redone exactly by that workgroup -- otherwise three (scan, merge, the
 * exact redo of flagged queries).
 * tickets  i32 [nq] (tpq_ivfpq_scan_tickets_bytes(nq) bytes), owned by the CALLER like every other
 *          buffer: all zero before the first call that uses them; every call leaves them all zero
 *          again, so one zeroing serves any number of calls.  Calls that share a ticket buffer must
 *          be ordered (same stream, or otherwise serialised): one buffer per stream in flight.  After
 *          a failed launch or a device fault zero the buffer again.  A graph captured with a ticket
 *          buffer replays with it: it must outlive the graph.  tickets == NULL (and the entry points
 *          without the argument): split queries take the three launches.
 * slots_hint  expected number of slots a query scans (n_probe x mean cell size; 0 = unknown).  Performance
 *          only: long cells let the kernel keep shorter candidate lists per wave (results are the same
 *          either way; a wrong hint costs an exact in-kernel redo of the queries it misleads). */
int tpq_ivfpq_pack_codes(const uint8_t* codes, uint8_t* packed, int64_t n_slots, int m,
                         int64_t slot_begin, int64_t slot_end, tpq_stream_t stream);

int tpq_ivfpq_scan_topk_packed(const uint8_t* packed, const uint8_t* codes, const float* lut,
                               const uint8_t* is_empty, const int64_t* cell_start,
                               const int64_t* cell_size, const int64_t* n_probe_list,
                               float* out_vals, int64_t* out_addr, const int64_t* address2id,
                               int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe, int m,
                               int k, int n_split, void* workspace, size_t workspace_bytes,
                               tpq_stream_t stream);
size_t tpq_ivfpq_scan_tickets_bytes(int nq);

/* Diagnostics: which kernels a scan call with these arguments runs -- a host-side function that launches nothing and
 * applies exactly the rules of the entry points above (tests assert the route a shape takes; bench.py names the timed
 * kernel from it).  `has_lut`: a materialised table is passed (tpq_ivfpq_scan_topk[_packed]) rather than query +
 * codebook (tpq_ivfpq_search_fused); `has_packed`: the scan-layout copy is passed; `residual`: the residual entry point.
 * Returns one of TPQ_SCAN_ROUTE_*, or -1 for arguments the entry points reject -- among them a scan-layout copy at an m
 * without a scan-layout kernel, with a table or on the residual entry point (the fused entry point scans the reference
 * layout then: TPQ_SCAN_ROUTE_REF).  The route returned is the one the entry point runs. */
#define TPQ_SCAN_ROUTE_REF 0            /* scan_ref_kernel / scan_residual_kernel: the reference layout, exact */
#define TPQ_SCAN_ROUTE_ONE_LAUNCH 1     /* scan_packed_kernel<.., RM > 0>: the scan workgroups finish their queries */
#define TPQ_SCAN_ROUTE_LISTS 2          /* scan_packed_kernel + scan_merge_refine_kernel + the flag-gated exact redo */
#define TPQ_SCAN_ROUTE_POOLS 3          /* large k: scan_packed_kernel<.., RM < 0> + scan_pool_merge_kernel + redo */
#define TPQ_SCAN_ROUTE_DUMP_F32 8       /* large batches, m = 8 / 16 / 32: fp32 table, scan_finish_exact_kernel + redo */
#define TPQ_SCAN_ROUTE_DUMP_SEL16 16    /* large batches, m = 64: 16-bit table, four-wave workgroups + finish + redo */
#define TPQ_SCAN_ROUTE_DUMP_SEL16_W8 17 /* ... eight-wave workgroups (k in (248, 504] on long cells) */
int tpq_ivfpq_scan_route(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint, int has_lut,
                         int has_packed, int has_tickets, int residual);
/* The dispatch order of a large batch.  The large-batch routes (TPQ_SCAN_ROUTE_DUMP_*) run one workgroup per query, and
 * workgroups start in index order: dispatched longest first, a batch ends on its shortest queries instead of on whichever
 * came last.  The scan entry points compute the order themselves, per call, on the stream (two small launches ahead of
 * the scan; no host read, no allocation, capturable in a graph), exactly when the batch needs more than one round of
 * the device's workgroup slots, holds at most 20 480 queries and the workspace has room for it behind the lists the
 * call uses -- three int32 per query, each array rounded up to 256 bytes, out of what tpq_ivfpq_scan_workspace_bytes
 * already covers; a smaller workspace keeps index order.  Results do not depend on the order.
 * tpq_ivfpq_scan_order is that computation on its own:
 *   work[q]  = sum over p < n_probe_list[q] (clamped to [0, max_nprobe]) of ceil(cell_size[q][p] / 2^tile_shift), a
 *              negative size counting 0 and a probe whose start equals the previous probe's start counting 0 (the scan
 *              skips it); saturates at 2^31 - 1
 *   order    i32 [nq]  a permutation of the queries, work non-increasing, equal work by ascending query
 *   rank     i32 [nq]  its inverse: rank[order[i]] == i
 * work is i32 [nq] like the other two; 0 <= tile_shift <= 16 (the scan's tiles: 64 slots at m > 32, 256 at m <= 32).
 * The ranking compares every pair of queries: its time grows with nq squared (about 18 us at 10 000 queries).
 * tpq_ivfpq_scan_ordered answers, without launching anything, whether a scan call with these arguments -- those of
 * tpq_ivfpq_scan_route, the workgroup slots of the device (0 = ask the current device) and the workspace size the
 * caller passes -- is dispatched in that order: 1 / 0, or -1 for arguments the entry points reject. */
int tpq_ivfpq_scan_order(const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list, int nq,
                         int max_nprobe, int tile_shift, int32_t* order, int32_t* rank, int32_t* work,
                         tpq_stream_t stream);
int tpq_ivfpq_scan_ordered(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint, int has_lut,
                           int has_packed, int has_tickets, int residual, int slots, size_t workspace_bytes);
int tpq_ivfpq_scan_topk_packed_tickets(const uint8_t* packed, const uint8_t* codes, const float* lut,
                                       const uint8_t* is_empty, const int64_t* cell_start,
                                       const int64_t* cell_size, const int64_t* n_probe_list,
                                       float* out_vals, int64_t* out_addr, const int64_t* address2id,
                                       int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe,
                                       int m, int k, int n_split, void* workspace,
                                       size_t workspace_bytes, int32_t* tickets, int64_t slots_hint,
                                       tpq_stream_t stream);

/* Fused a-3 + a-1: the scan workgroup builds its query's LUT itself from the query and the PQ
 * codebook (bit-identical entries to tpq_adc_lut: same fma chains), so the [m][nq][256] table is
 * never written to or read from HBM.  This is what IVFPQIndex.search_cells
 * (torchpq/index/IVFPQIndex.py:452-461: precompute_adc + IVFPQTopk.topk) collapses to.
 * query f32 [m*ds][nq], codebook f32 [m][ds][256]; `packed` may be NULL (reference-layout
 * kernel); everything else as tpq_ivfpq_scan_topk[_packed].
 * Large batches (nq >= 1024 with n_split == 1, m == 64, ds <= 2, k <= 504, `packed` given): three launches --
 * the scan workgroups (four per CU) stream over a 16-bit fixed-point SELECTION table built from query and
 * codebook and end with their lists of fast values; a finish kernel, one wave per query, evaluates every
 * candidate within the table's rigorous error band exactly (the reference's arithmetic and order, from the
 * codebook) and writes the result; the exact kernel redoes flagged queries (normally none).  Same results,
 * bit for bit.  The library deals the batch's last round of workgroups in parts of a query;
 * nothing of this shows at the boundary beyond the workspace size, which
 * tpq_ivfpq_scan_workspace_bytes(nq, k, n_split, 64) already covers.
 * Short codes (m == 8, 16, 32; k <= 248; m * ds <= 128 here, any table through tpq_ivfpq_scan_topk_packed) take the
 * same three launches over the fp32 table their workgroups stream over anyway: the scan workgroup ends after its
 * last tile, the finish kernel takes the exact entries from the codebook (this entry point) or from the caller's
 * table (tpq_ivfpq_scan_topk_packed).  tpq_ivfpq_scan_route tells which route a shape takes. */
int tpq_ivfpq_search_fused(const uint8_t* packed, const uint8_t* codes, const float* query,
                           const float* codebook, int ds, int metric, const uint8_t* is_empty,
                           const int64_t* cell_start, const int64_t* cell_size,
                           const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                           const int64_t* address2id, int64_t* out_ids, int64_t n_slots, int nq,
                           int max_nprobe, int m, int k, int n_split, void* workspace,
                           size_t workspace_bytes, tpq_stream_t stream);
int tpq_ivfpq_search_fused_tickets(const uint8_t* packed, const uint8_t* codes, const float* query,
                                   const float* codebook, int ds, int metric, const uint8_t* is_empty,
                                   const int64_t* cell_start, const int64_t* cell_size,
                                   const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                   const int64_t* address2id, int64_t* out_ids, int64_t n_slots,
                                   int nq, int max_nprobe, int m, int k, int n_split, void* workspace,
                                   size_t workspace_bytes, int32_t* tickets, int64_t slots_hint,
                                   tpq_stream_t stream);
/* The cell-major form of the m = 64 large-batch route (TPQ_SCAN_ROUTE_DUMP_SEL16).
 * tpq_ivfpq_search_fused_cells: the arguments of tpq_ivfpq_search_fused_tickets plus the probed cells themselves --
 * `cells` i64 [nq][max_nprobe], the ids behind cell_start / cell_size, in [0, n_cells); NULL gives
 * tpq_ivfpq_search_fused_tickets.  On a cell-dense batch (every code byte is read by hundreds of queries) the call then
 *   1. runs the route over each query's first 4 probes only: its exact top-k of those cells, tau_q = the k-th value;
 *   2. seeds the query's lists with that top-k;
 *   3. lists the remaining (query, probe) pairs by cell;
 *   4. decodes every listed cell once per 128 of its queries and takes the values of all of them from fp16 matrix-core
 *      products (three products of two-piece splits; rigorous error bound delta_q), appending every slot that may reach
 *      tau_q to the query's list;
 *   5. evaluates the lists exactly with the route's own finish kernel and redoes flagged queries (a list that overflowed,
 *      a NaN / Inf query, a cell id out of range, data outside the fp16 scale's range) with the exact kernel.
 * Same results, bit for bit.  All on `stream`, no host read, no allocation; the workspace is the one
 * tpq_ivfpq_scan_workspace_bytes sizes, and a smaller one keeps the query-major path.
 * tpq_ivfpq_scan_cell_major answers, without launching anything, whether a call with these arguments -- those of
 * tpq_ivfpq_scan_route, the number of cells, the slots of the storage and the workspace size the caller passes -- takes
 * the form when it hands over its cells: 1 / 0, or -1 for arguments the entry points reject.  The rule: the four-wave
 * route, k <= 128, more than 4 probes, nq * slots_hint / n_slots >= 96 and room in the workspace behind the lists in use.
 * tpq_ivfpq_scan_cell_norms, same arguments: whether step 4 of such a call reads the slot norms |x|^2 from an array
 * computed once per call (cell_norm_kernel) -- 1 when the form is taken and the workspace has room for 4 * n_slots bytes
 * (rounded up to 256) behind the lists and inversion arrays in use -- or forms them in every candidate block (0).  Same
 * results either way; 0 wherever tpq_ivfpq_scan_cell_major is 0.
 * tpq_ivfpq_cell_candidates is steps 3-4 on their own, with the caller's thresholds (m == 64, ds 1 or 2): for the
 * probes first_probe <= p < n_probe_list[q] of every query, every live slot whose fast value is >= threshold[q] - delta_q.
 *   out_count i32 [nq]             candidates admitted (beyond `capacity`: counted, not stored, out_flags[q] = 1)
 *   out_keys  u32 [nq][capacity]   order-preserving image of the fast value (a float f: bits | 2^31 when f >= 0, ~bits
 *                                  otherwise), in no particular order; out_addr u32 [nq][capacity]: ~slot; entries past
 *                                  the count hold ~(2^31 - 1) in out_addr and nothing in out_keys
 *   out_delta f32 [nq]             2 delta_q: every stored slot's exact value is >= threshold[q] - 2 delta_q
 *   out_flags i32 [nq]             1: the query took no part (NaN / Inf, a cell out of range, unscalable) or overflowed
 * capacity: a multiple of 64; workspace: tpq_ivfpq_cell_candidates_workspace_bytes, or
 * tpq_ivfpq_cell_candidates_norms_workspace_bytes (that size + 4 * n_slots rounded up to 256): a workspace of at least
 * the larger size takes the slot norms from an array computed once per call, a smaller one forms them in every block;
 * the same candidates with the same keys either way.
 * tpq_ivfpq_cell_fold_threshold (host only, launches nothing) is the fold step 4 applies to a euclidean query's
 * admission threshold: the smallest float t2 with  a >= t2  <=>  fl(a - q2) >= threshold  for every float a (q2 = |q|^2,
 * finite); -inf, +inf and NaN are returned as they are. */
int tpq_ivfpq_search_fused_cells(const uint8_t* packed, const uint8_t* codes, const float* query,
                                 const float* codebook, int ds, int metric, const uint8_t* is_empty,
                                 const int64_t* cell_start, const int64_t* cell_size,
                                 const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                 const int64_t* address2id, int64_t* out_ids, int64_t n_slots,
                                 int nq, int max_nprobe, int m, int k, int n_split, void* workspace,
                                 size_t workspace_bytes, int32_t* tickets, int64_t slots_hint,
                                 const int64_t* cells, int n_cells, tpq_stream_t stream);
int tpq_ivfpq_scan_cell_major(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint, int has_lut,
                              int has_packed, int has_tickets, int residual, int n_cells, int64_t n_slots,
                              size_t workspace_bytes);
int tpq_ivfpq_scan_cell_norms(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint, int has_lut,
                              int has_packed, int has_tickets, int residual, int n_cells, int64_t n_slots,
                              size_t workspace_bytes);
/* The workspace need not be zeroed: cell_seed_kernel clears every counter and array the later stages read. */
size_t tpq_ivfpq_cell_candidates_workspace_bytes(int nq, int max_nprobe, int n_cells, int first_probe);
/* The workspace need not be zeroed: the slot norms behind the arrays above are written by cell_norm_kernel for every listed cell. */
size_t tpq_ivfpq_cell_candidates_norms_workspace_bytes(int nq, int max_nprobe, int n_cells, int first_probe,
                                                       int64_t n_slots);
int tpq_ivfpq_cell_candidates(const uint8_t* codes, const float* query, const float* codebook, int ds, int metric,
                              const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                              const int64_t* n_probe_list, const int64_t* cells, int n_cells, int first_probe,
                              const float* threshold, int64_t n_slots, int nq, int max_nprobe, int m, int capacity,
                              int32_t* out_count, uint32_t* out_keys, uint32_t* out_addr, float* out_delta,
                              int32_t* out_flags, void* workspace, size_t workspace_bytes, tpq_stream_t stream);
float tpq_ivfpq_cell_fold_threshold(float threshold, float q2);
/* The threshold form of the cell-major form: steps 1 and 2 above are replaced by a first pass of step 4's kernel over
 * each query's first probes that keeps only group maxima of its values; the k-th largest maximum M_k bounds the k-th
 * best value from below, every slot of ALL probes with value >= M_k - 2 delta_q is appended, and step 5 evaluates the
 * lists.  No query-major pass, no seeds; same results, bit for bit.
 * tpq_ivfpq_scan_cell_threshold (arguments of tpq_ivfpq_scan_cell_major): 1 when tpq_ivfpq_search_fused_cells takes this
 * form -- tpq_ivfpq_scan_cell_norms is 1, the form's arrays fit the workspace behind the norms, there are more probes
 * than the first pass covers, slots_hint / max_nprobe >= 512 and the maxima expected of the first pass are at least 2 k.
 * tpq_ivfpq_scan_use_cell_threshold(on): the A/B switch of the two forms, process-wide, read on the host during a call;
 * 0 keeps every later call to steps 1 and 2, whatever tpq_ivfpq_scan_cell_threshold says.  Returns the previous setting.
 * tpq_ivfpq_scan_cell_threshold_probes(): the probes per query the first pass covers.
 * Diagnostics: the first pass fills a query's list of maxima from the END of its key area downwards, and the count of
 * them is kept behind the form's arrays, so both can be read from the workspace after the call
 * (IVFPQTopkHip.last_cell_threshold_state). */
int tpq_ivfpq_scan_cell_threshold(int nq, int k, int n_split, int m, int ds, int max_nprobe, int64_t slots_hint,
                                  int has_lut, int has_packed, int has_tickets, int residual, int n_cells,
                                  int64_t n_slots, size_t workspace_bytes);
int tpq_ivfpq_scan_use_cell_threshold(int on);
int tpq_ivfpq_scan_cell_threshold_probes(void);
/* The single-product key of the threshold form (ds = 2): both passes of step 4's kernel select on ONE fp16 product per
 * k-step -- the hi pieces of codebook and query -- instead of three, from half the codebook image in LDS, with a band
 * per query that bounds the dropped products per sub-quantizer from piece maxima of the codebook kept in the parameter
 * block (of the workspace and of the kept state; tpq_ivfpq_cell_kept_bytes and the layouts are unchanged).  Every
 * returned value is step 5's: same results, bit for bit.  The band is wider than that of three products (about three
 * times on SIFT-like data): data with many rows within it of the k-th best fill the lists sooner, and a query whose lists
 * overflow is redone exactly, as ever -- there is no automatic fall-back.
 * tpq_ivfpq_scan_use_cell_single_product(on): the A/B switch, process-wide, read on the host during a call; default 1;
 * 0 keeps every later call of the threshold form on three products.  Returns the previous setting.  ds = 1, the seeded
 * form, tpq_ivfpq_cell_candidates and every query-major route run three products whatever it says.
 * tpq_ivfpq_scan_last_cell_products(): the products per k-step the candidate kernels of the last packed scan call of this
 * process ran -- 1 or 3 --, 0 when that call did not take the cell-major form.  TPQ_VERSION is unchanged by these. */
#define TPQ_HAS_IVFPQ_CELL_SINGLE_PRODUCT 1
int tpq_ivfpq_scan_use_cell_single_product(int on);
int tpq_ivfpq_scan_last_cell_products(void);
/* The kept state of the cell-major form: what a call of the form with slot norms derives from the index alone -- the
 * codebook's scale and bound, the split fp16 codebook as the candidate kernels stage it, and an fp32 norm per slot
 * address (NaN: tombstone) -- in a caller-owned device buffer of tpq_ivfpq_cell_kept_bytes(n_slots, ds) bytes (host
 * arithmetic; 0 for ds outside 1, 2), so that a caller that searches an unchanged index many times pays for it once.
 * tpq_ivfpq_search_fused_cells_kept: tpq_ivfpq_search_fused_cells plus `kept`, its size and `kept_valid`.  A call that
 * takes the form with slot norms (tpq_ivfpq_scan_cell_norms is 1) and is handed kept_valid == 0 first writes the state, on
 * `stream`, then reads it; with kept_valid == 1 it only reads it: no parameter pass, no norm pass, no codebook
 * conversion.  The caller sets kept_valid = 1 for later calls while codes, codebook and tombstones are unchanged, and
 * orders calls on other streams behind the call that wrote the state.  Any other call ignores `kept` and writes nothing
 * to it, as does a call whose `kept` is NULL or smaller than the size above: those are tpq_ivfpq_search_fused_cells.  Same
 * results, bit for bit.  `kept` must be 16-byte aligned (the image is read with 16-byte loads; any other alignment is
 * rejected before anything is launched).  TPQ_VERSION is unchanged by these symbols.
 * tpq_ivfpq_scan_cell_inversions (diagnostics, host only): the count / scan / scatter chains the cell-major form has
 * launched in this process so far -- one per call of the seeded form and of the threshold form's one walk, two per call
 * of the threshold form beyond 8 192 cells. */
#define TPQ_HAS_IVFPQ_CELL_KEPT 1
size_t tpq_ivfpq_cell_kept_bytes(int64_t n_slots, int ds);
long long tpq_ivfpq_scan_cell_inversions(void);
int tpq_ivfpq_search_fused_cells_kept(const uint8_t* packed, const uint8_t* codes, const float* query,
                                      const float* codebook, int ds, int metric, const uint8_t* is_empty,
                                      const int64_t* cell_start, const int64_t* cell_size,
                                      const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                      const int64_t* address2id, int64_t* out_ids, int64_t n_slots,
                                      int nq, int max_nprobe, int m, int k, int n_split, void* workspace,
                                      size_t workspace_bytes, int32_t* tickets, int64_t slots_hint,
                                      const int64_t* cells, int n_cells, void* kept, size_t kept_bytes,
                                      int kept_valid, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * SURVEY 8(f)-3  residual-PQ list scan (pq_use_residual=True)
 * replaces IVFPQTopkCuda.topk_residual_precomputed  torchpq/kernels/IVFPQTopkCuda.py:212-283
 *          (kernel ivfpq_topk_residual_precomputed, torchpq/kernels/cuda/ivfpq_topk.cu:1039-1208)
 *      and IVFPQTopkCuda.topk_residual              torchpq/kernels/IVFPQTopkCuda.py:144-210
 *          (kernel ivfpq_topk_residual, ivfpq_topk.cu:973-1037)
 * value(slot of probe p) = base_sims[q][p]; then += LUT_p[j][code_j] for j ascending, with
 *   LUT_p = part1[q] + part2[cells[q][p]]  (part1 f32 [nq][m][256], part2 f32 [n_cells][m][256])
 *   or, when full_lut != NULL, LUT_p = full_lut[q][p]  (f32 [nq][max_nprobe][m][256]).
 * Other arguments and the output contract are those of tpq_ivfpq_scan_topk.
 * tpq_residual_part1: part1[q][j][c] = 2 * q_j . r_jc (index/IVFPQIndex.py:366-379).
 * ------------------------------------------------------------------------- */
int tpq_ivfpq_scan_topk_residual(const uint8_t* codes, const float* part1, const float* part2,
                                 const float* full_lut, const int64_t* cells,
                                 const float* base_sims, const uint8_t* is_empty,
                                 const int64_t* cell_start, const int64_t* cell_size,
                                 const int64_t* n_probe_list, float* out_vals, int64_t* out_addr,
                                 const int64_t* address2id, int64_t* out_ids, int64_t n_slots,
                                 int nq, int max_nprobe, int m, int k, tpq_stream_t stream);
int tpq_residual_part1(const float* query, const float* codebook, float* part1, int m, int ds,
                       int nq, tpq_stream_t stream);

/* Residual scan at the speed of the plain scan (same reference kernel, ivfpq_topk.cu:1039-1208,
 * same results bit for bit).  Only part1[q] lives in LDS (staged once per query, or built in the
 * workgroup from query [m*ds][nq] + codebook [m][ds][256] when part1 == NULL); the cell-dependent
 * half of the selection value is a per-slot constant:
 *   tpq_ivfpq_residual_slot_terms: slot_term f32 [n_slots] = sum_j part2[cell(s)][j][code_j(s)]
 *                                  cell_bound f32 [n_cells] = sum_j max_c |part2[cell][j][c]|
 * (derived from CellContainer._storage + part2; recompute after add/remove/expand).
 * Survivors are re-evaluated exactly (base_sims + fl(part1 + part2) ascending j); queries whose
 * candidate band overflows, or that list a cell twice, are redone by the exact kernel.
 * workspace: tpq_ivfpq_scan_workspace_bytes(nq, k, n_split, m).  m: any value of TPQ_PACKED_M_LIST. */
int tpq_ivfpq_residual_slot_terms(const uint8_t* codes, const float* part2,
                                  const int64_t* cell_start, const int64_t* cell_size,
                                  float* slot_term, float* cell_bound, int64_t n_slots,
                                  int n_cells, int m, tpq_stream_t stream);
int tpq_ivfpq_scan_topk_residual_packed(
    const uint8_t* packed, const uint8_t* codes, const float* part1, const float* query,
    const float* codebook, int ds, const float* part2, const float* slot_term,
    const float* cell_bound, const int64_t* cells, const float* base_sims, const uint8_t* is_empty,
    const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
    float* out_vals, int64_t* out_addr, const int64_t* address2id, int64_t* out_ids,
    int64_t n_slots, int nq, int max_nprobe, int m, int k, int n_split, void* workspace,
    size_t workspace_bytes, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * a-3  ADC look-up table
 * replaces PQCodec.precompute_adc  torchpq/codec/PQCodec.py:62-75
 *          (-> MultiKMeans.sim/euc_sim, torchpq/clustering/MultiKMeans.py:184-223)
 * query f32 [m*ds][nq], codebook f32 [m][ds][256] -> lut f32 [m][nq][256]
 * NEG_SQ_L2: lut = 2 q.c - |q|^2 - |c|^2 ; INNER: lut = q.c ; every dot/norm is an
 * ascending-dimension fp32 fma chain (exactly what v_mfma_f32_32x32x2_f32 computes).
 * ------------------------------------------------------------------------- */
int tpq_adc_lut(const float* query, const float* codebook, float* lut, int m, int ds, int nq,
                int metric, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * a-4  row-wise top-k (coarse probe select)
 * replaces fn.Topk.__call__        torchpq/fn/Topk.py:43-67
 *          Top1SelectCuda / Top32SelectCuda / TopkSelectCuda
 *          (torchpq/kernels/cuda/top1_select.cu:542, top32_select.cu:484-636,
 *           topk_select.cu:662-805)
 * x f32 [rows][cols] -> vals f32 [rows][k] descending, idx i64 [rows][k];
 * ties: smaller column first.  1 <= k <= min(cols, 1024).
 * ------------------------------------------------------------------------- */
int tpq_topk_select(const float* x, float* vals, int64_t* idx, int rows, int cols, int k,
                    tpq_stream_t stream);

/* a-4 fused: the epilogue of metric.negative_squared_l2_distance (torchpq/metric.py:89-96) applied
 * inside the select: v = (2*dots[r][c] - a2[r]) - b2[c] (the reference's rounding order), then
 * row top-k as above.  dots f32 [rows][cols] = x^T C (library GEMM), a2 [rows] = |x|^2,
 * b2 [cols] = |C|^2. */
int tpq_coarse_select(const float* dots, const float* a2, const float* b2, float* vals, int64_t* idx,
                      int rows, int cols, int k, tpq_stream_t stream);

/* a-4 + a-5 + the list-extent gathers in one call: the whole coarse step of IVFPQIndex.search
 * (torchpq/index/IVFPQIndex.py:486-512 and :425-426) as two launches -- an fp32-MFMA kernel that
 * writes sims = 2 x^T C - |x|^2 - |C|^2 (replaces the cuBLAS GEMM + 3 element-wise passes of
 * metric.negative_squared_l2_distance, torchpq/metric.py:31-98) into `workspace`, and the row
 * select whose epilogue also gathers cell_start/cell_size of the chosen cells and derives
 * n_probe_list (smart probing when smart_temperature > 0, else n_probe for every query).
 * query f32 [d][nq], centroids f32 [d][n_cells], cell_*_tbl i64 [n_cells]
 * -> topk_sims f32 [nq][n_probe] (descending), cells / cell_start / cell_size i64 [nq][n_probe],
 *    n_probe_list i64 [nq].   1 <= n_probe <= min(n_cells, 1024). */
/* The workspace need not be zeroed: similarities and group maxima are written before the row select reads them. */
size_t tpq_ivfpq_coarse_probe_workspace_bytes(int nq, int n_cells);
int tpq_ivfpq_coarse_probe(const float* query, const float* centroids,
                           const int64_t* cell_start_tbl, const int64_t* cell_size_tbl,
                           float* topk_sims, int64_t* cells, int64_t* cell_start,
                           int64_t* cell_size, int64_t* n_probe_list, int d, int nq, int n_cells,
                           int n_probe, float smart_temperature, void* workspace,
                           size_t workspace_bytes, tpq_stream_t stream);
/* The same call with the choice of the SELECTING arithmetic left to the caller (the result -- cells, order,
 * similarities -- is the fp32 kernel's, bit for bit, on every route).  The reference's reduced-precision coarse GEMM
 * (use_tensor_core / fp16_scale_mode, torchpq/metric.py:47-73, index/IVFPQIndex.py:98-125) trades accuracy for speed;
 * here the fp16 matrix cores only select: fast similarities of all (query, cell) pairs, a candidate band of twice a
 * rigorous error bound around the n_probe-th best, and the fp32 chain's own value for every candidate (d <= 128,
 * n_cells % 32 == 0; other shapes take the fp32 kernels on every route).
 *   TPQ_PROBE_ROUTE_AUTO  what tpq_ivfpq_coarse_probe does: the fp16 selection from 2 048 cells on (batches of more
 *                         than 256 queries; n_probe <= 112, or up to half the number of cell groups the pass keeps
 *                         maxima of -- 128 probes of 16 384 cells) and from 1 024 cells on for batches of >= 4 096
 *                         queries with n_probe <= 32, the fp32 kernels otherwise
 *   TPQ_PROBE_ROUTE_FP32  the fp32-MFMA similarity kernels
 *   TPQ_PROBE_ROUTE_FP16  the fp16 selection whenever the shape allows it
 * workspace: tpq_ivfpq_coarse_probe_route_workspace_bytes(d, nq, n_cells, route). */
#define TPQ_PROBE_ROUTE_AUTO 0
#define TPQ_PROBE_ROUTE_FP32 1
#define TPQ_PROBE_ROUTE_FP16 2
/* The workspace need not be zeroed, on either route (the fp16 pass clears its own counters on the stream). */
size_t tpq_ivfpq_coarse_probe_route_workspace_bytes(int d, int nq, int n_cells, int route);
int tpq_ivfpq_coarse_probe_route(const float* query, const float* centroids,
                                 const int64_t* cell_start_tbl, const int64_t* cell_size_tbl,
                                 float* topk_sims, int64_t* cells, int64_t* cell_start,
                                 int64_t* cell_size, int64_t* n_probe_list, int d, int nq, int n_cells,
                                 int n_probe, float smart_temperature, int route, const void* prepared,
                                 void* workspace, size_t workspace_bytes, tpq_stream_t stream);
/* What the fp16 selection needs of the CENTROIDS alone (their mean, the fp16 scale, MFMA fragments, row copies,
 * |C|^2) can be prepared once per codebook into a caller-owned block and handed to every call (`prepared`; NULL: it is
 * prepared into the workspace per call, ~0.1 ms at 16 384 cells).  tpq_ivfpq_coarse_probe_prepared_bytes is 0 for shapes
 * without the fp16 pass.  The block is only read by the probe calls. */
/* The prepared block need not be zeroed: tpq_ivfpq_coarse_probe_prepare clears its header on the stream and writes the rest. */
size_t tpq_ivfpq_coarse_probe_prepared_bytes(int d, int n_cells);
int tpq_ivfpq_coarse_probe_prepare(const float* centroids, int d, int n_cells, void* prepared,
                                   size_t prepared_bytes, tpq_stream_t stream);

/* a-5  smart probing          torchpq/index/IVFPQIndex.py:499-512
 * topk_sims f32 [rows][n_probe] -> n_probe_list i64 [rows] in [0, n_probe]
 * p = softmax(-sqrt(|s|)/T); H = -sum(p*log2(p)/log2(n_probe)); out = ceil(H*n_probe) */
int tpq_smart_probing(const float* topk_sims, int64_t* n_probe_list, int rows, int n_probe,
                      float temperature, tpq_stream_t stream);

/* id -> address, linear form (BaseContainer(use_inverse_id_mapping=False))
 * replaces get_address_by_id   torchpq/kernels/cuda/get_address_by_id.cu:8-44
 * (wrapper GetAddressByIdCuda, torchpq/container/BaseContainer.py:79-98): every id against every
 * stored id, O(n_ids x capacity); address[i] = smallest slot with address2id == ids[i], else -1
 * (negative ids are never found: free slots hold -1). */
int tpq_get_address_by_id(const int64_t* address2id, int64_t capacity, const int64_t* ids,
                          int64_t* address, int64_t n_ids, tpq_stream_t stream);

/* a-7  address -> id           torchpq/container/BaseContainer.py:58-65 */
int tpq_get_id_by_address(const int64_t* address2id, int64_t capacity, const int64_t* address,
                          int64_t* ids, int64_t n, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * a-8  k-means assign / PQ encode: batched arg-max similarity
 * replaces MaxSimCuda.__call__(A, B, dim=2, mode="tn")
 *          torchpq/kernels/MaxSimCuda.py:184-238,296-340; kernel max_sim_tn
 *          torchpq/kernels/cuda/max_sim.cu:182-309
 * A f32 [l][d][m] (data), B f32 [l][d][n] (centroids)
 *   -> vals f32 [l][m], inds i64 [l][m]  (arg-max over the n centroids)
 * NEG_SQ_L2: sim = 2 a.b - |a|^2 - |b|^2, INNER: sim = a.b, dots = ascending-d fp32 fma
 * chains on the fp32 MFMA.  Ties -> smallest centroid index (the reference's cross-block
 * arg-max is a benign race, max_sim.cu:152-180).
 * ------------------------------------------------------------------------- */
int tpq_max_sim(const float* A, const float* B, float* vals, int64_t* inds, int l, int d, int m,
                int n, int metric, tpq_stream_t stream);

/* a-8 (training path)  the same (max, arg-max) on the bf16 matrix cores with fp32-level accuracy
 * replaces the max_sim call of the Lloyd loop, torchpq/clustering/MultiKMeans.py:415-453
 *          (get_labels :301-333 -> MaxSimCuda, kernel max_sim_tn torchpq/kernels/cuda/max_sim.cu:182-309)
 * Every fp32 operand is split exactly into three bf16 pieces and the six piece products of order
 * <= 4 are accumulated in fp32 on v_mfma_f32_32x32x16_bf16: |error of a.b| <= 2^-23 sum|a_k b_k| from
 * the dropped products plus fp32 accumulation rounding -- the accuracy class of the fp32 fma
 * chain, but not its bits: near-ties (relative gap < ~1e-6) may pick a different index than
 * tpq_max_sim.  Shapes: d <= 64, any n (256 centroids per pass), padded slice 16 ceil(d/16) m
 * floats < 2 GiB (tpq_max_sim_split_supported); otherwise TPQ_ERR_UNSUPPORTED. */
int tpq_max_sim_split_supported(int d, int64_t m, int n);
int tpq_max_sim_split(const float* A, const float* B, float* vals, int64_t* inds, int l, int d, int m,
                      int n, int metric, tpq_stream_t stream);

/* a-8 / a-11 (encode path)  the labels of tpq_max_sim, bit for bit, at bf16-matrix-core speed
 * replaces the max_sim call behind VQCodec.encode / IVFPQIndex.add (coarse assign):
 *          torchpq/index/IVFPQIndex.py:233-256 -> clustering/KMeans.py:440-452 (predict)
 *          -> kernels/MaxSimCuda.py:296-340, kernel max_sim_tn torchpq/kernels/cuda/max_sim.cu:182-309
 * A f32 [d][m] points, B f32 [d][n] centroids (one problem) -> inds i64 [m] = arg-max over the
 * centroids of the oracle's fp32 arithmetic (ascending-k fmaf chains; ties -> smallest index).
 * An error-bounded top-2 selection decides every point whose two best fast values differ by more
 * than twice the bound; the others are re-evaluated exactly on the device.  Euclidean problems with
 * >= 4 096 centroids: the points are prepared per call as tpq_lloyd_prepare does, one fp16 product
 * against the centroids in chunks of 256 decides 90-95 % of them, and the rest get the exact kernel's
 * own value for each of their CANDIDATES (the 2-3 centroids within twice the bound of the best);
 * the others the two-piece bf16 selection with the exact kernel over what it leaves.
 * vals (optional, f32 [m]): the maximum itself -- the FAST value (within the bound, ~1e-5 of the
 * scale) for points decided by the selection, the exact one for re-checked points: good for an
 * inertia, not for bit comparisons.
 * Wide vectors, 128 < d <= 1024 (GIST: 960), both metrics: fp16 selection GEMM-shaped (256 x 256 tiles,
 * both operands through LDS), and the exact step runs on CANDIDATES -- for every undecided point the (2-3)
 * centroids within twice the bound of its best get the exact kernel's own value (same instruction
 * sequence), never all n of them; candidate lists that overflow (degenerate data) fall back to the
 * exact kernel.  Problems below 2^33 multiply-adds go to tpq_max_sim directly (same labels).
 * Shapes: d <= 128: m < 2^31, padded slice 16 ceil(d/16) m floats < 2 GiB; 128 < d <= 1024: m < 2^28,
 * n <= 2^22 (workspace ~1.4 x the points); otherwise TPQ_ERR_UNSUPPORTED (use tpq_max_sim).
 * workspace: tpq_coarse_assign_workspace_bytes(d, m, n).
 * tpq_coarse_assign_route: the same call with the choice between the paths made by the caller instead of
 * the size thresholds above -- TPQ_ASSIGN_ROUTE_AUTO (what tpq_coarse_assign does) or
 * TPQ_ASSIGN_ROUTE_CASCADE (the fp16 cascade for every shape it supports, however small: the parity tests
 * drive it over ragged and degenerate shapes this way).  Labels are the same on every route.
 * workspace: tpq_coarse_assign_route_workspace_bytes(d, m, n, route). */
#define TPQ_ASSIGN_ROUTE_AUTO 0
#define TPQ_ASSIGN_ROUTE_CASCADE 1
int tpq_coarse_assign_supported(int d, int64_t m, int n);
/* The workspace need not be zeroed: every counter and flag of the route taken is cleared on the stream by the call. */
size_t tpq_coarse_assign_workspace_bytes(int d, int64_t m, int n);
/* diagnostics: byte offset inside the workspace of the int32 count of points the last call
 * re-checked exactly (d > 128: points that got an exact step on their candidates) */
size_t tpq_coarse_assign_count_offset(int d, int64_t m, int n);
int tpq_coarse_assign(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n,
                      int metric, void* workspace, size_t workspace_bytes, tpq_stream_t stream);
/* The workspace need not be zeroed: every counter and flag of the route taken is cleared on the stream by the call. */
size_t tpq_coarse_assign_route_workspace_bytes(int d, int64_t m, int n, int route);
int tpq_coarse_assign_route(const float* A, const float* B, float* vals, int64_t* inds, int d, int64_t m, int n,
                            int metric, int route, void* workspace, size_t workspace_bytes, tpq_stream_t stream);

/* a-8 (training path, batched)  the labels of tpq_max_sim, bit for bit, for l codebook-sized problems
 * replaces the max_sim call of the Lloyd loop, torchpq/clustering/MultiKMeans.py:415-453
 * A f32 [l][d][m], B f32 [l][d][n], n <= 256, d <= 64 -> inds i64 [l][m] (exact) and, optionally, vals
 * f32 [l][m] (the selection's fast maxima, ~1e-5 of the scale; exact for re-checked points).
 * The error-bounded bf16 top-2 selection + exact re-check of tpq_coarse_assign with the centroids
 * resident in LDS and the points streamed (the PQ-codebook training shape, configs[4]).
 * workspace: tpq_max_sim_select_workspace_bytes(l, d, m, n) (dominated by the l x m int32 lists). */
int tpq_max_sim_select_supported(int l, int d, int64_t m, int n);
/* The workspace need not be zeroed, and may be the one an earlier call used: maxima, counts and means are cleared by the call. */
size_t tpq_max_sim_select_workspace_bytes(int l, int d, int64_t m, int n);
int tpq_max_sim_select(const float* A, const float* B, float* vals, int64_t* inds, int l, int d, int64_t m,
                       int n, int metric, void* workspace, size_t workspace_bytes, tpq_stream_t stream);

/* a-8 + a-9 on PREPARED data: one Lloyd iteration of the PQ-codebook training shape
 * replaces, per iteration, the get_labels -> compute_centroids pair of the reference's driver
 *          torchpq/clustering/MultiKMeans.py:415-453 (max_sim_tn, kernels/cuda/max_sim.cu:182-309;
 *          compute_centroids, kernels/cuda/compute_centroids.cu:10-86)
 * tpq_lloyd_prepare (once per fit: the data never changes, only the centroids do):
 *   data f32 [l][d][m], centroids0 f32 [l][d][n] (the initial centroids; their mean is the centring
 *   vector) -> `prepared`: every point centred, scaled by a power of two per sub-problem and split
 *   into two fp16 pieces in MFMA-fragment order (4 bytes per element, as the fp32 original), plus
 *   |a'|^2, |x|^2 per point, the centring vector, the scale and a not-finite / out-of-range flag per
 *   sub-problem.  prepared_bytes >= tpq_lloyd_prepared_bytes(l, d, m) (~ the size of data).
 * tpq_lloyd_step: centroids f32 [l][d][n] -> inds i64 [l][m] = the labels of tpq_max_sim, BIT FOR BIT
 *   (error-bounded top-2 selection on the fp16 matrix cores + exact fp32 re-check of the ambiguous
 *   points on `data`), vals (optional) f32 [l][m] = the maxima (fast values, ~1e-6 of the scale; exact
 *   for re-checked points), new_centroids (optional) f32 [l][d][n] = tpq_compute_centroids of those
 *   labels (empty cluster -> 0).  A sub-problem whose data or centroids are not finite / leave the
 *   fp16 range is handled entirely by the exact path (same results, slower).
 * Shapes: d <= 64, n <= 256, slices below 2 GiB (tpq_lloyd_supported); euclidean only. */
int tpq_lloyd_supported(int l, int d, int64_t m, int n);
/* The prepared block need not be zeroed: tpq_lloyd_prepare clears means, scales and flags on the stream and writes the rest. */
size_t tpq_lloyd_prepared_bytes(int l, int d, int64_t m);
int tpq_lloyd_prepare(const float* data, const float* centroids0, void* prepared, size_t prepared_bytes,
                      int l, int d, int64_t m, int n, tpq_stream_t stream);
/* The workspace need not be zeroed, and serves step after step: maxima, counts, flags and the sums are cleared by every call. */
size_t tpq_lloyd_step_workspace_bytes(int l, int d, int64_t m, int n);
/* diagnostics: byte offset inside the workspace of the int32 [l] counts of points left undecided by
 * level 1 (the one-product coarse pass) / level 2 (the three-product pass; = re-checked exactly) */
size_t tpq_lloyd_step_count_offset(int l, int d, int64_t m, int n, int level);
int tpq_lloyd_step(const float* data, const void* prepared, const float* centroids, float* new_centroids,
                   float* vals, int64_t* inds, int l, int d, int64_t m, int n, void* workspace,
                   size_t workspace_bytes, tpq_stream_t stream);

/* a-9  k-means update
 * replaces ComputeCentroidsCuda.__call__  torchpq/kernels/ComputeCentroidsCuda.py:43-81
 *          kernel compute_centroids       torchpq/kernels/cuda/compute_centroids.cu:10-86
 * data f32 [l][d][n], labels i64 [l][n] -> centroids f32 [l][d][k]; empty cluster -> 0.
 * workspace: tpq_compute_centroids_workspace_bytes(l, d, k) (zeroed by the call).
 * Non-finite data (documented divergence): for k <= 256, d >= 32 the sums run as one-hot x data on
 * the bf16 matrix cores, where a NaN / Inf coordinate reaches every cluster of its 16-point group
 * through 0 * x (up to 256 centroids turn NaN in that dimension); the scalar kernels used for the
 * other shapes, and the reference, confine it to the point's own cluster.  Finite inputs are
 * unaffected; callers that may hold NaN / Inf must sanitise the data first. */
/* The workspace need not be zeroed: the call clears the sums and counts on the stream. */
size_t tpq_compute_centroids_workspace_bytes(int l, int d, int k);
int tpq_compute_centroids(const float* data, const int64_t* labels, float* centroids, int l, int d,
                          int64_t n, int k, void* workspace, size_t workspace_bytes,
                          tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * a-12 / a-14  container placement
 * tpq_get_ioa           replaces GetIOACuda            torchpq/kernels/cuda/get_ioa.cu:9-47
 *   ioa[i] = number of j < i with labels[j] == labels[i] (input order).
 *   workspace: tpq_get_ioa_workspace_bytes(n) bytes.
 * tpq_get_write_address replaces GetWriteAddressV2Cuda torchpq/kernels/cuda/get_write_address_v2.cu:9-41
 *   the ioa-th empty slot within [cell_start, cell_start+cell_capacity) of the label's cell, -1 if none.
 * tpq_get_cell_by_address replaces GetDivByAddressV2Cuda torchpq/kernels/cuda/get_div_by_address_v2.cu:9-95
 *   cell whose [start, start+capacity) contains the address, else -1 (cells ordered by start).
 * ------------------------------------------------------------------------- */
/* The workspace need not be zeroed: keys and positions are written for all n labels before the sort reads them. */
size_t tpq_get_ioa_workspace_bytes(int64_t n);
int tpq_get_ioa(const int64_t* labels, int64_t* ioa, int64_t n, int64_t n_cells, void* workspace,
                size_t workspace_bytes, tpq_stream_t stream);
int tpq_get_write_address(const uint8_t* is_empty, const int64_t* cell_start,
                          const int64_t* cell_capacity, const int64_t* labels, const int64_t* ioa,
                          int64_t* write_address, int64_t n_slots, int64_t n_labels,
                          tpq_stream_t stream);
int tpq_get_cell_by_address(const int64_t* address, const int64_t* cell_start,
                            const int64_t* cell_capacity, int64_t* cells, int64_t n_address,
                            int64_t n_cells, tpq_stream_t stream);

/* a-6  expand: re-lay the lists out for larger per-cell capacities
 * replaces CellContainer.expand  torchpq/container/CellContainer.py:249-311 (a torch.cat of the whole
 * storage per expanding cell).  Cell c moves from [old_start[c], + old_capacity[c]) to
 * [new_start[c], + new_capacity[c]) (new_capacity >= old_capacity, new_start = exclusive prefix sum
 * of new_capacity); the added tail of every cell is initialised free (codes 0, id -1, is_empty 1).
 * storage u8 [m/4][old_slots][4] -> new_storage u8 [m/4][new_slots][4]; the new buffers need no
 * initialisation by the caller. */
int tpq_grow_cells(const uint8_t* storage, const int64_t* address2id, const uint8_t* is_empty,
                   const int64_t* old_start, const int64_t* old_capacity, const int64_t* new_start,
                   const int64_t* new_capacity, uint8_t* new_storage, int64_t* new_address2id,
                   uint8_t* new_is_empty, int64_t old_slots, int64_t new_slots, int n_cells, int m,
                   tpq_stream_t stream);

/* a-13  PQ decode   replaces PQDecodeCuda  torchpq/kernels/cuda/pq_decode.cu:8-53
 * codebook f32 [m][ds][256], codes u8 [m][n] -> out f32 [m*ds][n] */
int tpq_pq_decode(const float* codebook, const uint8_t* codes, float* out, int m, int ds, int64_t n,
                  tpq_stream_t stream);

/* codes u8 [m][n] scattered into _storage [m/4][n_slots][4] at address[i]
 * (CellContainer.set_data_by_address, torchpq/container/CellContainer.py:213-239);
 * when `packed` is non-NULL the scan-layout copy is updated in the same pass. */
int tpq_scatter_codes(const uint8_t* codes, const int64_t* address, uint8_t* storage,
                      uint8_t* packed, int m, int64_t n, int64_t n_slots, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFPQRIndex re-rank step (Jegou et al., "Searching in one billion vectors: re-rank with source coding")
 * stands in for IVFPQR.topk's second half   torchpq/legacy/IVFPQR.py:408-473
 * (the reference's new-API class, torchpq/index/IVFPQRIndex.py, has no search).
 *
 * storage      u8  [(m+m_r)/4][capacity][4]  rows 0..m-1 the first-stage code, rows m..m+m_r-1 the re-rank code
 * codebook     f32 [m][ds][256]     first-stage codebook (ds = d/m); may be NULL when !use_residual
 * codebook_r   f32 [m_r][ds_r][256] re-rank codebook (ds_r = d/m_r)
 * query        f32 [d][nq]          (pre-normalised by the host for TPQ_METRIC_INNER)
 * cand_address i64 [nq][k1]         candidates of the list scan; < 0 or >= capacity = none
 * out_vals f32 / out_address i64 / out_ids i64 [nq][k]; address2id and out_ids are both given or both NULL.
 *
 * Value of a candidate with codes c[0..m), c_r[0..m_r) (all fp32, no fma unless stated, i ascending):
 *   use_residual:  r_i = codebook[i/ds][i%ds][c[i/ds]] + codebook_r[i/ds_r][i%ds_r][c_r[i/ds_r]];
 *       TPQ_METRIC_NEG_SQ_L2:  t = q_i - r_i;  acc = acc - t*t      (acc starts at 0.f)
 *       TPQ_METRIC_INNER:      acc = acc + q_i * r_i
 *   !use_residual: v = 0.f; for j ascending: v += LUT_r[j][c_r[j]], LUT_r the table tpq_adc_lut builds from
 *       codebook_r (fma chains over the sub-vector; 2*dot - |q_j|^2 - |c|^2 for the L2 metric), built in the kernel.
 * Output per query: the k best candidates by (value descending, address ascending); positions beyond the
 * real candidates are (-inf, -1, -1); a real candidate whose value is -inf keeps its address and id and stands
 * ahead of them.  A query with a NaN or +-Inf component (or one whose products overflow) still returns: its own
 * row then holds, in no pinned order, -1 or candidates of that row, none more often than cand_address names it,
 * and the rows of the finite queries are what they are without it.  1 <= k <= k1 <= 1024 and capacity < 2^31 - 1, else TPQ_ERR_UNSUPPORTED;
 * storage and the codebooks are 16-byte aligned.  No workspace.
 * ------------------------------------------------------------------------- */
int tpq_ivfpqr_rerank(const uint8_t* storage, int64_t capacity, int m, int m_r, const float* codebook,
                      const float* codebook_r, const float* query, int d, int nq, const int64_t* cand_address,
                      int k1, int k, int use_residual, int distance, const int64_t* address2id, float* out_vals,
                      int64_t* out_address, int64_t* out_ids, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFFlatIndex list scan + top-k: the probed cells hold the vectors themselves (no reference counterpart; the
 * index every IVF library ships between exact search and IVFPQ).
 *
 * vectors      f32 [d][n_slots]     dimension-major, slot-contiguous: CellContainer._storage of code_size = 4 d
 *                                   (u8 [d][n_slots][4]) read as fp32 -- row i holds the four bytes of component i
 * query        f32 [d][nq]          (pre-normalised by the host for TPQ_METRIC_INNER)
 * is_empty     u8  [n_slots] or NULL  a mask: any set of slots the caller wants skipped (non-zero = skip), one for
 *                                   the whole call -- the container's tombstones, or those OR-ed with the
 *                                   complement of a filter (IVFFlatIndex.search_filtered).  The byte of a slot is
 *                                   read before any of its 4 d bytes of vector: a 64-slot tile without a live slot
 *                                   is not read, a tile with a few live slots is not read either -- its live slots
 *                                   are gathered with those of other such tiles, 64 at a time -- and in any other
 *                                   tile only the live slots' vectors are.  NULL: no slot is skipped, no mask read
 * cell_start / cell_size i64 [nq][max_nprobe]; n_probe_list i64 [nq], clamped to [0, max_nprobe]; a probe whose
 *              start equals the previous probe's start is skipped, as in tpq_ivfpq_scan_topk
 * out_vals f32 / out_addr i64 [nq][k]
 *
 * Value of a slot with vector x (all fp32, no fma, i ascending, acc starts at 0.f):
 *       TPQ_METRIC_NEG_SQ_L2:  t = q_i - x_i;  acc = acc - t*t
 *       TPQ_METRIC_INNER:      acc = acc + q_i * x_i
 * Output per query: the k best live slots of its probed cells by (value descending, address ascending);
 * tombstoned slots, slots outside [start, start + size) or outside the storage, and slots whose value is NaN never
 * enter; positions beyond the candidates are (-inf, -1); a slot whose value is -inf keeps its address and stands
 * ahead of them.  A query with a NaN or +-Inf component (or one whose products overflow) still returns: which slots
 * its own row holds is not pinned, and the rows of the other queries are what they are without it.
 * 1 <= k <= 1024; n_slots < 2^31 - 1, else TPQ_ERR_UNSUPPORTED; any d >= 1 (the only LDS that grows with d is the
 * query itself).  n_split >= 1 workgroups share a query's tiles (small batches; the caller picks it from nq and
 * the CU count) and a second launch merges their lists through the caller's workspace of
 * tpq_ivfflat_scan_workspace_bytes(nq, k, n_split) bytes (0 when n_split == 1).  The library allocates nothing.
 * ------------------------------------------------------------------------- */
/* The workspace need not be zeroed: every workgroup writes its whole list (pads included) before the merge reads it. */
size_t tpq_ivfflat_scan_workspace_bytes(int nq, int k, int n_split);
int tpq_ivfflat_scan_topk(const float* vectors, const float* query, const uint8_t* is_empty,
                          const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                          float* out_vals, int64_t* out_addr, int64_t n_slots, int d, int nq, int max_nprobe, int k,
                          int metric, int n_split, void* workspace, size_t workspace_bytes, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFPQ4Index list scan + top-k: product-quantized lists with 16 centroids per sub-quantizer (4-bit codes; the
 * reference began such a path, top-1 only, and has no index for it).
 *
 * Codes        m sub-quantizers, m % 8 == 0, 8 <= m <= 256, sub-vector length ds = d / m >= 1, 16 centroids each.
 *              A vector's code is m / 2 bytes: byte b holds sub-quantizer 2 b in bits 0-3 and sub-quantizer 2 b + 1
 *              in bits 4-7.
 * codes        u8 [m / 8][n_slots][4]: CellContainer._storage of code_size = m / 2, contiguous_size = 4.  Read as
 *              32-bit little-endian words it is [m / 8][n_slots]: word w of slot s holds sub-quantizers 8 w ... 8 w + 7,
 *              lowest nibble first.
 * query        f32 [d][nq], d = m * ds (pre-normalised by the host for TPQ_METRIC_INNER)
 * codebook     f32 [m][ds][16]
 * is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr, n_slots, nq, max_nprobe, k, n_split, workspace:
 *              as tpq_ivfflat_scan_topk
 *
 * Table entry of sub-quantizer j and centroid c (all fp32, no fma, i ascending, e starts at 0.f):
 *       TPQ_METRIC_NEG_SQ_L2:  t = q[j*ds + i] - codebook[j][i][c];  e = e - t*t
 *       TPQ_METRIC_INNER:      e = e + q[j*ds + i] * codebook[j][i][c]
 * -- the arithmetic of tpq_ivfflat_scan_topk's value over the sub-vector; NOT the 2 q.c - |q|^2 - |c|^2 form of
 * tpq_adc_lut.  The table (m x 16 floats per query) is built inside the scan workgroup and never exists in memory.
 * Value of a slot:  v = 0.f;  for j = 0 ... m - 1 ascending:  v = v + table[j][code_j]  (one fp32 add per step).
 * Candidates, order and padding are exactly those of tpq_ivfflat_scan_topk: the first n_probe_list[q] cells
 * (clamped to [0, max_nprobe]); a probe whose start equals the previous probe's start is skipped; slots outside the
 * storage are cut; tombstones are skipped when is_empty is given; a NaN value never enters; the k best by (value
 * descending, address ascending); (-inf, -1) beyond them.  The result does not depend on n_split.
 * An m outside the above, ds < 1 or a k outside [1, 1024] returns TPQ_ERR_UNSUPPORTED (as does n_slots >= 2^31 - 1,
 * or a d / max_nprobe whose query and probe table do not fit the LDS next to the table); nothing is launched.
 * Workspace: tpq_ivfpq4_scan_workspace_bytes(nq, k, n_split) bytes (0 when n_split == 1).  The library allocates nothing.
 * ------------------------------------------------------------------------- */
/* The workspace need not be zeroed: every workgroup writes its whole list (pads included) before the merge reads it. */
size_t tpq_ivfpq4_scan_workspace_bytes(int nq, int k, int n_split);
int tpq_ivfpq4_scan_topk(const uint8_t* codes, const float* query, const float* codebook, const uint8_t* is_empty,
                         const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                         float* out_vals, int64_t* out_addr, int64_t n_slots, int m, int ds, int nq, int max_nprobe,
                         int k, int metric, int n_split, void* workspace, size_t workspace_bytes,
                         tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFPQ4Index list scan + top-k over RESIDUAL codes (IVFPQ4Index(pq_use_residual=True)): a slot of cell c holds the
 * 4-bit code of x - centroid(c), so the table depends on the probe.  No reference counterpart.
 *
 * codes, query, codebook, is_empty, cell_start, cell_size, n_probe_list, out_vals, out_addr, n_slots, m, ds, nq,
 * max_nprobe, k, metric, n_split, workspace: as tpq_ivfpq4_scan_topk
 * centroids    f32 [n_cells][d], cell-major: one centroid is one contiguous row (the TRANSPOSE of the coarse
 *              codebook [d][n_cells] of tpq_ivfpq_coarse_probe)
 * cells        i64 [nq][max_nprobe]: the probed cells, in the positions of cell_start / cell_size
 *
 * All fp32, no fma, each operation rounded on its own.  Reconstruction of dimension j*ds + i of a code of probe p
 * whose sub-quantizer j holds centroid index c:
 *       y = centroids[cells[q][p]][j*ds + i] + codebook[j][i][c]                     (one add)
 * Table entry of (p, j, c), i ascending, e starts at 0.f:
 *       TPQ_METRIC_NEG_SQ_L2:  t = q[j*ds + i] - y;  e = e - t*t
 *       TPQ_METRIC_INNER:      e = e + q[j*ds + i] * y
 * Value of a slot scanned under probe p:  v = 0.f;  for j = 0 ... m - 1 ascending:  v = v + table_p[j][code_j].
 * So the value is the metric between the query and the vector centroid + codeword, summed sub-vector by sub-vector;
 * with all-zero centroids it is tpq_ivfpq4_scan_topk's, bit for bit.  The tables (m x 16 floats per query and probe)
 * are built inside the scan workgroup, once per scanned probe and part, and never exist in memory.
 * Candidates, the skipped duplicate probe, the cut at the storage, tombstones, the exclusion of NaN values, the order
 * (value descending, address ascending), the padding and the independence of n_split are exactly those of
 * tpq_ivfpq4_scan_topk (a slot of two overlapping cells is valued under each probe that scans it).
 * A cell index outside [0, n_cells) in a scanned probe is the caller's error; it is clamped into the range, so nothing
 * outside `centroids` is read.  Unsupported shapes as tpq_ivfpq4_scan_topk (the LDS holds two buffers of up to eight
 * tables here, 64 KiB at most, next to the query); n_cells < 1 or a null centroids / cells is TPQ_ERR_INVALID_ARGUMENT; nothing is launched.
 * Workspace: tpq_ivfpq4_scan_workspace_bytes(nq, k, n_split) bytes.  The library allocates nothing.
 * ------------------------------------------------------------------------- */
int tpq_ivfpq4_scan_residual_topk(const uint8_t* codes, const float* query, const float* codebook,
                                  const float* centroids, const int64_t* cells, int n_cells, const uint8_t* is_empty,
                                  const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                  float* out_vals, int64_t* out_addr, int64_t n_slots, int m, int ds, int nq,
                                  int max_nprobe, int k, int metric, int n_split, void* workspace,
                                  size_t workspace_bytes, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFFlatIndex range search: every stored vector of the probed cells whose value reaches a threshold (no
 * reference counterpart).  vectors, query, is_empty, cell_start, cell_size, n_probe_list, n_slots, d, nq,
 * max_nprobe, metric and n_split are those of tpq_ivfflat_scan_topk.
 *
 * Value      of a slot: exactly the value tpq_ivfflat_scan_topk defines (acc = 0.f, i ascending,
 *            acc = acc - t*t with t = q_i - x_i, or acc = acc + q_i*x_i; one fp32 operation per step, no fma).
 * Candidates of a query: those of tpq_ivfflat_scan_topk -- its first n_probe_list[q] cells (clamped to
 *            [0, max_nprobe]), a probe whose start equals the previous probe's start skipped, the slots inside
 *            [start, start + size) and inside the storage that are not tombstoned.
 * Hit        a candidate with value >= threshold[q] (threshold f32 [nq]).  A NaN value is never a hit, a NaN
 *            threshold gives no hits, -inf gives every candidate whose value is not NaN.
 * Order      scan order: probe rank ascending, then address ascending; a slot of two overlapping cells appears
 *            twice, as it does in the top-k scan.  The order does not depend on n_split.
 * Output     lims i64 [nq + 1], lims[0] = 0: the hits of query q are out_vals[lims[q] : lims[q+1]] (f32) and
 *            out_addr[lims[q] : lims[q+1]] (i64).
 * A query with a NaN or +-Inf component returns what this definition gives (usually nothing) and touches no
 * other query's segment.
 *
 * Two passes, no global atomics, no sort, deterministic.  A query's tiles are cut into n_split parts as in the
 * top-k scan, a part's tiles into eight contiguous chunks, one per wave: segment (q * n_split + part) * 8 + wave.
 *   1. tpq_ivfflat_range_count writes the hits of every segment: wave_counts i32
 *      [tpq_ivfflat_range_segments(nq, n_split)] (= nq * n_split * 8; 0 for nq <= 0 or n_split outside [1, 1024]).
 *   2. THE CALLER turns the counts into exclusive prefix sums: wave_offsets i64 [segments + 1], wave_offsets[0] = 0,
 *      the last entry the total number of hits, which sizes out_vals / out_addr; lims[q] = wave_offsets[q * n_split
 *      * 8].  The library does not do this step and allocates nothing.
 *   3. tpq_ivfflat_range_fill, with the inputs of the count pass, computes the values again (the same code, the
 *      same bits) and stores segment s at wave_offsets[s] onwards.  A wave stores nothing at or beyond
 *      wave_offsets[s + 1], whatever it finds: inputs that changed between the passes lose hits, they do not
 *      become a store outside the segment.  A segment without hits is not scanned again.
 * 1 <= n_split <= 1024; n_slots < 2^31 - 1, else TPQ_ERR_UNSUPPORTED; any d >= 1.  nq == 0 is TPQ_OK.
 * ------------------------------------------------------------------------- */
size_t tpq_ivfflat_range_segments(int nq, int n_split);
int tpq_ivfflat_range_count(const float* vectors, const float* query, const uint8_t* is_empty,
                            const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                            const float* threshold, int32_t* wave_counts, int64_t n_slots, int d, int nq,
                            int max_nprobe, int metric, int n_split, tpq_stream_t stream);
int tpq_ivfflat_range_fill(const float* vectors, const float* query, const uint8_t* is_empty,
                           const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                           const float* threshold, const int64_t* wave_offsets, float* out_vals, int64_t* out_addr,
                           int64_t n_slots, int d, int nq, int max_nprobe, int metric, int n_split,
                           tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFPQIndex range search: every stored code of the probed cells whose ADC value reaches a threshold (no
 * reference counterpart).  codes, is_empty, cell_start, cell_size, n_probe_list, n_slots, nq, max_nprobe, m and
 * n_split are those of tpq_ivfpq_scan_topk; the scan reads the reference layout, codes u8 [m/4][n_slots][4].
 *
 * Candidates of a query: those of tpq_ivfpq_scan_topk -- its first n_probe_list[q] probes (clamped to
 *            [0, max_nprobe]), a probe whose start equals the previous probe's start skipped, the slots inside
 *            [start, start + size) and inside [0, n_slots) (a cell that leaves the storage is cut) that are not
 *            tombstoned (is_empty).
 * Value      plain PQ: v = 0.f; for j = 0..m-1 ascending: v += lut[j][q][code_j], one fp32 add per step -- the value
 *            of tpq_ivfpq_scan_topk.  The table is either `lut` f32 [m][nq][256] (tpq_adc_lut's output) or, when
 *            lut == NULL, built in the workgroup from query f32 [m*ds][nq], codebook f32 [m][ds][256], ds and
 *            metric, as tpq_ivfpq_search_fused does: bit-identical entries.
 *            residual PQ: the value of tpq_ivfpq_scan_topk_residual -- v = base_sims[q][p], then v += LUT_p[j][code_j]
 *            for j ascending, with LUT_p[j][c] = part1[q][j][c] + part2[cells[q][p]][j][c] (one fp32 add per entry),
 *            or LUT_p = full_lut[q][p] when full_lut is given; when part1 == NULL (and full_lut == NULL) part1 is
 *            built in the workgroup from query and codebook (2 q_j . r_jc, the entries of tpq_residual_part1).  The
 *            value stored is v + 0.0f, as in the top-k scan: a range hit and a top-k result of one slot carry the
 *            same bits.
 * Hit        a candidate with value >= threshold[q] (threshold f32 [nq]).  A NaN value is never a hit, a NaN
 *            threshold gives no hits, -inf gives every candidate whose value is not NaN.
 * Order      scan order: probe rank ascending, then address ascending; a slot of two overlapping cells appears
 *            twice.  Neither the order nor the bits depend on how the work is cut (n_split).
 * Output     lims i64 [nq + 1], lims[0] = 0: the hits of query q are out_vals[lims[q] : lims[q+1]] (f32) and
 *            out_addr[lims[q] : lims[q+1]] (i64).
 * A query with a NaN or +-Inf component returns what this definition gives and touches no other query's segment.
 *
 * Two passes, no global atomics, no sort, deterministic -- the protocol of tpq_ivfflat_range_count / _fill.
 *   plain     a query's tiles are cut into n_split parts as in the top-k scan, a part's tiles into eight contiguous
 *             chunks, one per wave: segment (q * n_split + part) * 8 + wave; tpq_ivfpq_range_segments(nq, n_split)
 *             = nq * n_split * 8 segments (0 for nq <= 0 or n_split outside [1, 1024]).
 *   residual  the table depends on the probed cell: one workgroup per (query, probe rank), the cell's tiles in eight
 *             contiguous chunks: segment (q * max_nprobe + p) * 8 + wave; tpq_ivfpq_range_residual_segments(nq,
 *             max_nprobe) = nq * max_nprobe * 8 segments (0 for nq <= 0 or max_nprobe < 1).  A probe that is not
 *             scanned has eight zero counts.
 *   1. the count pass writes the hits of every segment: wave_counts i32 [segments].
 *   2. THE CALLER turns the counts into exclusive prefix sums: wave_offsets i64 [segments + 1], wave_offsets[0] = 0,
 *      the last entry the total number of hits, which sizes out_vals / out_addr; lims[q] = wave_offsets[q * (segments
 *      / nq)].  The library does not do this step and allocates nothing.
 *   3. the fill pass, with the inputs of the count pass, computes the values again (the same code, the same bits)
 *      and stores segment s at wave_offsets[s] onwards.  A wave stores nothing at or beyond wave_offsets[s + 1],
 *      whatever it finds: inputs that changed between the passes lose hits, they do not become a store outside the
 *      segment.  A segment without hits is not scanned again, a workgroup without hits stages no table.
 * m % 4 == 0 and 1 <= n_split <= 1024, else TPQ_ERR_INVALID_ARGUMENT; n_slots < 2^31 - 1 and the workgroup's LDS
 * (m KiB of table, the staged query when the table is built there, the probe table) <= 160 KiB -- m <= 156 -- else
 * TPQ_ERR_UNSUPPORTED.  nq == 0 is TPQ_OK.  Every check comes before the first HIP call.  There is no scan-layout
 * ("packed") route: the range scan reads `codes` whatever the index keeps for its top-k search.
 * ------------------------------------------------------------------------- */
size_t tpq_ivfpq_range_segments(int nq, int n_split);
int tpq_ivfpq_range_count(const uint8_t* codes, const float* lut, const float* query, const float* codebook, int ds,
                          int metric, const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                          const int64_t* n_probe_list, const float* threshold, int32_t* wave_counts, int64_t n_slots,
                          int nq, int max_nprobe, int m, int n_split, tpq_stream_t stream);
int tpq_ivfpq_range_fill(const uint8_t* codes, const float* lut, const float* query, const float* codebook, int ds,
                         int metric, const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                         const int64_t* n_probe_list, const float* threshold, const int64_t* wave_offsets,
                         float* out_vals, int64_t* out_addr, int64_t n_slots, int nq, int max_nprobe, int m,
                         int n_split, tpq_stream_t stream);
size_t tpq_ivfpq_range_residual_segments(int nq, int max_nprobe);
int tpq_ivfpq_range_residual_count(const uint8_t* codes, const float* part1, const float* query,
                                   const float* codebook, int ds, const float* part2, const float* full_lut,
                                   const int64_t* cells, const float* base_sims, const uint8_t* is_empty,
                                   const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                   const float* threshold, int32_t* wave_counts, int64_t n_slots, int nq,
                                   int max_nprobe, int m, tpq_stream_t stream);
int tpq_ivfpq_range_residual_fill(const uint8_t* codes, const float* part1, const float* query, const float* codebook,
                                  int ds, const float* part2, const float* full_lut, const int64_t* cells,
                                  const float* base_sims, const uint8_t* is_empty, const int64_t* cell_start,
                                  const int64_t* cell_size, const int64_t* n_probe_list, const float* threshold,
                                  const int64_t* wave_offsets, float* out_vals, int64_t* out_addr, int64_t n_slots,
                                  int nq, int max_nprobe, int m, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFPQIndex filtered search: the k best stored codes of the probed cells AMONG the slots a filter allows (no
 * reference counterpart).  codes, the tables, is_empty, cell_start, cell_size, n_probe_list, n_slots, nq, max_nprobe
 * and m are those of tpq_ivfpq_range_count / tpq_ivfpq_range_residual_count; the scan reads the reference layout,
 * codes u8 [m/4][n_slots][4], whatever the index keeps for its unfiltered search.
 *
 * Filter     filter_bits u32 [n_filters][filter_stride]: bit (s & 31) of word (s >> 5) of row f says that slot
 *            address s is allowed by filter f; filter_stride >= ceil(n_slots / 32); the bits of slots >= n_slots are
 *            padding and are never looked at.  filter_of_query i32 [nq] names the row of every query, NULL: every
 *            query uses row 0.  A value outside [0, n_filters) gives that query no candidate; neither array is then
 *            read out of range.
 * Candidates of a query: those of tpq_ivfpq_range_count -- its first n_probe_list[q] probes (clamped to
 *            [0, max_nprobe]), a probe whose start equals the previous probe's start skipped, the slots inside
 *            [start, start + size) and inside [0, n_slots) (a cell that leaves the storage is cut) that are not
 *            tombstoned (is_empty) -- AND whose bit is set in the query's row.
 * Value      that of tpq_ivfpq_range_count (plain PQ: v = 0.f, then v += lut[j][q][code_j] for j ascending, the
 *            table given as `lut` or built from query, codebook, ds and metric) and of tpq_ivfpq_range_residual_count
 *            (residual PQ: v = base_sims[q][p], then v += LUT_p[j][code_j], stored as v + 0.0f), bit for bit: a
 *            filtered result, a range hit and an unfiltered top-k result of one slot carry the same bits.  A NaN value
 *            never enters.
 * Output     per query the k best candidates by (value descending, address ascending) -- a strict total order: the
 *            result does not depend on the order the slots are met in, nor on n_split; out_vals f32 [nq][k], out_addr
 *            i64 [nq][k], positions beyond the candidates (-inf, -1); out_ids i64 [nq][k] or NULL = address2id[out_addr]
 *            (-1 at the pads), only together with address2id.
 * The scan tests a slot's bit before it reads the slot's code: a 64-slot tile without an allowed live slot reads no
 * code, the allowed slots of several tiles are valued together on full waves.
 *   plain     one workgroup per (query, part), n_split parts, the parts' lists merged as in tpq_ivfpq_scan_topk;
 *             workspace: tpq_ivfpq_scan_filtered_workspace_bytes(nq, k, n_split) bytes (0 when n_split == 1, or for
 *             arguments out of range); too small: TPQ_ERR_WORKSPACE.
 *   residual  one workgroup per query walks its probes, as tpq_ivfpq_scan_topk_residual; no workspace.
 * m % 4 == 0, 1 <= k <= 1024, 1 <= n_split <= 1024, n_filters >= 1 and filter_stride >= ceil(n_slots / 32), else
 * TPQ_ERR_INVALID_ARGUMENT; n_slots < 2^31 - 1 and m <= 148 -- the workgroup's LDS holds m KiB of table, 4 KiB of
 * candidate queues, 4 KiB of pending slots, the probe table and the staged query when the table is built there, in
 * 160 KiB -- else TPQ_ERR_UNSUPPORTED.  nq == 0 is TPQ_OK without a launch.  Every check comes before the first HIP
 * call.  Deterministic, no global atomics.  The library allocates nothing.
 *
 * tpq_slot_filter_build ORs the bit of every address[i], i < n, that lies in [0, n_slots) into `bits` u32
 * [>= ceil(n_slots / 32)], one filter row THE CALLER HAS ZEROED (or that holds an earlier set: the result is the
 * union); other addresses -- the -1 tpq_get_address_by_id gives for an unknown id -- are ignored.  Global atomic OR:
 * the result does not depend on the order.  n == 0 is TPQ_OK.
 * ------------------------------------------------------------------------- */
/* The workspace need not be zeroed: every workgroup writes its whole list (pads included) before the merge reads it. */
size_t tpq_ivfpq_scan_filtered_workspace_bytes(int nq, int k, int n_split);
int tpq_ivfpq_scan_filtered_topk(const uint8_t* codes, const float* lut, const float* query, const float* codebook,
                                 int ds, int metric, const uint8_t* is_empty, const int64_t* cell_start,
                                 const int64_t* cell_size, const int64_t* n_probe_list, const uint32_t* filter_bits,
                                 const int32_t* filter_of_query, int n_filters, int64_t filter_stride,
                                 float* out_vals, int64_t* out_addr, const int64_t* address2id, int64_t* out_ids,
                                 int64_t n_slots, int nq, int max_nprobe, int m, int k, int n_split, void* workspace,
                                 size_t workspace_bytes, tpq_stream_t stream);
int tpq_ivfpq_scan_filtered_residual_topk(const uint8_t* codes, const float* part1, const float* query,
                                          const float* codebook, int ds, const float* part2, const float* full_lut,
                                          const int64_t* cells, const float* base_sims, const uint8_t* is_empty,
                                          const int64_t* cell_start, const int64_t* cell_size,
                                          const int64_t* n_probe_list, const uint32_t* filter_bits,
                                          const int32_t* filter_of_query, int n_filters, int64_t filter_stride,
                                          float* out_vals, int64_t* out_addr, const int64_t* address2id,
                                          int64_t* out_ids, int64_t n_slots, int nq, int max_nprobe, int m, int k,
                                          tpq_stream_t stream);
int tpq_slot_filter_build(const int64_t* address, int64_t n, uint32_t* bits, int64_t n_slots, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFPQ4Index filtered search: the k best stored 4-bit codes of the probed cells AMONG the slots a filter allows,
 * plain codes (tpq_ivfpq4_scan_filtered_topk) and residual codes (tpq_ivfpq4_scan_filtered_residual_topk).  No
 * reference counterpart.
 *
 * codes, query, codebook, (centroids, cells, n_cells,) is_empty, cell_start, cell_size, n_probe_list, out_vals,
 * out_addr, n_slots, m, ds, nq, max_nprobe, k, metric, n_split, workspace: as tpq_ivfpq4_scan_topk /
 * tpq_ivfpq4_scan_residual_topk.
 * Filter     the format of tpq_ivfpq_scan_filtered_topk: filter_bits u32 [n_filters][filter_stride], bit (s & 31) of
 *            word (s >> 5) of row f says that slot address s is allowed by filter f; filter_stride >= ceil(n_slots /
 *            32); the bits of slots >= n_slots are padding and are never looked at.  filter_of_query i32 [nq] names
 *            the row of every query, NULL: every query uses row 0.  A row outside [0, n_filters) gives that query k
 *            pads; neither the filter nor the codes are read for it.
 * Result     candidates, values, order and padding are exactly those of tpq_ivfpq4_scan_topk / _residual_topk called
 *            with is_empty | ~allowed_row(q) as the tombstone mask of query q, bit for bit: value descending, address
 *            ascending; a NaN value never enters; (-inf, -1) beyond the candidates; n_probe_list clamped to
 *            [0, max_nprobe]; a cell that leaves the storage is cut; a probe whose start equals the previous probe's
 *            start is scanned once; for residual codes a slot of two overlapping cells is valued under each probe that
 *            scans it.  The result does not depend on n_split.
 * The scan tests a slot's bit before it reads the slot's code (and the tombstone byte only where the bit is set): a
 * 64-slot tile without an allowed live slot reads no code word; the allowed slots of several tiles -- for residual
 * codes of several probes, each looked up in the table of its own probe -- are valued together on full waves.
 * Unsupported shapes and bad arguments are those of tpq_ivfpq4_scan_topk (m % 8 == 0 in [8, 256], ds >= 1, k in
 * [1, 1024], n_slots < 2^31 - 1: else TPQ_ERR_UNSUPPORTED; metric, n_split in [1, 1024], n_cells >= 1, null pointers:
 * TPQ_ERR_INVALID_ARGUMENT), plus n_filters >= 1, filter_stride >= ceil(n_slots / 32) and a non-null filter_bits, else
 * TPQ_ERR_INVALID_ARGUMENT.  The LDS holds, next to what the unfiltered scan keeps there, the waves' pending lists (4 KiB;
 * 8 KiB for residual codes, whose entries carry a table index): an (m, ds, max_nprobe) that pushes it over 160 KiB
 * returns TPQ_ERR_UNSUPPORTED with a message.  nq == 0 is TPQ_OK without a launch.  Every check comes before the first
 * HIP call.  Workspace: tpq_ivfpq4_scan_workspace_bytes(nq, k, n_split) bytes; too small: TPQ_ERR_WORKSPACE.
 * Deterministic, no global atomics.  The library allocates nothing.
 * ------------------------------------------------------------------------- */
/* TPQ_VERSION is unchanged by these two symbols; a caller that must build against older headers tests this macro. */
#define TPQ_HAS_IVFPQ4_SCAN_FILTERED 1
int tpq_ivfpq4_scan_filtered_topk(const uint8_t* codes, const float* query, const float* codebook,
                                  const uint8_t* is_empty, const int64_t* cell_start, const int64_t* cell_size,
                                  const int64_t* n_probe_list, const uint32_t* filter_bits,
                                  const int32_t* filter_of_query, int n_filters, int64_t filter_stride,
                                  float* out_vals, int64_t* out_addr, int64_t n_slots, int m, int ds, int nq,
                                  int max_nprobe, int k, int metric, int n_split, void* workspace,
                                  size_t workspace_bytes, tpq_stream_t stream);
int tpq_ivfpq4_scan_filtered_residual_topk(const uint8_t* codes, const float* query, const float* codebook,
                                           const float* centroids, const int64_t* cells, int n_cells,
                                           const uint8_t* is_empty, const int64_t* cell_start,
                                           const int64_t* cell_size, const int64_t* n_probe_list,
                                           const uint32_t* filter_bits, const int32_t* filter_of_query, int n_filters,
                                           int64_t filter_stride, float* out_vals, int64_t* out_addr, int64_t n_slots,
                                           int m, int ds, int nq, int max_nprobe, int k, int metric, int n_split,
                                           void* workspace, size_t workspace_bytes, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * IVFPQ4Index range search: every stored 4-bit code of the probed cells whose value reaches a threshold, optionally
 * among the slots a filter allows; plain codes (tpq_ivfpq4_range_count / _fill) and residual codes
 * (tpq_ivfpq4_range_residual_count / _fill).  No reference counterpart.
 *
 * codes, query, codebook, (centroids, cells, n_cells,) is_empty, cell_start, cell_size, n_probe_list, n_slots, m, ds,
 * nq, max_nprobe, metric, n_split: as tpq_ivfpq4_scan_topk / tpq_ivfpq4_scan_residual_topk.
 *
 * Candidates of a query: exactly those of tpq_ivfpq4_scan_topk / _residual_topk -- its first n_probe_list[q] probes
 *            (clamped to [0, max_nprobe]), a probe whose start equals the previous probe's start skipped, the slots
 *            inside [start, start + size) and inside [0, n_slots) (a cell that leaves the storage is cut) that are not
 *            tombstoned (is_empty); for residual codes a slot of two overlapping cells is a candidate once per probe
 *            that scans it.
 * Value      that of tpq_ivfpq4_scan_topk / _residual_topk: the table entries defined there (the workgroup builds
 *            them, for residual codes from the probed cell's centroid; a cell index outside [0, n_cells) is clamped
 *            into the range), then v = 0.f; for j = 0 ... m - 1 ascending: v = v + table[j][code_j], one fp32 add per
 *            step.  Nothing is added to it: a range hit and a top-k result of one slot under one probe carry the same
 *            bits.
 * Hit        a candidate with value >= threshold[q] (threshold f32 [nq]).  A NaN value is never a hit, a NaN
 *            threshold gives no hits, -inf gives every candidate whose value is not NaN.
 * Filter     optional, the format of tpq_ivfpq4_scan_filtered_topk: filter_bits u32 [n_filters][filter_stride], bit
 *            (s & 31) of word (s >> 5) of row f says that slot address s is allowed by filter f; filter_of_query i32
 *            [nq] names the row of every query, NULL: every query uses row 0.  filter_bits == NULL: no filter, the
 *            other three filter arguments are ignored.  With a filter a candidate must also have its bit set in the
 *            query's row; a row outside [0, n_filters) gives that query no hit, and neither the filter nor the codes
 *            are read for it.  The scan tests a slot's bit before its tombstone byte and before any code word: a
 *            64-slot tile without an allowed live slot reads no code; other tiles are valued in place.
 * Order      scan order: probe rank ascending, then address ascending.  Neither the order nor the bits depend on how
 *            the work is cut (n_split).
 * Output     lims i64 [nq + 1], lims[0] = 0: the hits of query q are out_vals[lims[q] : lims[q+1]] (f32) and
 *            out_addr[lims[q] : lims[q+1]] (i64).
 * A query with a NaN or +-Inf component returns what this definition gives and touches no other query's segment.
 *
 * Two passes, no global atomics, no sort, deterministic -- the protocol of tpq_ivfpq_range_count / _fill.
 *   plain     a query's tiles are cut into n_split parts as in the top-k scan, a part's tiles into eight contiguous
 *             chunks, one per wave: segment (q * n_split + part) * 8 + wave; tpq_ivfpq4_range_segments(nq, n_split)
 *             = nq * n_split * 8 segments (0 for nq <= 0 or n_split outside [1, 1024]).
 *   residual  the table depends on the probed cell: one workgroup per (query, probe rank), the cell's tiles in eight
 *             contiguous chunks: segment (q * max_nprobe + p) * 8 + wave; tpq_ivfpq4_range_residual_segments(nq,
 *             max_nprobe) = nq * max_nprobe * 8 segments (0 for nq <= 0 or max_nprobe < 1).  A probe that is not
 *             scanned has eight zero counts.
 *   1. the count pass writes the hits of every segment: wave_counts i32 [segments].
 *   2. THE CALLER turns the counts into exclusive prefix sums: wave_offsets i64 [segments + 1], wave_offsets[0] = 0,
 *      the last entry the total number of hits, which sizes out_vals / out_addr; lims[q] = wave_offsets[q * (segments
 *      / nq)].  The library does not do this step and allocates nothing.
 *   3. the fill pass, with the inputs of the count pass, computes the values again (the same code, the same bits)
 *      and stores segment s at wave_offsets[s] onwards.  A wave stores nothing at or beyond wave_offsets[s + 1],
 *      whatever it finds: inputs that changed between the passes lose hits, they do not become a store outside the
 *      segment.  A segment without hits is not scanned again, a workgroup without hits stages nothing.
 * m % 8 == 0 in [8, 256], ds >= 1, n_slots < 2^31 - 1, else TPQ_ERR_UNSUPPORTED; an invalid metric, n_split outside
 * [1, 1024], n_cells < 1 or a null pointer: TPQ_ERR_INVALID_ARGUMENT; with a non-null filter_bits, n_filters >= 1 and
 * filter_stride >= ceil(n_slots / 32), else TPQ_ERR_INVALID_ARGUMENT.  The workgroup's LDS holds the table (m x 64
 * bytes), the staged query (m * ds * 4 bytes) and, for plain codes, the probe table: a shape over 160 KiB returns
 * TPQ_ERR_UNSUPPORTED with a message.  nq == 0 is TPQ_OK without a launch.  Every check comes before the first HIP call.
 * ------------------------------------------------------------------------- */
/* TPQ_VERSION is unchanged by these six symbols; a caller that must build against older headers tests this macro. */
#define TPQ_HAS_IVFPQ4_RANGE 1
size_t tpq_ivfpq4_range_segments(int nq, int n_split);
int tpq_ivfpq4_range_count(const uint8_t* codes, const float* query, const float* codebook, const uint8_t* is_empty,
                           const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                           const uint32_t* filter_bits, const int32_t* filter_of_query, int n_filters,
                           int64_t filter_stride, const float* threshold, int32_t* wave_counts, int64_t n_slots, int m,
                           int ds, int nq, int max_nprobe, int metric, int n_split, tpq_stream_t stream);
int tpq_ivfpq4_range_fill(const uint8_t* codes, const float* query, const float* codebook, const uint8_t* is_empty,
                          const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                          const uint32_t* filter_bits, const int32_t* filter_of_query, int n_filters,
                          int64_t filter_stride, const float* threshold, const int64_t* wave_offsets, float* out_vals,
                          int64_t* out_addr, int64_t n_slots, int m, int ds, int nq, int max_nprobe, int metric,
                          int n_split, tpq_stream_t stream);
size_t tpq_ivfpq4_range_residual_segments(int nq, int max_nprobe);
int tpq_ivfpq4_range_residual_count(const uint8_t* codes, const float* query, const float* codebook,
                                    const float* centroids, const int64_t* cells, int n_cells, const uint8_t* is_empty,
                                    const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                    const uint32_t* filter_bits, const int32_t* filter_of_query, int n_filters,
                                    int64_t filter_stride, const float* threshold, int32_t* wave_counts,
                                    int64_t n_slots, int m, int ds, int nq, int max_nprobe, int metric,
                                    tpq_stream_t stream);
int tpq_ivfpq4_range_residual_fill(const uint8_t* codes, const float* query, const float* codebook,
                                   const float* centroids, const int64_t* cells, int n_cells, const uint8_t* is_empty,
                                   const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                                   const uint32_t* filter_bits, const int32_t* filter_of_query, int n_filters,
                                   int64_t filter_stride, const float* threshold, const int64_t* wave_offsets,
                                   float* out_vals, int64_t* out_addr, int64_t n_slots, int m, int ds, int nq,
                                   int max_nprobe, int metric, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * FlatIndex fused exact search: the k best stored vectors of every query without a [nq][n_slots] similarity
 * matrix -- a similarity GEMM on the fp32 matrix cores with a top-k epilogue (the semantics of the reference's
 * TopkBMMCuda, torchpq/kernels/TopkBMMCuda.py, which FlatIndex itself does not use).
 *
 * vectors      f32 [d][n_slots]     FlatIndex._storage [d, capacity, 1] as it is; also IVFFlatIndex's vectors
 * query        f32 [d][nq]          (pre-normalised by the host for "cosine")
 * address2id   i64 [n_slots] or NULL   a slot is live iff its entry is >= 0; NULL: every slot is live
 * out_vals     f32 [nq][k]          descending
 * out_addr     i64 [nq][k]
 * out_ids      i64 [nq][k] or NULL  address2id[out_addr] (-1 at the pads); only together with address2id
 *
 * Value of (query q, slot s): dot = sum_i x_q[i] y_s[i], |x_q|^2 and |y_s|^2 are ascending-dimension fp32 fmaf chains
 * from 0.f (what v_mfma_f32_32x32x2_f32 computes; the arithmetic of tpq_ivfpq_coarse_probe's similarities):
 *       TPQ_METRIC_NEG_SQ_L2:  v = 2.f*dot;  v = v - |x|^2;  v = v - |y|^2
 *       TPQ_METRIC_INNER:      v = dot
 * Output per query: the k best live slots by (value descending, address ascending) -- a strict total order, so the
 * result does not depend on the order the slots are met in; a slot whose value is NaN never enters; a live slot
 * whose value is -inf keeps its address and stands ahead of the pads; positions beyond the candidates are
 * (-inf, -1, -1).  A query with a NaN or +-Inf component still returns: its own row is not pinned, every other row
 * is what it is without it.
 * 1 <= k <= 1024, any d >= 1, 1 <= n_parts <= 1024, else TPQ_ERR_INVALID_ARGUMENT; n_slots < 2^31 - 1, else
 * TPQ_ERR_UNSUPPORTED.  nq == 0 or n_slots == 0 is TPQ_OK (no slots: all pads).
 * n_parts: the contiguous slot ranges (of whole 256-slot chunks) a query's walk over the database is cut into, one
 * workgroup per (128 queries, range), so that a small batch still fills the chip; the caller picks it from nq,
 * n_slots and the CU count.  The result is the same bits for every n_parts, empty ranges included.
 * workspace: tpq_flat_topk_workspace_bytes(nq, k, n_parts) bytes -- one sorted list of 64 R keys of 8 bytes per
 * (query, range), R = 1, 2, 4, 8, 16 covering k; a function of (nq, k, n_parts) only: nothing of size nq x n_slots
 * exists anywhere (0 for nq <= 0 or arguments out of range); too small: TPQ_ERR_WORKSPACE.  Two launches (tiles,
 * then a merge that also gathers the ids), no global atomics, deterministic.  The library allocates nothing.
 * ------------------------------------------------------------------------- */
/* The workspace need not be zeroed: a list that took no candidate is written as pads before the merge reads it. */
size_t tpq_flat_topk_workspace_bytes(int nq, int k, int n_parts);
int tpq_flat_topk(const float* vectors, const float* query, const int64_t* address2id,
                  float* out_vals, int64_t* out_addr, int64_t* out_ids,
                  int64_t n_slots, int d, int nq, int k, int metric, int n_parts,
                  void* workspace, size_t workspace_bytes, tpq_stream_t stream);

/* ---------------------------------------------------------------------------
 * FlatIndex range search: every live stored vector whose value reaches a threshold, over the whole database (no
 * reference counterpart) -- the similarity tiles of tpq_flat_topk with a count and a fill epilogue.  vectors, query,
 * address2id, n_slots, d, nq, metric and n_parts are those of tpq_flat_topk.
 *
 * Value      of (query q, slot s): exactly the value tpq_flat_topk defines (the same code, the same bits), -0.0
 *            returned as +0.0.
 * Hit        a slot below n_slots that is live (address2id NULL, or address2id[s] >= 0) with value >= threshold[q]
 *            (threshold f32 [nq]).  A NaN value is never a hit, a NaN threshold gives no hits, -inf gives every live
 *            slot whose value is not NaN -- a live slot whose value is -inf included.
 * Order      address ascending, for every n_parts.
 * Output     lims i64 [nq + 1], lims[0] = 0: the hits of query q are out_vals[lims[q] : lims[q+1]] (f32),
 *            out_addr[lims[q] : lims[q+1]] (i64) and, where out_ids is given (only together with address2id),
 *            out_ids[lims[q] : lims[q+1]] = address2id[out_addr] (i64).
 * A query with a NaN or +-Inf component returns what this definition gives (usually nothing) and touches no
 * other query's segment.
 *
 * Two passes, no global atomics, no sort, deterministic.  A query's walk is cut into n_parts ranges of whole
 * 256-slot chunks as in tpq_flat_topk, one workgroup per (128 queries, range): segment q * n_parts + part.
 *   1. tpq_flat_range_count writes the hits of every segment: counts i32 [tpq_flat_range_segments(nq, n_parts)]
 *      (= nq * n_parts; 0 for nq <= 0 or n_parts outside [1, 1024]), empty ranges and n_slots == 0 included (0).
 *   2. THE CALLER turns the counts into exclusive prefix sums: offsets i64 [segments + 1], offsets[0] = 0, the last
 *      entry the total number of hits, which sizes out_vals / out_addr / out_ids; lims[q] = offsets[q * n_parts].
 *      The library does not do this step and allocates nothing.
 *   3. tpq_flat_range_fill, with the inputs of the count pass, computes the values again and stores segment s at
 *      offsets[s] onwards.  Nothing is stored at or beyond offsets[s + 1], whatever is found: inputs that changed
 *      between the passes lose hits, they do not become a store outside the segment.  A workgroup whose 128
 *      segments are all empty does not walk its range again.
 * Temporary memory is the counts and offsets: nothing of size nq x n_slots exists anywhere.
 * any d >= 1, 1 <= n_parts <= 1024, else TPQ_ERR_INVALID_ARGUMENT; n_slots < 2^31 - 1, else TPQ_ERR_UNSUPPORTED.
 * nq == 0 is TPQ_OK.
 * ------------------------------------------------------------------------- */
size_t tpq_flat_range_segments(int nq, int n_parts);
int tpq_flat_range_count(const float* vectors, const float* query, const int64_t* address2id, const float* threshold,
                         int32_t* counts, int64_t n_slots, int d, int nq, int metric, int n_parts, tpq_stream_t stream);
int tpq_flat_range_fill(const float* vectors, const float* query, const int64_t* address2id, const float* threshold,
                        const int64_t* offsets, float* out_vals, int64_t* out_addr, int64_t* out_ids,
                        int64_t n_slots, int d, int nq, int metric, int n_parts, tpq_stream_t stream);

/* Measurement utility (no reference counterpart): streams `bytes` of `src` through 16-byte
 * loads from `n_blocks` workgroups of 256 threads (0 = 8 per CU) and discards them.  bench.py
 * times it on a buffer larger than the 256 MiB Infinity Cache to obtain the box's sustained HBM
 * read rate, the "measured stream peak" that SURVEY 8d asks roofline fractions to be quoted
 * against next to the 8 TB/s spec figure.  `sink_or_null`: optional u32 the kernel may bump. */
int tpq_ubench_stream_read(const void* src, size_t bytes, void* sink_or_null, int n_blocks,
                           tpq_stream_t stream);
/* Measurement utility: the same streaming read with its knobs exposed -- `threads` per workgroup (a multiple of 64,
 * <= 1024), `unroll` 16-byte loads in flight per lane (4, 8, 16), `chunk_bytes` = the size of a contiguous piece dealt to
 * ONE workgroup (a probed cell of the list scan; 0 = the buffer cut evenly over the workgroups), `nontemporal` loads or
 * plain ones.  bench.py sweeps a few settings, the scan's own pattern among them, and quotes the best as the stream peak:
 * a record labelled "hbm" must not exceed it. */
int tpq_ubench_stream_read_ex(const void* src, size_t bytes, void* sink_or_null, int n_blocks, int threads,
                              int unroll, size_t chunk_bytes, int nontemporal, tpq_stream_t stream);
/* Measurement utility: the k-means update's read pattern without its compute -- data f32
 * [l][d][n] read by one-wave blocks, 32 rows x 256 bytes per 64-point tile, `chunks` blocks per
 * (sub-problem, 32-row group) taking tiles round-robin.  Tells a pattern-bound kernel from a
 * compute-bound one (tools/kmeans_microbench.py --rows-read). */
int tpq_ubench_rows_read(const float* src, int l, int d, int64_t n, int chunks, void* sink_or_null,
                         tpq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TORCHPQ_AMD_H_ */
