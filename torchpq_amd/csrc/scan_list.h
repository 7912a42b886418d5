// IVF list scan: the frame of a list kernel -- everything around the value of a slot that the reference-layout scans
// (scan_ref.h), the IVFFlat scan and range search (scan_flat.hip), the 4-bit scan (scan_pq4.hip) and the IVFPQ range
// search (scan_range.hip) share: the probe count, the LDS carve-up, a part's tiles and a wave's chunk of them, the tile
// walk, the admission step, the look-ups of an 8-bit code word (where they compile alike), the metric's arithmetic, the residual table, the
// range segments; on the host the launch, the checks and the argument filling of the list entry points.
// Takes scan_shared.h and scan_args.h only (scan_range.hip includes nothing else); scan_packed_kernel.h takes
// clamped_n_probe from here.
#pragma once
#include "scan_shared.h"

namespace tpq {

__host__ __device__ constexpr size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
// a probe table of max_nprobe cells: start, size, and the exclusive prefix of the tiles (one more entry)
__host__ __device__ constexpr size_t probe_table_bytes(int max_nprobe) { return (size_t)(3 * max_nprobe + 1) * 4; }

// the query's probe count, clamped to [0, max_nprobe] -- and to the call's probe cap, when it has one
__device__ __forceinline__ int clamped_n_probe(const ScanArgs& a, int q) {
  const int n_probe = (int)a.n_probe_list[q];
  const int n = n_probe < 0 ? 0 : (n_probe > a.max_nprobe ? a.max_nprobe : n_probe);
  return (a.probe_cap > 0 && n > a.probe_cap) ? a.probe_cap : n;
}

// ---- LDS of a top-k list kernel: [region0][queues 8 x 512][probe table 3 n + 1][tau][tail] ------------------------
// region0 holds the kernel's payload (a table, the query) and, once the scan is over, the finisher's merge lists
template <class T>
__host__ __device__ constexpr T list_region0(T payload_bytes, int R) {
  const T lists = (T)(kScanWaves * R * 64 * 8);
  return payload_bytes > lists ? payload_bytes : lists;
}
static size_t list_scan_lds_bytes(size_t region0, int max_nprobe, size_t tail_bytes) {
  return align16(region0 + kScanWaves * 512 + probe_table_bytes(max_nprobe) + 4 + tail_bytes);
}
// lists of the parts of split queries (none when a query is one workgroup): [values nq * n_split * 64 R][indices ...]
static size_t list_ws_bytes(int nq, int R, int n_split) {
  return n_split > 1 ? (size_t)nq * n_split * R * 64 * 8 : 0;
}

__device__ __forceinline__ ProbeTable probe_table_at(void* at, int max_nprobe) {
  int* ptab = reinterpret_cast<int*>(at);
  return ProbeTable{ptab, ptab + max_nprobe, ptab + 2 * max_nprobe};
}

struct ListLds {
  float* qv;          // the waves' candidate queues: values [8][64] ...
  int* qi;            // ... and slots [8][64]
  ProbeTable tab;
  unsigned* tau_key;  // the workgroup-shared admission threshold, as a key
  char* tail;         // whatever the kernel keeps behind the frame (a staged query)
  __device__ __forceinline__ ListLds(char* smem, size_t region0, int max_nprobe)
      : qv(reinterpret_cast<float*>(smem + region0)),
        qi(reinterpret_cast<int*>(smem + region0 + kScanWaves * 256)),
        tab(probe_table_at(smem + region0 + kScanWaves * 512, max_nprobe)),
        tau_key(reinterpret_cast<unsigned*>(tab.start + 3 * max_nprobe + 1)),
        tail(reinterpret_cast<char*>(tau_key + 1)) {}
  // wave 0 fills the probe table and opens the threshold (the caller's next barrier publishes both)
  __device__ __forceinline__ void init(const ScanArgs& a, int q, int n_probe, int wave, int lane) const {
    if (wave == 0) {
      build_probe_table(a, q, n_probe, tab);
      if (lane == 0) *tau_key = f2key(-INFINITY);
    }
  }
};

// the finisher of a top-k list kernel: its merge lists lie over region0
template <int R>
__device__ __forceinline__ void finish_list_scan(const ScanArgs& a, int q, int part, WaveTopK<R>& top, char* smem) {
  finish_query<R>(a, q, part, top, reinterpret_cast<float*>(smem),
                  reinterpret_cast<int*>(smem + kScanWaves * R * 64 * 4));
}

// ---- tiles ---------------------------------------------------------------------------------------------------------
struct TileRange {
  int begin, end;
};
// part `part` of n_split of a query's `total` tiles
__device__ __forceinline__ TileRange part_tiles(int total, int part, int n_split) {
  return TileRange{(int)(((int64_t)total * part) / n_split), (int)(((int64_t)total * (part + 1)) / n_split)};
}
// the wave's contiguous chunk of [t_begin, t_end) (the range kernels: segments in wave order are tile-ascending)
__device__ __forceinline__ TileRange wave_chunk(int t_begin, int t_end, int wave) {
  const int n_tiles = t_end - t_begin;
  return TileRange{t_begin + (int)(((int64_t)n_tiles * wave) / kScanWaves),
                   t_begin + (int)(((int64_t)n_tiles * (wave + 1)) / kScanWaves)};
}

// The lane's place in tile T of a probe table: its offset into the probed cell, and the cell's extent.  A slot is
// scanned when it is in_cell(); the kernels that also cut a cell at the storage test slot() against n_slots themselves.
struct Tile {
  int off, start, size;
  __device__ __forceinline__ bool in_cell() const { return off < size; }
  __device__ __forceinline__ int slot() const { return start + off; }
};
// The tile walk, tiles visited in ascending order: p = probe_of(tab, p, T), from p = 0 before the first tile, then
// tile_at(tab, p, T, lane).  (One function that advances a reference compiles to another loop, with one more LDS read.)
__device__ __forceinline__ int probe_of(const ProbeTable& tab, int p, int T) {
  while (T >= tab.tile_begin[p + 1]) ++p;
  return p;
}
__device__ __forceinline__ Tile tile_at(const ProbeTable& tab, int p, int T, int lane) {
  const int off = ((T - tab.tile_begin[p]) << 6) + lane;
  return Tile{off, tab.start[p], tab.size[p]};
}

// ---- admission -----------------------------------------------------------------------------------------------------
// workgroup-shared admission threshold: any wave's k-th best bounds the final k-th best.  Polls it, admits slot s when
// `live` and v >= tau -- a NaN value fails the test and never enters -- with the value `pushed`, and publishes the
// wave's threshold when the push raised it.
template <int R>
__device__ __forceinline__ void admit(WaveSelector<R>& sel, unsigned* tau_key, bool live, float v, int s, float pushed) {
  const float tau_s = key2f(lds_poll_u32(tau_key));
  sel.tau = fmaxf(sel.tau, tau_s);
  const float tau_before = sel.tau;
  sel.push(live && (v >= sel.tau), pushed, s);
  if (sel.tau > tau_before && lane_id() == 0) atomicMax(tau_key, f2key(sel.tau));
}
template <int R>
__device__ __forceinline__ void admit(WaveSelector<R>& sel, unsigned* tau_key, bool live, float v, int s) {
  admit(sel, tau_key, live, v, s, v);
}

// ---- pending slots -------------------------------------------------------------------------------------------------
// The kernels that test a slot before they read it (scan_filtered.hip, the masked scan of scan_flat.hip) compact the
// slots that pass into a list the wave owns in LDS -- kPendingBytes behind the frame, at ListLds::tail -- and value 64
// of them at a time, one per lane.
constexpr int kPendingPerWave = 128;  // at most 63 left over + the 64 of one tile
constexpr size_t kPendingBytes = (size_t)kScanWaves * kPendingPerWave * 4;

// the wave's pending slots, in LDS words of its own
struct Pending {
  int* at;
  int n;  // wave-uniform, < 64 between tiles
  __device__ __forceinline__ void append(bool ok, int s) {
    const unsigned long long mask = __ballot(ok);
    if (mask == 0ull) return;
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
    if (ok) at[n + rank] = s;
    n += __popcll(mask);
  }
  // the last `count` (<= 64) pending slots, one per lane below `count`
  __device__ __forceinline__ int take(int count) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    n -= count;
    const int lane = lane_id();
    const int s = lane < count ? at[n + lane] : 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    return s;
  }
};

// ---- filter rows ---------------------------------------------------------------------------------------------------
// The bit rows of the filtered scans (scan_filtered.hip, scan_pq4_filtered.hip): bit s & 31 of word s >> 5 for slot s.
namespace filtered {

struct FilterArgs {
  const uint32_t* bits;     // [n_filters][stride]
  const int32_t* of_query;  // [nq] or nullptr: row 0
  int64_t stride;
  int n_filters;
};

// the query's row, or nullptr when it names none: the query then has no candidate and neither array is read further
__device__ __forceinline__ const uint32_t* filter_row(const FilterArgs& f, int q) {
  const int r = f.of_query ? f.of_query[q] : 0;
  return (r >= 0 && r < f.n_filters) ? f.bits + (int64_t)r * f.stride : nullptr;
}

// a lane's slot of a tile: inside the cell, inside the storage, and allowed (the only read is the filter word)
struct Member {
  int s;
  bool ok;
};
__device__ __forceinline__ Member member(const uint32_t* __restrict__ row, int start, int size, int off,
                                         int64_t n_slots) {
  const int64_t s64 = (int64_t)start + off;
  bool ok = off < size && s64 >= 0 && s64 < n_slots;
  if (ok) ok = ((row[s64 >> 5] >> (unsigned)(s64 & 31)) & 1u) != 0;
  return Member{(int)s64, ok};
}

}  // namespace filtered

// ---- values --------------------------------------------------------------------------------------------------------
// one dimension of a value: -(q - x)^2 or q x added to acc, each operation rounded on its own
template <int METRIC>
__device__ __forceinline__ float metric_step(float acc, float q, float x) {
  if constexpr (METRIC == TPQ_METRIC_NEG_SQ_L2) {
    const float t = __fsub_rn(q, x);
    return __fsub_rn(acc, __fmul_rn(t, t));
  } else {
    return __fadd_rn(acc, __fmul_rn(q, x));
  }
}

// The four sub-quantizers of one 8-bit code word, looked up in their rows at `row` and added in ascending order: the
// ungrouped loops of scan_residual_kernel and residual_slot_term_kernel.  The two grouped sums -- scan_ref_kernel's,
// indexed from the storage's base, and pqrange::slot_value's (scan_range.hip), walking a column pointer -- keep the four
// lines written out: through this function, or through one shared grouped function, they compile to other code.
__device__ __forceinline__ float lut_word(float v, const float* row, uint32_t w) {
  v += row[w & 255u];
  v += row[256 + ((w >> 8) & 255u)];
  v += row[512 + ((w >> 16) & 255u)];
  v += row[768 + (w >> 24)];
  return v;
}

// Residual PQ, the table of probe p of query q: LUT_p = part1[q] + part2[cell] (one fp32 add per entry,
// load_precomputed_v3, ivfpq_topk.cu:522-560; part1 read, or built from the query staged at xq) or LUT_p = full[q][p].
// Every thread of the workgroup takes its share; the caller holds the barriers on either side.
__device__ __forceinline__ void build_residual_lut(const ScanArgs& a, const ResidualArgs& ra, int q, int p, float* lut,
                                                   const float* xq, bool build_part1) {
  const int n4 = a.m * 64;  // float4 count of one table
  float4* dst = reinterpret_cast<float4*>(lut);
  if (ra.full) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(ra.full) + ((int64_t)q * a.max_nprobe + p) * n4;
    for (int i = threadIdx.x; i < n4; i += kScanThreads) dst[i] = src[i];
  } else {
    const float4* __restrict__ s1 = reinterpret_cast<const float4*>(ra.part1) + (int64_t)q * n4;
    const float4* __restrict__ s2 =
        reinterpret_cast<const float4*>(ra.part2) + ra.cells[(int64_t)q * a.max_nprobe + p] * (int64_t)n4;
    for (int i = threadIdx.x; i < n4; i += kScanThreads) {
      const float4 x = build_part1 ? fused_lut4(a, i >> 6, i & 63, xq) : s1[i];
      const float4 y = s2[i];
      dst[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
    }
  }
}

// ---- range search: two passes over the same tiles, one segment of the output per wave ---------------------------
struct RangeArgs {
  const float* threshold;       // [nq]
  int* wave_counts;             // count pass: [segments], eight per workgroup
  const int64_t* wave_offsets;  // fill pass: [segments + 1] exclusive prefix sums of the counts
};

// A wave's segment.  Count pass: the number of hits.  Fill pass: hits are appended from `pos` on, in lane order, and
// nothing is stored at or beyond `end` -- what the count pass saw is all this wave may write: with other inputs than
// the count pass had (or offsets that are not its prefix sums) hits are dropped, never stored in the next segment.
template <bool FILL>
struct Segment {
  int64_t pos = 0, end = 0;
  int n = 0;
  // fill pass: the workgroup whose segments start at `seg` has no hit -- it leaves before it stages anything (the same
  // two words for every thread: uniform)
  static __device__ __forceinline__ bool no_hit(const RangeArgs& r, int64_t seg) {
    if constexpr (FILL) return r.wave_offsets[seg + kScanWaves] <= r.wave_offsets[seg];
    return false;
  }
  // wave `wave` of that workgroup
  __device__ __forceinline__ Segment(const RangeArgs& r, int64_t seg, int wave) {
    if constexpr (FILL) {
      pos = r.wave_offsets[seg + wave];
      end = r.wave_offsets[seg + wave + 1];
    }
  }
  // fill pass, once the workgroup's barriers are behind the wave: nothing to write, so nothing is read
  __device__ __forceinline__ bool empty() const {
    if constexpr (FILL) return pos < 0 || end <= pos;
    return false;
  }
  __device__ __forceinline__ void emit(const ScanArgs& a, bool hit, float v, int s) {
    const unsigned long long mask = __ballot(hit);
    if constexpr (FILL) {
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
      const int64_t o = pos + rank;
      if (hit && o < end) {
        a.out_vals[o] = v;
        a.out_addr[o] = (int64_t)s;
      }
      pos += __popcll(mask);
    } else {
      n += __popcll(mask);
    }
  }
  __device__ __forceinline__ void close(const RangeArgs& r, int64_t seg, int wave) const {
    if constexpr (!FILL) {
      if (lane_id() == 0) r.wave_counts[seg + wave] = n;
    }
  }
};

// ---- host ----------------------------------------------------------------------------------------------------------
static int check_lds(const char* what, size_t lds) {
  if (lds > 160 * 1024) {
    set_error("%s: needs %zu bytes of LDS (> 160 KiB per CU on gfx950)", what, lds);
    return TPQ_ERR_UNSUPPORTED;
  }
  return TPQ_OK;
}

static int need_ws(const void* ws, size_t have, size_t need, const char* who) {
  if (need && (!ws || have < need)) {
    set_error("%s: workspace too small (%zu < %zu)", who, have, need);
    return TPQ_ERR_WORKSPACE;
  }
  return TPQ_OK;
}

// the list workspace of a top-k entry point: checked, then handed to the kernels
static int take_list_ws(ScanArgs& a, int R, void* workspace, size_t workspace_bytes, const char* what) {
  const size_t need = list_ws_bytes(a.nq, R, a.n_split);
  if (int rc = need_ws(workspace, workspace_bytes, need, what)) return rc;
  if (need) {
    a.ws_vals = reinterpret_cast<float*>(workspace);
    a.ws_idx = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + need / 2);
  }
  return TPQ_OK;
}

// one workgroup per (query, part) of `kernel(a, args...)`, then the merge of the parts' lists when queries are split
template <class Kernel, class Merge, class... Args>
static int launch_list_scan(Kernel kernel, Merge merge_kernel, const char* name, const ScanArgs& a, size_t lds,
                            hipStream_t st, const Args&... args) {
  if (int rc = check_lds(name, lds)) return rc;
  if (int rc = launch_with_lds(kernel, name, dim3((unsigned)a.nq * a.n_split), dim3(kScanThreads), lds, st, a, args...))
    return rc;
  if (a.n_split > 1) {
    hipLaunchKernelGGL(merge_kernel, dim3(a.nq), dim3(64), 0, st, a);
    TPQ_LAUNCH_CHECK("scan_merge_kernel");
  }
  return TPQ_OK;
}

// The checks the list entry points share, each in the place the entry point makes it (all of them before any HIP call)
static int check_batch(const char* what, int nq, int max_nprobe) {
  TPQ_REQUIRE(nq >= 0 && max_nprobe >= 1, "%s: bad nq/max_nprobe (%d, %d)", what, nq, max_nprobe);
  return TPQ_OK;
}
static int check_n_slots(const char* what, int64_t n_slots) {
  TPQ_REQUIRE(n_slots >= 0, "%s: n_slots=%lld", what, (long long)n_slots);
  if (n_slots >= (int64_t)kPadIdx) {
    set_error("%s: n_slots=%lld >= 2^31-1 is not supported", what, (long long)n_slots);
    return TPQ_ERR_UNSUPPORTED;
  }
  return TPQ_OK;
}
static int check_lists(const char* what, int metric, int n_split, int64_t n_slots) {
  TPQ_REQUIRE(metric == TPQ_METRIC_NEG_SQ_L2 || metric == TPQ_METRIC_INNER, "%s: metric=%d", what, metric);
  TPQ_REQUIRE(n_split >= 1 && n_split <= 1024, "%s: n_split=%d out of range", what, n_split);
  return check_n_slots(what, n_slots);
}
// ... and, for a batch that is not empty: the pointers, the grid
static int check_grid(const char* what, bool pointers, int nq, int n_split) {
  TPQ_REQUIRE(pointers, "%s: null pointer argument", what);
  TPQ_REQUIRE((int64_t)nq * n_split < 0x7fffffffLL, "%s: nq * n_split = %lld workgroups", what,
              (long long)nq * n_split);
  return TPQ_OK;
}

// the arguments every scan entry point shares, set by name (the rest of ScanArgs stays zero)
static ScanArgs scan_args(const uint8_t* codes, const uint8_t* packed, const float* lut, const uint8_t* is_empty,
                          const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list,
                          float* out_vals, int64_t* out_addr, const int64_t* address2id, int64_t* out_ids,
                          int64_t n_slots, int nq, int max_nprobe, int m, int k, int n_split) {
  ScanArgs a{};
  a.codes = codes; a.packed = packed; a.lut = lut; a.is_empty = is_empty;
  a.cell_start = cell_start; a.cell_size = cell_size; a.n_probe_list = n_probe_list;
  a.out_vals = out_vals; a.out_addr = out_addr; a.address2id = address2id; a.out_ids = out_ids;
  a.n_slots = n_slots; a.nq = nq; a.max_nprobe = max_nprobe; a.m = m; a.k = k; a.n_split = n_split;
  return a;
}

}  // namespace tpq
