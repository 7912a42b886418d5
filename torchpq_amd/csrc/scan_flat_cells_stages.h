// The stages of the cell-major IVFFlat routes that never read a stored vector, and the frame of the one that does last:
// workspace, seed (stage 2), inversion (stage 3), finish (stage 5) and the launch sequence, shared by
// scan_flat_cells.hip (fp32 lists, FcArgsT<float>) and scan_flat_f16_cells.hip (fp16 lists, FcArgsT<uint32_t>).  The
// stages are described in the head of scan_flat_cells.hip; a unit brings its candidate kernel (stage 4), the value of a
// candidate (Value::value<METRIC>(a, slot, q): the chain its query-major scan specifies) and what its seed kernel
// prepares per query beyond |q|^2 and tau_q (Prep: fp32 nothing, fp16 the query's scale and its absolute band).
#pragma once
#include <cfloat>

#include "scan_list.h"
#include "sims_chunk.h"

namespace tpq {
namespace fcells {

constexpr int kFcBlock = 128;       // queries of a work item: 4 waves x 32 MFMA columns
constexpr int kFcSlice = 128;       // consecutive queries per inversion workgroup
constexpr int kFcInvThreads = 512;
constexpr int kFcWindow = 16384;    // cells of the inversion's LDS histogram (64 KiB)
constexpr int kFcUnroll = 8;        // row loads in flight per lane of the finish kernel (kFlatUnroll of scan_flat.hip)
constexpr int kFcCtrlInts = 64;     // [0] flagged queries, [1] the candidate kernel's item counter

template <class V>
struct FcArgsT {
  const V* vectors;      // float: [d][n_slots]; uint32_t: [d / 2][n_slots], two halves per word
  const float* query;    // [d][nq]
  const uint8_t* is_empty;
  const int64_t* cells;  // [nq][max_nprobe]
  const int64_t* cell_start;
  const int64_t* cell_size;
  const int64_t* n_probe_list;
  float* out_vals;    // [nq][k]: stage 1's seeds, then the result
  int64_t* out_addr;
  int n_slots, n_cells, d, nq, max_nprobe, k, p0, cand_cap;
  float kb;  // delta = kb (|q|^2 + |x|^2)
  // the workspace
  int* ctrl;      // [kFcCtrlInts]
  int* flags;     // [nq]
  float* tau;     // [nq]
  float* qn;      // [nq] |q|^2
  int* cnt;       // [nq] candidates reserved (beyond cand_cap: counted, not stored)
  int* hist;      // [n_cells] pairs per cell, then the scatter's cursor
  int* cell_off;  // [n_cells + 1] exclusive prefix of the pairs
  int* blk_off;   // [n_cells + 1] exclusive prefix of ceil(pairs / kFcBlock)
  int* cell_st;   // [n_cells] extent of a listed cell
  int* cell_sz;
  int* pairs;     // [nq (max_nprobe - p0)] query numbers, grouped by cell
  int* cand;      // [nq][cand_cap] slot addresses
};

__host__ __device__ constexpr size_t fc_align(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t fc_workspace_bytes(int nq, int max_nprobe, int n_cells, int cand_cap, int p0) {
  const size_t np = max_nprobe > p0 ? (size_t)(max_nprobe - p0) : 0;
  return fc_align(kFcCtrlInts * 4) + 4 * fc_align((size_t)nq * 4) + 3 * fc_align((size_t)n_cells * 4) +
         2 * fc_align(((size_t)n_cells + 1) * 4) + fc_align((size_t)nq * np * 4) + fc_align((size_t)nq * cand_cap * 4);
}

// the regions of fc_workspace_bytes; returns the first byte behind them
template <class V>
static char* fc_carve(FcArgsT<V>& a, void* workspace) {
  char* p = reinterpret_cast<char*>(workspace);
  auto take = [&](size_t bytes) {
    char* r = p;
    p += fc_align(bytes);
    return r;
  };
  const size_t np = a.max_nprobe > a.p0 ? (size_t)(a.max_nprobe - a.p0) : 0;
  a.ctrl = reinterpret_cast<int*>(take(kFcCtrlInts * 4));
  a.flags = reinterpret_cast<int*>(take((size_t)a.nq * 4));
  a.tau = reinterpret_cast<float*>(take((size_t)a.nq * 4));
  a.qn = reinterpret_cast<float*>(take((size_t)a.nq * 4));
  a.cnt = reinterpret_cast<int*>(take((size_t)a.nq * 4));
  a.hist = reinterpret_cast<int*>(take((size_t)a.n_cells * 4));
  a.cell_st = reinterpret_cast<int*>(take((size_t)a.n_cells * 4));
  a.cell_sz = reinterpret_cast<int*>(take((size_t)a.n_cells * 4));
  a.cell_off = reinterpret_cast<int*>(take(((size_t)a.n_cells + 1) * 4));
  a.blk_off = reinterpret_cast<int*>(take(((size_t)a.n_cells + 1) * 4));
  a.pairs = reinterpret_cast<int*>(take((size_t)a.nq * np * 4));
  a.cand = reinterpret_cast<int*>(take((size_t)a.nq * a.cand_cap * 4));
  return p;
}

// the query's probe count, clamped to [0, max_nprobe]
template <class V>
__device__ __forceinline__ int fc_n_probe(const FcArgsT<V>& a, int q) {
  const int64_t n = a.n_probe_list[q];
  return n < 0 ? 0 : (n > a.max_nprobe ? a.max_nprobe : (int)n);
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------
// prep(a, q, tau) runs for every query and returns the threshold the candidate kernel tests against
struct FcNoPrep {
  template <class V>
  __device__ __forceinline__ float operator()(const FcArgsT<V>&, int, float tau) const { return tau; }
};

template <class V, class Prep>
__global__ __launch_bounds__(256) void fc_seed_kernel(FcArgsT<V> a, Prep prep) {
  const int tid = (int)(blockIdx.x * 256 + threadIdx.x);
  for (int i = tid; i < a.n_cells; i += (int)gridDim.x * 256) a.hist[i] = 0;
  if (tid < kFcCtrlInts) a.ctrl[tid] = 0;
  const int q = tid;
  if (q >= a.nq) return;
  const float q2 = sims_query_sq_norm(a.query + q, a.d, a.nq);
  const float tau = a.out_vals[(int64_t)q * a.k + a.k - 1];
  const int n_probe = fc_n_probe(a, q);
  // (a NaN or +-Inf component makes |q|^2 NaN or +inf: one test)
  bool bad = !(q2 <= FLT_MAX) || tau == INFINITY;
  for (int p = a.p0; p < n_probe; ++p) {
    const int64_t c = a.cells[(int64_t)q * a.max_nprobe + p];
    bad = bad || c < 0 || c >= (int64_t)a.n_cells;
  }
  a.tau[q] = prep(a, q, tau);
  a.qn[q] = q2;
  a.cnt[q] = 0;
  a.flags[q] = (bad && n_probe > a.p0) ? 1 : 0;  // (no probe beyond P0: stage 1's row is the result)
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------
// the listed pairs of the slice from q0 whose cell lies in [w0, w0 + kFcWindow), flattened over the workgroup: pair i is
// (q0 + i / np, p0 + i % np), so the rows of cell_start, cell_size and cells are read coalesced.  f(q, st, sz, cell)
template <class V, class F>
__device__ __forceinline__ void fc_slice_pairs(const FcArgsT<V>& a, int q0, int w0, F&& f) {
  const int np = a.max_nprobe - a.p0;  // (> 0: the launch)
  const int nqs = a.nq - q0 < kFcSlice ? a.nq - q0 : kFcSlice;
  for (int i = (int)threadIdx.x; i < nqs * np; i += kFcInvThreads) {
    const int dq = i / np;
    const int q = q0 + dq, p = a.p0 + (i - dq * np);
    if (p >= fc_n_probe(a, q) || a.flags[q] != 0) continue;
    const int64_t o = (int64_t)q * a.max_nprobe + p;
    // the extent as fetch_probes (scan_shared.h) takes it: empty, or the previous probe's start again -> not scanned
    const int st = (int)a.cell_start[o], sz = (int)a.cell_size[o];
    if (sz <= 0 || (p > 0 && a.cell_start[o - 1] == (int64_t)st)) continue;
    const int c = (int)a.cells[o];  // in [0, n_cells): the seed kernel's check
    if (c < w0 || c >= w0 + kFcWindow) continue;
    f(q, st, sz, c);
  }
}

// the slice's pairs per cell of the window, in LDS
template <class V>
__device__ __forceinline__ void fc_count_slice(const FcArgsT<V>& a, int q0, int w0, int wn, int* cell_h) {
  __syncthreads();  // (the previous window's readers)
  for (int c = (int)threadIdx.x; c < wn; c += kFcInvThreads) cell_h[c] = 0;
  __syncthreads();
  fc_slice_pairs(a, q0, w0, [&](int, int, int, int c) { atomicAdd(&cell_h[c - w0], 1); });
  __syncthreads();
}

template <class V>
__global__ __launch_bounds__(kFcInvThreads) void fc_count_kernel(FcArgsT<V> a) {
  extern __shared__ int cell_h[];
  const int q0 = (int)blockIdx.x * kFcSlice;
  for (int w0 = 0; w0 < a.n_cells; w0 += kFcWindow) {
    const int wn = a.n_cells - w0 < kFcWindow ? a.n_cells - w0 : kFcWindow;
    fc_count_slice(a, q0, w0, wn, cell_h);
    for (int c = (int)threadIdx.x; c < wn; c += kFcInvThreads) {
      const int h = cell_h[c];
      if (h) atomicAdd(&a.hist[w0 + c], h);
    }
  }
}

// one block: exclusive prefixes of the histogram (pairs) and of ceil(pairs / kFcBlock) (work items); the histogram
// becomes the scatter's cursor
template <class V>
__global__ __launch_bounds__(1024) void fc_scan_kernel(FcArgsT<V> a) {
  __shared__ int sp[2][1024], sb[2][1024];
  const int tid = (int)threadIdx.x;
  const int per = (a.n_cells + 1023) / 1024;
  const int lo = tid * per < a.n_cells ? tid * per : a.n_cells;
  const int hi = lo + per < a.n_cells ? lo + per : a.n_cells;
  int np = 0, nb = 0;
  for (int c = lo; c < hi; ++c) {
    const int h = a.hist[c];
    np += h;
    nb += (h + kFcBlock - 1) / kFcBlock;
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
    a.hist[c] = op;
    op += h;
    ob += (h + kFcBlock - 1) / kFcBlock;
  }
  if (tid == 1023) {
    a.cell_off[a.n_cells] = sp[cur][1023];
    a.blk_off[a.n_cells] = sb[cur][1023];
  }
}

template <class V>
__global__ __launch_bounds__(kFcInvThreads) void fc_scatter_kernel(FcArgsT<V> a) {
  extern __shared__ int cell_h[];
  const int q0 = (int)blockIdx.x * kFcSlice;
  for (int w0 = 0; w0 < a.n_cells; w0 += kFcWindow) {
    const int wn = a.n_cells - w0 < kFcWindow ? a.n_cells - w0 : kFcWindow;
    fc_count_slice(a, q0, w0, wn, cell_h);
    // one returning atomic per cell the slice lists: its h consecutive positions, the first of them left in LDS
    for (int c = (int)threadIdx.x; c < wn; c += kFcInvThreads) {
      const int h = cell_h[c];
      if (h) cell_h[c] = atomicAdd(&a.hist[w0 + c], h);
    }
    __syncthreads();
    fc_slice_pairs(a, q0, w0, [&](int q, int st, int sz, int c) {
      const int pos = atomicAdd(&cell_h[c - w0], 1);
      a.pairs[pos] = q;
      if (pos == a.cell_off[c]) {  // (every query lists the cell with the same extent)
        a.cell_st[c] = st;
        a.cell_sz[c] = sz;
      }
    });
  }
}

// ---- stage 4, what the candidate kernels share --------------------------------------------------------------------------
// the item's cell: the last c with blk_off[c] <= w (empty cells repeat their neighbour's prefix)
template <class V>
__device__ __forceinline__ int fc_item_cell(const FcArgsT<V>& a, int w) {
  int lo = 0, hi = a.n_cells;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.blk_off[mid] <= w) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- stage 5 ---------------------------------------------------------------------------------------------------------
template <int R, int METRIC, class Value, class V>
__global__ __launch_bounds__(256) void fc_finish_kernel(FcArgsT<V> a) {
  __shared__ float qv[4 * 64];
  __shared__ int qi[4 * 64];
  const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
  const int q = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
  if (q >= a.nq) return;  // (wave-uniform; the kernel has no barrier)
  if (a.flags[q] != 0) {
    if (lane == 0) atomicAdd(&a.ctrl[0], 1);
    return;
  }
  const int reserved = a.cnt[q];
  const int n = reserved < a.cand_cap ? reserved : a.cand_cap;
  WaveSelector<R> sel;
  sel.init(qv + wave * 64, qi + wave * 64, a.k);
  // the seeds, with the values they have (all of them read before the row is written below)
  for (int e0 = 0; e0 < a.k; e0 += 64) {
    const int e = e0 + lane;
    bool ok = false;
    float v = 0.f;
    int s = 0;
    if (e < a.k) {
      const int64_t ad = a.out_addr[(int64_t)q * a.k + e];
      if (ad >= 0) {
        ok = true;
        v = a.out_vals[(int64_t)q * a.k + e];
        s = (int)ad;
      }
    }
    sel.push(ok, v, s);
  }
  const int* __restrict__ list = a.cand + (int64_t)q * a.cand_cap;
  for (int e0 = 0; e0 < n; e0 += 64) {
    const int e = e0 + lane;
    const int s = e < n ? list[e] : -1;
    const bool live = s >= 0 && s < a.n_slots;  // (every stored entry is a slot of the storage)
    float v = 0.f;
    if (live) v = Value::template value<METRIC>(a, s, q);
    sel.push(live && (v >= sel.tau), v, s);  // (a NaN fails the test; -inf >= -inf enters)
  }
  sel.flush();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = r * 64 + lane;
    if (e < a.k) {
      const int idx = key_index(sel.top.k[r]);
      const bool pad = idx == kPadIdx;
      a.out_vals[(int64_t)q * a.k + e] = pad ? -INFINITY : key_value(sel.top.k[r]);
      a.out_addr[(int64_t)q * a.k + e] = pad ? -1 : (int64_t)idx;
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int fc_cus() {
  int dev = 0, n_cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cus <= 0)
    n_cus = 256;
  return n_cus;
}

// stages 2 ... 5 on `st`; launch_cand(grid) launches the unit's candidate kernel on that many persistent workgroups and
// returns its status.  stop: tpq_ivf_flat_cells_stop_after (0: all stages)
template <int METRIC, class Value, class V, class Prep, class Cand>
static int fc_launch(const FcArgsT<V>& a, Prep prep, int stop, hipStream_t st, Cand&& launch_cand) {
  hipLaunchKernelGGL((fc_seed_kernel<V, Prep>), dim3((unsigned)((a.nq > kFcCtrlInts ? a.nq : kFcCtrlInts) + 255) / 256),
                     dim3(256), 0, st, a, prep);
  TPQ_LAUNCH_CHECK("fc_seed_kernel");
  if (a.max_nprobe <= a.p0 || stop == 2) return TPQ_OK;  // nothing beyond P0: stage 1's rows are the result
  const int slices = (a.nq + kFcSlice - 1) / kFcSlice;
  const size_t inv_lds = (size_t)(a.n_cells < kFcWindow ? a.n_cells : kFcWindow) * 4;
  if (int rc = launch_with_lds(fc_count_kernel<V>, "fc_count_kernel", dim3(slices), dim3(kFcInvThreads), inv_lds, st, a))
    return rc;
  hipLaunchKernelGGL(fc_scan_kernel<V>, dim3(1), dim3(1024), 0, st, a);
  TPQ_LAUNCH_CHECK("fc_scan_kernel");
  if (int rc = launch_with_lds(fc_scatter_kernel<V>, "fc_scatter_kernel", dim3(slices), dim3(kFcInvThreads), inv_lds, st, a))
    return rc;
  if (stop == 3) return TPQ_OK;
  // at most one item per listed cell plus one per kFcBlock pairs
  const int64_t max_items = (int64_t)a.n_cells + ((int64_t)a.nq * (a.max_nprobe - a.p0)) / kFcBlock + 1;
  const int64_t slots = 2 * (int64_t)fc_cus();
  if (int rc = launch_cand(dim3((unsigned)(max_items < slots ? max_items : slots)))) return rc;
  if (stop == 4) return TPQ_OK;
  return with_list_regs(list_regs(a.k), [&](auto r_c) -> int {
    constexpr int R = decltype(r_c)::value < 4 ? decltype(r_c)::value : 4;  // (k <= 256)
    hipLaunchKernelGGL((fc_finish_kernel<R, METRIC, Value, V>), dim3((unsigned)(a.nq + 3) / 4), dim3(256), 0, st, a);
    TPQ_LAUNCH_CHECK("fc_finish_kernel");
    return TPQ_OK;
  });
}

// what the two entry points check, in this order, all before any HIP call; *go: the arguments are good and nq > 0
inline int fc_check(const char* what, bool pointers, int64_t n_slots, int n_cells, int d, int nq, int max_nprobe, int k,
                    int metric, int first_probe, int cand_cap, bool* go) {
  *go = false;
  if (int rc = check_batch(what, nq, max_nprobe)) return rc;
  TPQ_REQUIRE(d >= 1 && n_cells >= 1, "%s: d=%d n_cells=%d", what, d, n_cells);
  TPQ_REQUIRE(first_probe >= 1, "%s: first_probe=%d: the threshold pass needs a probe", what, first_probe);
  TPQ_REQUIRE(k >= 1, "%s: k=%d", what, k);
  if (k > 256 || cand_cap < 64 || cand_cap % 64 != 0) {
    set_error("%s: k=%d (1 ... 256), cand_cap=%d (a multiple of 64) is not supported", what, k, cand_cap);
    return TPQ_ERR_UNSUPPORTED;
  }
  if (int rc = check_lists(what, metric, 1, n_slots)) return rc;
  if (nq == 0) return TPQ_OK;
  if (int rc = check_grid(what, pointers, nq, 1)) return rc;
  TPQ_REQUIRE((int64_t)nq * cand_cap < 0x7fffffffLL * 4 && (int64_t)nq * max_nprobe < 0x7fffffffLL,
              "%s: nq=%d x cand_cap=%d or max_nprobe=%d is too large", what, nq, cand_cap, max_nprobe);
  *go = true;
  return TPQ_OK;
}

}  // namespace fcells
}  // namespace tpq
