// IVF list scan: the dispatch order of a large batch (scan_order.hip), as scan.hip sees it.
#pragma once
#include "common.h"

namespace tpq {

// The pairwise ranking is quadratic in the batch: 18 us at 10 000 queries (measured), hence ~75 us at 20 480
// -- against the ~0.17 ms the order saves, which does not grow with the batch (the ragged end is a fraction of one
// workgroup's lifetime).  Up to here the order keeps more than half of what it saves; larger batches keep index order.
constexpr int kOrderMaxQueries = 20480;

// order / rank / work: three int32 [nq], each rounded up to 256 bytes, behind the lists a dump-route call uses
inline size_t order_ws_bytes(int nq) { return 3 * (((size_t)nq * 4 + 255) & ~(size_t)255); }

// order[i] = the query dispatched i-th (work non-increasing, equal work by ascending query), rank = its inverse,
// work[q] = tiles of 2^tile_shift slots the query scans -- of its first `probe_cap` probes when that is positive
// (ScanArgs::probe_cap); two launches on `st`
int launch_scan_order(const int64_t* cell_start, const int64_t* cell_size, const int64_t* n_probe_list, int nq,
                      int max_nprobe, int tile_shift, int* order, int* rank, int* work, hipStream_t st,
                      int probe_cap);

}  // namespace tpq
