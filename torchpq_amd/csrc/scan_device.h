// Device code of the IVF list scan (shared by scan.hip and the per-M scan_packed.hip units), one header per stage;
// scan.hip, scan_flat.hip and scan_pq4.hip add scan_ref.h (the reference-layout kernels, the split merge), which the per-M units do not parse.
#pragma once
#include "scan_args.h"           // ScanArgs, ResidualArgs, the modes of scan_packed_kernel (kDump*, TPQ_DUMP_PAIRS), TPQ_PROF, lds_poll_*
#include "scan_shared.h"         // wait_vmcnt, probe table, store_list / merge_list / write_final / finish_query, fused LUT, rank_merge
#include "scan_list.h"           // the frame of a list kernel (scan_ref.h, scan_flat.hip, scan_pq4.hip, scan_range.hip), check_lds, need_ws, scan_args
#include "scan_lut.h"            // stage_lut_blocked, lut16_compute / lut16_store
#include "scan_exact.h"          // LdsLut, ResidualLut, exact_from_* / exact_lane*
#include "scan_packed_kernel.h"  // packed_waves / packed_slots / packed_tile_shift, scan_packed_kernel
#include "scan_finish.h"         // finalize_and_write, scan_merge_refine_kernel, scan_finish_exact_kernel, scan_pool_merge_kernel

// per-M translation units (scan_packed.hip compiled with -DTPQ_PACKED_M=<M>)
// (keep the list in sync with build.sh and torchpq_amd/kernels PACKED_M)
#define TPQ_PACKED_M_LIST(X) \
  X(4) X(8) X(12) X(16) X(20) X(24) X(28) X(32) X(40) X(48) X(56) X(64) X(96) X(120) X(128)
#include "scan_host.h"           // list_regs*, *_lds_bytes*, pool_*, fill_ws*, validate, need_ws, set_lds, TPQ_DECLARE_PACKED
