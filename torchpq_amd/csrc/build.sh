#!/bin/bash
# Builds libtorchpq_amd.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
# Incremental: every object carries the compiler's own dependency list (build/<obj>.d, -MD), so a change to
# one of the scan headers (scan_device.h and the per-stage scan_*.h it includes) rebuilds the scan units only -- not the
# k-means / cascade units, which take the longest -- and scan_ref.h (the reference-layout kernels) scan.hip, scan_flat.hip and
# scan_pq4.hip alone (the 4-bit list scan takes scan_device.h and scan_ref.h as scan_flat.hip does, so every scan header rebuilds it;
# scan_pq4.h, its word loop and grouped tables, is shared with scan_pq4_filtered.hip, the filtered 4-bit scan, and scan_pq4_range.hip,
# the 4-bit range search, and rebuilds those three);
# scan_list.h (the frame of a list kernel) is included by scan_ref.h, scan_range.hip and, for clamped_n_probe, scan_packed_kernel.h,
# so a change to it rebuilds every scan unit; scan_range.hip (IVFPQ range search) takes scan_list.h, scan_shared.h and
# scan_args.h only, so the other scan headers -- the packed ones above all -- leave it alone; scan_filtered.hip (the filtered
# top-k scan) takes scan_ref.h for the split merge and, through it, the same three;
# scan_order.hip (the large batches' dispatch order) takes scan_order.h alone, which scan.hip shares; scan_cells.hip (the
# cell-major candidates of the m = 64 large-batch route) takes scan_cells.h, which scan.hip shares, mfma_util.h, wave_topk.h and scan_fk.h (the k-th key search, shared with scan_finish.h); fp16_cascade.h
# rebuilds the four cascade units (cascade_core, assign_cascade, probe_sims, lloyd) and assign_fast; row_select.h (the
# row select's device code) rebuilds select, coarse_probe and probe_sims; probe_fast.h rebuilds coarse_probe and
# probe_sims; mfma_util.h (the MFMA units' shared device helpers) rebuilds the cascade units, assign_fast, coarse_probe,
# max_sim, centroid_update, kmeans_split, lut, flat_topk and flat_range; sims_chunk.h (the fp32 similarity tile) rebuilds
# coarse_probe, flat_topk and flat_range.  The exact assign (max_sim.hip) and the centroid update
# (centroid_update.hip) are units of their own: a change to one does not recompile the other.
# The library is linked from the objects of the unit list below, not from whatever build/ holds: an object left
# behind by a unit that has since been renamed or split would define its symbols a second time.
# FORCE=1 rebuilds everything; JOBS=n bounds the parallel compiles (default: the host's cores).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${HERE}/../libtorchpq_amd.so"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math
       -Wall -Wno-unused-function -Wno-unused-variable -DNDEBUG)
JOBS="${JOBS:-$(nproc)}"
mkdir -p "${HERE}/build"
cd "${HERE}"   # (dependency files written by hand-run compiles may hold paths relative to this directory)
# a change of flags rebuilds everything (the flags of the last build are kept next to the objects)
FLAGLINE="${FLAGS[*]} ${EXTRA_FLAGS:-}"
if [[ ! -f "${HERE}/build/flags.txt" || "$(cat "${HERE}/build/flags.txt")" != "$FLAGLINE" ]]; then FORCE=1; fi
stale() {  # object missing, or older than any file its last compile read?
  local obj="$1" src="$2" dep="${1%.o}.d" f
  [[ "${FORCE:-0}" == "1" || ! -f "$obj" || ! -f "$dep" || "$obj" -ot "$src" ]] && return 0
  # the .d file: "obj: dep dep \" lines; every existing dependency must be older than the object
  for f in $(sed -e 's/^[^:]*://' -e 's/\\$//' "$dep"); do
    [[ -f "$f" && "$obj" -ot "$f" ]] && return 0
  done
  return 1
}
cmds=()
objs=()
# the scan-layout kernels: one translation unit per sub-quantizer count
for m in 64 120 128 96 56 48 40 32 28 24 20 16 12 8 4; do  # = TPQ_PACKED_M_LIST (scan_device.h), longest first
  obj="${HERE}/build/scan_packed_${m}.o"
  objs+=("$obj")
  if stale "$obj" "${HERE}/scan_packed.hip"; then
    cmds+=("'$HIPCC' ${FLAGS[*]} -DTPQ_PACKED_M=${m} -MD -MF '${obj%.o}.d' -x hip -c '${HERE}/scan_packed.hip' -o '$obj' ${EXTRA_FLAGS:-}")
  fi
done
for src in cascade_core.hip select.hip coarse_probe.hip max_sim.hip centroid_update.hip assign_cascade.hip assign_fast.hip probe_sims.hip lloyd.hip scan.hip scan_order.hip scan_cells.hip scan_flat.hip scan_pq4.hip scan_pq4_filtered.hip scan_pq4_range.hip scan_range.hip scan_filtered.hip kmeans_split.hip container.hip lut.hip pack.hip rerank.hip flat_topk.hip flat_range.hip ubench.hip api.cpp; do
  obj="${HERE}/build/${src%.*}.o"
  objs+=("$obj")
  if stale "$obj" "${HERE}/${src}"; then
    cmds+=("'$HIPCC' ${FLAGS[*]} -MD -MF '${obj%.o}.d' -x hip -c '${HERE}/${src}' -o '$obj' ${EXTRA_FLAGS:-}")
  fi
done
if (( ${#cmds[@]} )); then
  echo "compiling ${#cmds[@]} unit(s), ${JOBS} at a time"
  printf '%s\n' "${cmds[@]}" | xargs -d '\n' -n 1 -P "${JOBS}" bash -c || { echo "compile failed" >&2; exit 1; }
fi
echo "$FLAGLINE" > "${HERE}/build/flags.txt"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -Wl,-z,defs -o "$OUT" "${objs[@]}"
echo "built $OUT"
