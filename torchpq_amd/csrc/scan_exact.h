// IVF list scan: exact (ascending-j) re-evaluation of a slot from its packed bytes.
#pragma once
#include "scan_args.h"

namespace tpq {

template <int M>
struct LdsLut {
  const float* lut;
  __device__ __forceinline__ float operator()(int j, unsigned c) const {
    return lut[scan_layout::lut_dword(M, j, (int)c)];
  }
};
// residual PQ: entry = part1 (LDS) + part2[cell] (global, L2-resident), rounded like the LUT the
// reference builds per probe (load_precomputed_v3, ivfpq_topk.cu:522-560)
template <int M>
struct ResidualLut {
  const float* lut;
  const float* part2_cell;  // this lane's cell: [M][256]
  __device__ __forceinline__ float operator()(int j, unsigned c) const {
    return lut[scan_layout::lut_dword(M, j, (int)c)] + part2_cell[j * 256 + (int)c];
  }
};
// Exact (ascending-j) value of slot `idx` from its PACKED bytes: the lane un-permutes its slot
// into sub-quantizer order through a private LDS row (stride M/4+1 dwords: conflict-free), then
// sums LUT entries in the reference's order.
template <int M, class LutFn>
__device__ __forceinline__ float exact_from_chunks(const typename scan_layout::Layout<M>::chunk_t (&w)[scan_layout::Layout<M>::kChunks],
                                                   int idx, bool active, uint32_t* scratch, int row_id,
                                                   const LutFn& lutfn, float init = 0.f) {
  using L = scan_layout::Layout<M>;
  constexpr int G = M / 4;
  uint32_t* row = scratch + row_id * (G + 1);
  if (active) {
#pragma unroll
    for (int d = 0; d < G; ++d) {
      const scan_layout::BlockAt<M> kb(4 * d);
      const int sb = idx & (kb.size - 1);
      const uint32_t x = (uint32_t)(sb & 3);
      const uint32_t sel = 0x03020100u ^ (x * 0x01010101u);  // out.byte[k] = in.byte[k ^ x]
      const uint32_t wd = L::word(w, d);
      const int dst = (kb.base >> 2) + ((d - (kb.base >> 2)) ^ (sb >> 2));
      row[dst] = __builtin_amdgcn_perm(wd, wd, sel);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  float v = init;
  if (active) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint32_t wd = row[g];
      v += lutfn(4 * g + 0, wd & 255u);
      v += lutfn(4 * g + 1, (wd >> 8) & 255u);
      v += lutfn(4 * g + 2, (wd >> 16) & 255u);
      v += lutfn(4 * g + 3, wd >> 24);
    }
  }
  return active ? v : -INFINITY;
}
template <int M, class LutFn>
__device__ __forceinline__ float exact_from_packed(const uint8_t* __restrict__ packed,
                                                   int64_t n_slots, int idx, bool active,
                                                   uint32_t* scratch, int row_id,
                                                   const LutFn& lutfn, float init = 0.f) {
  using L = scan_layout::Layout<M>;
  typename L::chunk_t w[L::kChunks] = {};
  if (active) L::load(packed, n_slots, idx, w);
  return exact_from_chunks<M>(w, idx, active, scratch, row_id, lutfn, init);
}

// The same value with EVERY lane evaluating a slot of its own and no LDS row (plain PQ, LUT in LDS).  The packed layout
// stores sub-quantizer j of slot s at byte position j ^ (s mod block) so that the scan's lanes read 64 different LUT
// rows at a time; 64 candidates summed in sub-quantizer order would all read the SAME row at a time (one bank, 64-way).
// So, sixteen sub-quantizers at a time: the lane picks the four code dwords that hold them (the XOR's high bits move
// whole groups of 16: a select among the block's groups), fetches their LUT entries in POSITION order -- the XOR's low
// four bits spread the lanes over 16 rows --, brings the VALUES (not the codes) into sub-quantizer order with a butterfly
// of conditional swaps on those four bits, and adds them ascending j: the reference's order, hence its bits.  One pass
// for 64 candidates where the LDS-row form took 64 / refine_rows passes of a 64-step dependent LDS chain each (~3 us a
// pass); sixteen values live at a time (all 64 at once spilled registers into the scan's tile loop).  Used by the pool
// mode's drains (64 candidates at a time).  NOT by the short lists' refinement: at k = 100 a wave has ~10 candidates and
// one LDS-row pass is the faster form; carrying both forms put 25 more scratch reloads into every query's finish of the
// k <= 248 kernels -- 3 % at C2, 8-15 % on the reference grid's short cells, same box (k = 500: +7 %).  (Not code size:
// the same kernels without their in-kernel redo, 53 -> 39 KB, run no faster.)
template <int M, int BASE>
__device__ __forceinline__ float exact_lane_blocks(const typename scan_layout::Layout<M>::chunk_t (&w)[scan_layout::Layout<M>::kChunks],
                                                   int idx, const float* __restrict__ lut, float v) {
  using L = scan_layout::Layout<M>;
  if constexpr (BASE >= M) {
    return v;
  } else {
    constexpr int S = scan_layout::block_of(M, BASE).size;
    constexpr int GS = S < 16 ? S : 16;   // sub-quantizers per group
    constexpr int NG = S / GS;            // groups in the block
    constexpr int DW = GS / 4;            // dwords per group
    const int xs = idx & (S - 1);
    const int xg = xs / GS, xl = xs & (GS - 1);
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      // sub-quantizers BASE + GS q ... + GS - 1 live at positions of group q ^ xg
      uint32_t cd[DW];
#pragma unroll
      for (int t = 0; t < DW; ++t) {
        cd[t] = L::word(w, BASE / 4 + (q ^ 0) * DW + t);
#pragma unroll
        for (int x = 1; x < NG; ++x) cd[t] = (xg == x) ? L::word(w, BASE / 4 + (q ^ x) * DW + t) : cd[t];
      }
      float val[GS];
#pragma unroll
      for (int p = 0; p < GS; ++p) {
        const uint32_t c = (cd[p >> 2] >> (8 * (p & 3))) & 255u;
        // position GS (q ^ xg) + p holds sub-quantizer BASE + GS q + (p ^ xl): lut_dword(M, that, c)
        val[p] = lut[BASE * 256 + (int)c * S + GS * q + (p ^ xl)];
      }
#pragma unroll
      for (int b = 1; b < GS; b <<= 1) {
        const bool sw = (xl & b) != 0;
#pragma unroll
        for (int p = 0; p < GS; ++p) {
          if ((p & b) == 0) {
            const float lo = val[p], hi = val[p | b];
            val[p] = sw ? hi : lo;
            val[p | b] = sw ? lo : hi;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < GS; ++j) v += val[j];
    }
    return exact_lane_blocks<M, BASE + S>(w, idx, lut, v);
  }
}
template <int M>
__device__ __forceinline__ float exact_lane(const typename scan_layout::Layout<M>::chunk_t (&w)[scan_layout::Layout<M>::kChunks],
                                            int idx, const float* __restrict__ lut) {
  return exact_lane_blocks<M, 0>(w, idx, lut, 0.f);
}

}  // namespace tpq
