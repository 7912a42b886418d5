// IVF list scan: the look-up tables a packed-scan workgroup builds in LDS (fp32 in block order; 16-bit "sel16").
#pragma once
#include "scan_shared.h"

namespace tpq {

// jmax[j] (zeroed by the caller) collects max_c |LUT[j][c]| as the IEEE bit pattern of a
// non-negative float -- order-preserving as an unsigned, and LDS integer atomics are fast
// (float ones are not: DESIGN 3.5)
template <int M>
__device__ __forceinline__ void stage_lut_blocked(const ScanArgs& a, int q, float* lut,
                                                  int n_threads, unsigned* jmax, const float* xq,
                                                  const float* part1 = nullptr) {
  // thread handles (j, 4 consecutive c): 16-byte global load, 4 scalar LDS stores
  const float4* __restrict__ src = reinterpret_cast<const float4*>(a.lut);
  constexpr int m = M;
  // a wave-instruction covers JB sub-quantizers x 64/JB consecutive float4: 16 x 4 when m allows
  // (16 cache lines per load instead of one per lane, at the price of a 2-way bank conflict on the
  // stores: 1.2 % of the kernel in a same-box A/B; 8 x 8 and 32 x 2 measured slower), 8 x 8 or
  // 4 x 16 for m = 8 (mod 16) / 4 (mod 8)
  constexpr int JS = (m & 15) == 0 ? 4 : ((m & 7) == 0 ? 3 : 2);
  constexpr int JB = 1 << JS, CB = 64 >> JS;
  constexpr int jblocks = m >> JS;
  auto place = [&](int i, int& j, int& c4) {
    const int g = i >> 6, r = i & 63;
    const int jb = g % jblocks, cb4 = g / jblocks;
    j = jb * JB + (r & (JB - 1));
    c4 = cb4 * CB + (r >> JS);
  };
  auto put = [&](int j, int c4, const float4& x) {
    const int c = c4 * 4;
    lut[scan_layout::lut_dword(m, j, c + 0)] = x.x;
    lut[scan_layout::lut_dword(m, j, c + 1)] = x.y;
    lut[scan_layout::lut_dword(m, j, c + 2)] = x.z;
    lut[scan_layout::lut_dword(m, j, c + 3)] = x.w;
    const float mx = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
    atomicMax(&jmax[j], __float_as_uint(mx));
  };
  constexpr int DSM = M <= 32 ? 4 : 2;  // (m = 64 keeps 2 x 4 loads in flight: its eight-wave kernels sit at the VGPR cap)
  if (!part1 && !a.lut && a.ds <= DSM) {
    // fused table, short sub-vectors: a thread's entries come from ds codebook loads each, and a plain loop
    // pays one L2 round trip per entry group (8 groups per thread at m = 64: 4.6 of the 23 us a single-query
    // workgroup lives; 8.5 us when 512 workgroups stage at once).  All loads of U entry groups are issued first.
    // (round 6: ds = 3, 4 too -- SIFT's m = 32 walked its 8 groups per thread one round trip at a time: 14.2 of the
    // 15.5 us a workgroup of the reference grid's IVF4096 x 32 probes spent before its first tile)
    constexpr int U = TPQ_LUT_U;
    const int ds = a.ds;
    for (int i0 = threadIdx.x; i0 < m * 64; i0 += U * n_threads) {
      float4 y[U][DSM];
      int j[U], c4[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * n_threads;
        place(i < m * 64 ? i : i0, j[u], c4[u]);
        const float4* __restrict__ cb = reinterpret_cast<const float4*>(a.codebook) + (int64_t)j[u] * ds * 64 + c4[u];
#pragma unroll
        for (int e = 0; e < DSM; ++e) y[u][e] = e < ds ? cb[e * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + u * n_threads >= m * 64) break;
        float4 dot = make_float4(0.f, 0.f, 0.f, 0.f), c2 = dot;
        float q2 = 0.f;
#pragma unroll
        for (int e = 0; e < DSM; ++e) {
          if (e >= ds) break;
          const float4 yy = y[u][e];
          const float x = xq[j[u] * ds + e];
          q2 = fmaf(x, x, q2);
          dot.x = fmaf(x, yy.x, dot.x); dot.y = fmaf(x, yy.y, dot.y);
          dot.z = fmaf(x, yy.z, dot.z); dot.w = fmaf(x, yy.w, dot.w);
          c2.x = fmaf(yy.x, yy.x, c2.x); c2.y = fmaf(yy.y, yy.y, c2.y);
          c2.z = fmaf(yy.z, yy.z, c2.z); c2.w = fmaf(yy.w, yy.w, c2.w);
        }
        float4 v = dot;  // (fused_lut4's arithmetic, operation for operation)
        if (a.euclid) {
          v.x = 2.f * dot.x; v.y = 2.f * dot.y; v.z = 2.f * dot.z; v.w = 2.f * dot.w;
          if (a.euclid != 2) {
            v.x = v.x - q2; v.y = v.y - q2; v.z = v.z - q2; v.w = v.w - q2;
            v.x = v.x - c2.x; v.y = v.y - c2.y; v.z = v.z - c2.z; v.w = v.w - c2.w;
          }
        }
        put(j[u], c4[u], v);
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < m * 64; i += n_threads) {
    int j, c4;
    place(i, j, c4);
    const float4 x = part1 ? reinterpret_cast<const float4*>(part1)[((int64_t)q * m + j) * 64 + c4]
                     : a.lut ? src[((int64_t)j * a.nq + q) * 64 + c4]
                             : fused_lut4(a, j, c4, xq);
    put(j, c4, x);
  }
}

// ---- the 16-bit selection table ("sel16") -------------------------------------------------------------
// T[j][c] = round((LUT[j][c] + A_j) * inv), A_j = max_c |LUT[j][c]|, inv = 65535 / (2 max_j A_j): u16, laid out by
// scan_layout::lut16_halfword.  F(slot) = sum_j T[j][code_j] is an EXACT integer (< 2^24: carried as a float), and
// |F - (e_real + sum_j A_j) * inv| <= 0.51 m + 1 (per entry: the fp32 roundings of x * inv + (A_j * inv + 0.5), 0.008, and the
// rounding to an integer, 0.5; + 1 for the rounding of inv itself), so the selection band of the fp32 fast value
// carries over with delta = (0.51 m + 1) + (m - 1) u sum_j A_j * inv units.  Half the LDS of the fp32 table: four
// workgroups per CU at m = 64 instead of two.
// phase 1: the thread's M * 64 / NT float4 groups of entries (stage_lut_blocked's placement and, entry for entry, its
// arithmetic) into registers; the per-sub-quantizer maxima of |x| as BIT PATTERNS (NaN and Inf order above every
// finite value: the caller sees them in the maximum) into jmax
template <int M, int NT>
__device__ __forceinline__ void lut16_compute(const ScanArgs& a, int q, const float* xq, unsigned* jmax,
                                              float4 (&ent)[M * 64 / NT]) {
  constexpr int NE = M * 64 / NT;
  static_assert(M * 64 % NT == 0, "whole groups per thread");
  constexpr int JS = (M & 15) == 0 ? 4 : ((M & 7) == 0 ? 3 : 2);
  constexpr int JB = 1 << JS, CB = 64 >> JS;
  constexpr int jblocks = M >> JS;
  auto place = [&](int i, int& j, int& c4) {
    const int g = i >> 6, r = i & 63;
    const int jb = g % jblocks, cb4 = g / jblocks;
    j = jb * JB + (r & (JB - 1));
    c4 = cb4 * CB + (r >> JS);
  };
  auto note = [&](int j, const float4& x) {
    const unsigned b0 = __float_as_uint(x.x) & 0x7fffffffu, b1 = __float_as_uint(x.y) & 0x7fffffffu;
    const unsigned b2 = __float_as_uint(x.z) & 0x7fffffffu, b3 = __float_as_uint(x.w) & 0x7fffffffu;
    const unsigned m01 = b0 > b1 ? b0 : b1, m23 = b2 > b3 ? b2 : b3;
    atomicMax(&jmax[j], m01 > m23 ? m01 : m23);
  };
  const float4* __restrict__ src = reinterpret_cast<const float4*>(a.lut);
  if (!a.lut && a.ds <= 2) {
    constexpr int U = 4;
    static_assert(NE % U == 0, "batches of four");
    const int ds = a.ds;
#pragma unroll
    for (int u0 = 0; u0 < NE; u0 += U) {
      float4 y[U][2];
      int j[U], c4[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        place((int)threadIdx.x + (u0 + u) * NT, j[u], c4[u]);
        const float4* __restrict__ cb = reinterpret_cast<const float4*>(a.codebook) + (int64_t)j[u] * ds * 64 + c4[u];
        y[u][0] = cb[0];
        y[u][1] = ds > 1 ? cb[64] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float4 dot = make_float4(0.f, 0.f, 0.f, 0.f), c2 = dot;
        float q2 = 0.f;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (e >= ds) break;
          const float4 yy = y[u][e];
          const float x = xq[j[u] * ds + e];
          q2 = fmaf(x, x, q2);
          dot.x = fmaf(x, yy.x, dot.x); dot.y = fmaf(x, yy.y, dot.y);
          dot.z = fmaf(x, yy.z, dot.z); dot.w = fmaf(x, yy.w, dot.w);
          c2.x = fmaf(yy.x, yy.x, c2.x); c2.y = fmaf(yy.y, yy.y, c2.y);
          c2.z = fmaf(yy.z, yy.z, c2.z); c2.w = fmaf(yy.w, yy.w, c2.w);
        }
        float4 v = dot;  // (fused_lut4's arithmetic, operation for operation)
        if (a.euclid) {
          v.x = 2.f * dot.x; v.y = 2.f * dot.y; v.z = 2.f * dot.z; v.w = 2.f * dot.w;
          if (a.euclid != 2) {
            v.x = v.x - q2; v.y = v.y - q2; v.z = v.z - q2; v.w = v.w - q2;
            v.x = v.x - c2.x; v.y = v.y - c2.y; v.z = v.z - c2.z; v.w = v.w - c2.w;
          }
        }
        ent[u0 + u] = v;
        note(j[u], v);
      }
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    int j, c4;
    place((int)threadIdx.x + u * NT, j, c4);
    ent[u] = a.lut ? src[((int64_t)j * a.nq + q) * 64 + c4] : fused_lut4(a, j, c4, xq);
    note(j, ent[u]);
  }
}
// phase 2 (after a barrier: jmax is complete): quantise and store
template <int M, int NT>
__device__ __forceinline__ void lut16_store(const float4 (&ent)[M * 64 / NT], const unsigned* jmax, float inv,
                                            uint16_t* lut16) {
  constexpr int NE = M * 64 / NT;
  constexpr int JS = (M & 15) == 0 ? 4 : ((M & 7) == 0 ? 3 : 2);
  constexpr int JB = 1 << JS, CB = 64 >> JS;
  constexpr int jblocks = M >> JS;
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int i = (int)threadIdx.x + u * NT;
    const int g = i >> 6, r = i & 63;
    const int j = (g % jblocks) * JB + (r & (JB - 1));
    const int c = ((g / jblocks) * CB + (r >> JS)) * 4;
    // T = trunc(x * inv + (A_j * inv + 0.5)): ONE fma per entry (round 6; it was add, multiply, add, min -- the scan is
    // VALU-issue-bound).  |x| <= A_j, so the real value lies in [0.5, 65535.5]; roundings: the fma's (half an
    // ulp at < 2^16: 2^-8) and the constant's two (2^-9 each) -- the 0.008 the band's 0.51 per entry allows for; the
    // truncation of a value in (0.49, 65535.51) needs no clamp.
    const float k0 = __uint_as_float(jmax[j]) * inv + 0.5f;
    auto qz = [&](float x) -> uint16_t { return (uint16_t)(unsigned)fmaf(x, inv, k0); };
    lut16[scan_layout::lut16_halfword(M, j, c + 0)] = qz(ent[u].x);
    lut16[scan_layout::lut16_halfword(M, j, c + 1)] = qz(ent[u].y);
    lut16[scan_layout::lut16_halfword(M, j, c + 2)] = qz(ent[u].z);
    lut16[scan_layout::lut16_halfword(M, j, c + 3)] = qz(ent[u].w);
  }
}

}  // namespace tpq
