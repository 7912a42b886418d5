// Device-side pieces the MFMA units share (the assign / k-means family, the fp16 cascade, coarse_probe.hip, lut.hip):
// operand vector types, the compile-time loop, the loads-ahead block of a sequential chain, the exact bf16 split and its constant fragments, the wave-aggregated
// list append.  All force-inlined: a unit's kernels own every instruction they run.
#pragma once
#include <type_traits>

#include "common.h"

namespace tpq {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// compile-time loop: f(integral_constant<int, I>) for I in [I0, I1)
template <int I0, int I1, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I0 < I1) {
    f(std::integral_constant<int, I0>{});
    static_for<I0 + 1, I1>(f);
  }
}

// A block of a chain that is sequential in k while its loads are not: N loads issued together, then use(u, y_u) in
// ascending u.
template <int N, class L, class U>
__device__ __forceinline__ void load_then_use(L&& load, U&& use) {
  decltype(load(0)) y[N];
#pragma unroll
  for (int u = 0; u < N; ++u) y[u] = load(u);
#pragma unroll
  for (int u = 0; u < N; ++u) use(u, y[u]);
}

// x -> (p1, p2, p3), exact: x == p1 + p2 + p3 (3 x 8 significant bits, round to nearest even)
__device__ __forceinline__ void split3_bf16(float x, __bf16& p1, __bf16& p2, __bf16& p3) {
  p1 = (__bf16)x;
  const float r1 = x - (float)p1;
  p2 = (__bf16)r1;
  const float r2 = r1 - (float)p2;
  p3 = (__bf16)r2;
}

// B fragment of ones at k = 0, 1, 2 (the lanes of k-group 0: half == 0), zero elsewhere: against an A fragment that
// holds the three pieces of a number per row at k = 0, 1, 2 one bf16 MFMA adds that number to every column
__device__ __forceinline__ bf16x8 ones3_bf16x8(int half) {
  bf16x8 ones = {0, 0, 0, 0, 0, 0, 0, 0};
  if (half == 0) {
    ones[0] = (__bf16)1.0f;
    ones[1] = (__bf16)1.0f;
    ones[2] = (__bf16)1.0f;
  }
  return ones;
}

// a zero 32 x 32 accumulator (as an MFMA's C operand it is the inline constant 0)
__device__ __forceinline__ f32x16 zero_f32x16() {
  return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// Wave-aggregated append: EVERY lane of the wave calls it; the lanes with `take` set receive consecutive slots
// counted from *counter (an LDS or a global counter), reserved by one atomic of the first such lane, and return
// true.  The caller bounds the slot against its list's capacity.
__device__ __forceinline__ bool wave_append(bool take, int* counter, int& slot) {
  const unsigned long long mk = __ballot(take);
  if (!mk) return false;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mk) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(mk));
  base = __shfl(base, leader, 64);
  slot = base + __popcll(mk & ((1ull << lane) - 1ull));
  return take;
}

}  // namespace tpq
