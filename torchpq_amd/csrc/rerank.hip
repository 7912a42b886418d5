// Re-rank step of IVFPQRIndex (tpq_ivfpqr_rerank): the k1 candidates the list scan returned for a query are
// re-valued from BOTH codes of their slot (first-stage code + re-rank code of its residual) and the best k kept.
//
// One workgroup takes a group of queries (as many as give it up to 1 024 (query, candidate) pairs) and walks the
// dimensions in order, 16 at a time: the 16 rows of both codebooks ([d][256] f32 each, 16 KiB per slice) are
// staged in LDS, every pair looks its two centroids' components up there and carries its accumulator across the
// slices in a register -- the summation order of the value definition (include/torchpq_amd.h) is the loop order.
// Nothing of size [nq, k1, d] is ever written.  The final selection ranks the k1 keys of a query against each
// other in LDS (a 64-bit key per candidate: value image, then ~address -- wave_topk.h's order) and every
// candidate of rank < k writes its own output row.
#include "common.h"
#include "wave_topk.h"

namespace tpq {
namespace rerank {

constexpr int kThreads = 256;
constexpr int kPairsPerThread = 4;
constexpr int kMaxPairs = kThreads * kPairsPerThread;  // = the largest k1
constexpr int kDimChunk = 16;                          // dimensions per staged codebook slice
constexpr int kMaxQueries = 64;                        // queries per workgroup
constexpr int kQStride = kDimChunk + 1;                // odd: lanes of different queries hit different banks

enum Mode { kResidualL2 = 0, kResidualDot = 1, kLutL2 = 2, kLutDot = 3 };

inline int queries_per_group(int k1) {
  const int q = kMaxPairs / k1;
  return q < 1 ? 1 : (q > kMaxQueries ? kMaxQueries : q);
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void rerank_kernel(
    const uint32_t* __restrict__ storage,  // [(m + m_r) / 4][capacity] words of 4 codes
    int64_t capacity, int m, int ds, int ds_r,
    const float* __restrict__ cb,          // [d][256] (= [m][ds][256]); unused by the LUT modes
    const float* __restrict__ cbr,         // [d][256] (= [m_r][ds_r][256])
    const float* __restrict__ query,       // [d][nq]
    int d, int nq, int group, const int64_t* __restrict__ cand, int k1, int k,
    const int64_t* __restrict__ address2id, float* __restrict__ out_vals, int64_t* __restrict__ out_address,
    int64_t* __restrict__ out_ids) {
  constexpr bool kResidual = MODE == kResidualL2 || MODE == kResidualDot;
  __shared__ float s_cb[kResidual ? kDimChunk * 256 : 4];
  __shared__ float s_cbr[kDimChunk * 256];
  __shared__ float s_q[kMaxQueries * kQStride];
  __shared__ unsigned long long s_key[kMaxPairs];

  const int tid = (int)threadIdx.x;
  const int q0 = (int)blockIdx.x * group;
  const int n_q = min(group, nq - q0);
  const int n_pairs = n_q * k1;

  int ql[kPairsPerThread];     // query of the pair, local to the group
  int adr[kPairsPerThread];    // slot address (< 2^31), 0 when there is no candidate
  bool real[kPairsPerThread];  // a candidate with an address inside the storage
  float acc[kPairsPerThread], dot[kPairsPerThread], c2[kPairsPerThread], q2[kPairsPerThread];
  uint32_t w[kPairsPerThread], wr[kPairsPerThread];
#pragma unroll
  for (int t = 0; t < kPairsPerThread; ++t) {
    const int p = tid + t * kThreads;
    ql[t] = 0;
    adr[t] = 0;
    real[t] = false;
    if (p < n_pairs) {
      ql[t] = p / k1;
      const int64_t a = cand[(int64_t)q0 * k1 + p];
      real[t] = a >= 0 && a < capacity;
      adr[t] = real[t] ? (int)a : 0;
    }
    acc[t] = dot[t] = c2[t] = q2[t] = 0.f;
    w[t] = wr[t] = 0u;
  }

  int j = 0, rem = 0, jr = 0, rem_r = 0;  // sub-quantizer and offset inside it, per codebook (uniform)
  for (int i0 = 0; i0 < d; i0 += kDimChunk) {
    const int n = min(kDimChunk, d - i0);
    __syncthreads();  // the previous slice is no longer read
    for (int e = tid * 4; e < n * 256; e += kThreads * 4) {
      if constexpr (kResidual)
        *reinterpret_cast<float4*>(s_cb + e) = *reinterpret_cast<const float4*>(cb + (int64_t)i0 * 256 + e);
      *reinterpret_cast<float4*>(s_cbr + e) = *reinterpret_cast<const float4*>(cbr + (int64_t)i0 * 256 + e);
    }
    for (int e = tid; e < n_q * n; e += kThreads) {
      const int qq = e / n, ii = e - qq * n;
      s_q[qq * kQStride + ii] = query[(int64_t)(i0 + ii) * nq + q0 + qq];
    }
    __syncthreads();
    for (int ii = 0; ii < n; ++ii) {
      if constexpr (kResidual) {
        if (rem == 0 && (j & 3) == 0) {
#pragma unroll
          for (int t = 0; t < kPairsPerThread; ++t)
            w[t] = real[t] ? storage[(int64_t)(j >> 2) * capacity + adr[t]] : 0u;
        }
      }
      if (rem_r == 0 && (jr & 3) == 0) {
#pragma unroll
        for (int t = 0; t < kPairsPerThread; ++t)
          wr[t] = real[t] ? storage[(int64_t)((m + jr) >> 2) * capacity + adr[t]] : 0u;
      }
      const int sh = 8 * (j & 3), sh_r = 8 * (jr & 3);
#pragma unroll
      for (int t = 0; t < kPairsPerThread; ++t) {
        const float x = s_q[ql[t] * kQStride + ii];
        const float y = s_cbr[ii * 256 + ((wr[t] >> sh_r) & 255u)];
        if constexpr (kResidual) {
          const float r = __fadd_rn(s_cb[ii * 256 + ((w[t] >> sh) & 255u)], y);
          if constexpr (MODE == kResidualL2) {
            const float u = __fsub_rn(x, r);
            acc[t] = __fsub_rn(acc[t], __fmul_rn(u, u));
          } else {
            acc[t] = __fadd_rn(acc[t], __fmul_rn(x, r));
          }
        } else {  // one entry of the ADC table of the re-rank codec, in tpq_adc_lut's arithmetic
          dot[t] = __fmaf_rn(x, y, dot[t]);
          if constexpr (MODE == kLutL2) {
            c2[t] = __fmaf_rn(y, y, c2[t]);
            q2[t] = __fmaf_rn(x, x, q2[t]);
          }
        }
      }
      if (++rem == ds) {
        rem = 0;
        ++j;
      }
      if (++rem_r == ds_r) {
        rem_r = 0;
        ++jr;
        if constexpr (!kResidual) {
#pragma unroll
          for (int t = 0; t < kPairsPerThread; ++t) {
            float r = dot[t];
            if constexpr (MODE == kLutL2) {
              r = __fmul_rn(2.f, r);
              r = __fsub_rn(r, q2[t]);
              r = __fsub_rn(r, c2[t]);
            }
            acc[t] = __fadd_rn(acc[t], r);
            dot[t] = c2[t] = q2[t] = 0.f;
          }
        }
      }
    }
  }

  // selection: (value descending, address ascending, position ascending); a missing candidate is (-inf, pad)
#pragma unroll
  for (int t = 0; t < kPairsPerThread; ++t) {
    const int p = tid + t * kThreads;
    acc[t] = real[t] ? acc[t] + 0.f : -INFINITY;
    if (p < n_pairs)
      s_key[p] = ((unsigned long long)f2key(acc[t]) << 32) | (unsigned)~(unsigned)(real[t] ? adr[t] : kPadIdx);
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kPairsPerThread; ++t) {
    const int p = tid + t * kThreads;
    if (p >= n_pairs) continue;
    const int seg = ql[t] * k1, c = p - seg;
    const unsigned long long mine = s_key[p];
    int rank = 0;
    for (int f = 0; f < k1; ++f) {
      const unsigned long long other = s_key[seg + f];
      rank += (other > mine || (other == mine && f < c)) ? 1 : 0;
    }
    if (rank < k) {
      const int64_t o = (int64_t)(q0 + ql[t]) * k + rank;
      out_vals[o] = acc[t];
      out_address[o] = real[t] ? (int64_t)adr[t] : -1;
      if (out_ids) out_ids[o] = real[t] ? address2id[adr[t]] : -1;
    }
  }
}

}  // namespace rerank
}  // namespace tpq

using namespace tpq;

extern "C" int tpq_ivfpqr_rerank(const uint8_t* storage, int64_t capacity, int m, int m_r, const float* codebook,
                                 const float* codebook_r, const float* query, int d, int nq,
                                 const int64_t* cand_address, int k1, int k, int use_residual, int distance,
                                 const int64_t* address2id, float* out_vals, int64_t* out_address,
                                 int64_t* out_ids, tpq_stream_t stream) {
  TPQ_REQUIRE(nq >= 0, "ivfpqr_rerank: nq=%d", nq);
  if (nq == 0) return TPQ_OK;
  TPQ_REQUIRE(storage && codebook_r && query && cand_address && out_vals && out_address,
              "ivfpqr_rerank: null pointer");
  TPQ_REQUIRE(!use_residual || codebook, "ivfpqr_rerank: use_residual needs the first-stage codebook");
  TPQ_REQUIRE((out_ids == nullptr) == (address2id == nullptr), "ivfpqr_rerank: out_ids and address2id go together");
  TPQ_REQUIRE(m >= 4 && m % 4 == 0 && m_r >= 4 && m_r % 4 == 0,
              "ivfpqr_rerank: n_subvectors=%d / n_subvectors_rerank=%d must be positive multiples of 4", m, m_r);
  TPQ_REQUIRE(d > 0 && d % m == 0 && d % m_r == 0, "ivfpqr_rerank: d=%d is not a multiple of m=%d and m_r=%d", d, m,
              m_r);
  TPQ_REQUIRE(1 <= k && k <= k1, "ivfpqr_rerank: need 1 <= k=%d <= k1=%d", k, k1);
  TPQ_REQUIRE(distance == TPQ_METRIC_NEG_SQ_L2 || distance == TPQ_METRIC_INNER, "ivfpqr_rerank: distance=%d",
              distance);
  TPQ_REQUIRE(capacity > 0, "ivfpqr_rerank: capacity=%lld", (long long)capacity);
  TPQ_REQUIRE(((uintptr_t)codebook | (uintptr_t)codebook_r | (uintptr_t)storage) % 16 == 0,
              "ivfpqr_rerank: storage and codebooks must be 16-byte aligned");
  if (k1 > rerank::kMaxPairs || capacity >= (int64_t)kPadIdx) {
    set_error("ivfpqr_rerank: k1=%d > %d or capacity=%lld >= 2^31-1 is not supported", k1, rerank::kMaxPairs,
              (long long)capacity);
    return TPQ_ERR_UNSUPPORTED;
  }
  const int group = rerank::queries_per_group(k1);
  const dim3 grid((unsigned)ceil_div(nq, group)), block(rerank::kThreads);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(storage);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ds = d / m, ds_r = d / m_r;
  const int mode = use_residual ? (distance == TPQ_METRIC_NEG_SQ_L2 ? rerank::kResidualL2 : rerank::kResidualDot)
                                : (distance == TPQ_METRIC_NEG_SQ_L2 ? rerank::kLutL2 : rerank::kLutDot);
#define TPQ_RERANK_LAUNCH(MODE)                                                                                   \
  hipLaunchKernelGGL(rerank::rerank_kernel<MODE>, grid, block, 0, s, words, capacity, m, ds, ds_r, codebook,      \
                     codebook_r, query, d, nq, group, cand_address, k1, k, address2id, out_vals, out_address,     \
                     out_ids)
  switch (mode) {
    case rerank::kResidualL2: TPQ_RERANK_LAUNCH(rerank::kResidualL2); break;
    case rerank::kResidualDot: TPQ_RERANK_LAUNCH(rerank::kResidualDot); break;
    case rerank::kLutL2: TPQ_RERANK_LAUNCH(rerank::kLutL2); break;
    default: TPQ_RERANK_LAUNCH(rerank::kLutDot); break;
  }
#undef TPQ_RERANK_LAUNCH
  TPQ_LAUNCH_CHECK("rerank_kernel");
  return TPQ_OK;
}
