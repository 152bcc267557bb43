// Device helpers shared by K33 (embed_search.hip) and K34 (embed_search_q8.hip):
// the bf16x3 product step, the hi / lo split of a query, K19's key and the
// sorted-over-the-lanes insert.  Moved here unchanged from K33.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/common.h"

// K33's entry points that K35 (embed_search_ivf.hip) calls: the whole search
// for its coarse step, the merge launch for its key lists
extern "C" {
uint64_t tcamd_search_workspace(int rows, int N);
int tcamd_search_topk(const float* q, uint64_t q_stride_bytes, int rows, const void* idx_hi, const void* idx_lo, int N,
                      int D, const int32_t* k_row, int kmax, void* workspace, int32_t* indices, float* scores,
                      void* stream);
int tcamd_search_merge(const void* ws, const int32_t* k_row, int rows, int slices, int kmax, int32_t* indices,
                       float* scores, void* stream);
}

namespace tcamd_search {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4u ld16(const void* p) { return *reinterpret_cast<const v4u*>(p); }
__device__ __forceinline__ bf16x8 fr(v4u v) { return __builtin_bit_cast(bf16x8, v); }

// 16-B chunk c of staged row r sits at chunk c ^ swz(r)
__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

// bf16x3 product, the two small cross terms first (x3_mma of K10c)
__device__ __forceinline__ f32x4 x3_mma(v4u ah, v4u al, v4u bh, v4u bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr(al), fr(bh), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr(ah), fr(bl), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr(ah), fr(bh), c, 0, 0, 0);
}

// K19's key (topk_key of csrc/kernels/topk.hip)
__device__ __forceinline__ uint64_t topk_key(uint32_t bits, uint32_t idx) {
  uint32_t m;
  if ((bits & 0x7fffffffu) > 0x7f800000u) {
    m = 0u;  // NaN: below -inf (whose image is 0x007fffff)
  } else {
    if (bits == 0x80000000u) bits = 0u;  // -0.0 ties with +0.0
    m = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return ((uint64_t)m << 32) | (uint64_t)(0xFFFFFFFFu - idx);
}

// the fp32 bits back out of a key's monotone image (both zeros come back as +0.0)
__device__ __forceinline__ float key_score(uint64_t key) {
  const uint32_t m = (uint32_t)(key >> 32);
  return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

// ... and K19's butterfly (wave_max_u64)
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// lane `l` (wave-uniform) of a 64-bit value
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// `cand` into the keys sorted descending over the lanes; lane 63's key drops out
__device__ __forceinline__ uint64_t insert_key(uint64_t kept, uint64_t cand, int lane) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)kept, 1, 64);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(kept >> 32), 1, 64);
  const uint64_t up = ((uint64_t)hi << 32) | lo;
  const bool above = lane == 0 || up > cand;  // the lane above stays where it is
  return kept > cand ? kept : (above ? cand : up);
}

__device__ __forceinline__ void split8(const float* f, v4u& hi, v4u& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t h0 = tcamd::f32_to_bf16_rne(f[2 * e]), h1 = tcamd::f32_to_bf16_rne(f[2 * e + 1]);
    const uint32_t l0 = tcamd::f32_to_bf16_rne(f[2 * e] - __uint_as_float(h0 << 16));
    const uint32_t l1 = tcamd::f32_to_bf16_rne(f[2 * e + 1] - __uint_as_float(h1 << 16));
    hi[e] = h0 | (h1 << 16);
    lo[e] = l0 | (l1 << 16);
  }
}

}  // namespace tcamd_search
