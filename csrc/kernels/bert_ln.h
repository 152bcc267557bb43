// Row LayerNorm pieces shared by the BERT kernels (csrc/kernels/bert.hip K11 /
// embedding LayerNorm, csrc/kernels/bert_pack.hip packed embedding LayerNorm): one wave
// owns one row of H = 64 * E bf16 elements, lane l the 16-B chunks l, l + 64, ...
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace tcamd_bert {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const bf16x2 v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LayerNorm of one row held as v[E] per lane (lane l owns the 16-B chunks
// l, l + 64, ...) -> bf16 out row: exact two-pass mean / variance over the
// register copy, wave butterflies through DPP-backed shuffles
template <int E>
__device__ __forceinline__ void ln_store_row(const float (&v)[E], const uint16_t* __restrict__ gamma,
                                             const uint16_t* __restrict__ beta, uint16_t* orow, int lane, float eps) {
  constexpr int H = 64 * E, C = E / 8;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) s += v[e];
  const float mean = wave_sum(s) * (1.0f / H);
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float d = v[e] - mean;
    ss += d * d;
  }
  const float rstd = rsqrtf(wave_sum(ss) * (1.0f / H) + eps);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int off = (c * 64 + lane) * 8;
    const v4u g = *reinterpret_cast<const v4u*>(gamma + off);
    const v4u bt = *reinterpret_cast<const v4u*>(beta + off);
    v4u o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float g0 = __uint_as_float(g[q] << 16), g1 = __uint_as_float(g[q] & 0xffff0000u);
      const float b0 = __uint_as_float(bt[q] << 16), b1 = __uint_as_float(bt[q] & 0xffff0000u);
      o[q] = pack2((v[c * 8 + 2 * q] - mean) * rstd * g0 + b0, (v[c * 8 + 2 * q + 1] - mean) * rstd * g1 + b1);
    }
    *reinterpret_cast<v4u*>(orow + off) = o;
  }
}

}  // namespace tcamd_bert
