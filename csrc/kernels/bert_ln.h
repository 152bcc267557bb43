// Row LayerNorm pieces shared by the BERT kernels (csrc/kernels/bert.hip K11 /
// embedding LayerNorm, csrc/kernels/bert_pack.hip packed embedding LayerNorm): one wave
// owns one row of H = 64 * E elements, lane l the 8-element chunks l, l + 64, ...
// (16 B of a bf16 row, 32 B of an fp32 one)
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

// The fp32 form (the fp32-parity model): gamma / beta / out fp32, the same
// two-pass statistics.  orow3 (or null): the row also as the next bf16x3
// GEMM's operand, bf16 [3H] = [hi | hi | lo] (x3_cat's layout), bitwise x3_cat
// of the fp32 row: the fence keeps hipcc from contracting o - hi into an fma
// over the unrounded product.
template <int E>
__device__ __forceinline__ void ln_store_row(const float (&v)[E], const float* __restrict__ gamma,
                                             const float* __restrict__ beta, float* orow, uint16_t* orow3, int lane,
                                             float eps) {
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
    float o[8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + off + 4 * hf);
      const float4 bt = *reinterpret_cast<const float4*>(beta + off + 4 * hf);
      o[4 * hf] = (v[c * 8 + 4 * hf] - mean) * rstd * g.x + bt.x;
      o[4 * hf + 1] = (v[c * 8 + 4 * hf + 1] - mean) * rstd * g.y + bt.y;
      o[4 * hf + 2] = (v[c * 8 + 4 * hf + 2] - mean) * rstd * g.z + bt.z;
      o[4 * hf + 3] = (v[c * 8 + 4 * hf + 3] - mean) * rstd * g.w + bt.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(o[e]));
    reinterpret_cast<float4*>(orow + off)[0] = make_float4(o[0], o[1], o[2], o[3]);
    reinterpret_cast<float4*>(orow + off)[1] = make_float4(o[4], o[5], o[6], o[7]);
    if (orow3) {
      v4u hi, lo;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        hi[q] = pack2(o[2 * q], o[2 * q + 1]);
        lo[q] = pack2(o[2 * q] - __uint_as_float(hi[q] << 16), o[2 * q + 1] - __uint_as_float(hi[q] & 0xffff0000u));
      }
      *reinterpret_cast<v4u*>(orow3 + off) = hi;
      *reinterpret_cast<v4u*>(orow3 + H + off) = hi;
      *reinterpret_cast<v4u*>(orow3 + 2 * H + off) = lo;
    }
  }
}

}  // namespace tcamd_bert
