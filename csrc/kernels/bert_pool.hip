// K32 — the last LayerNorm of bert_large fused with sentence pooling (gfx950).
//
//   h[t] = LayerNorm(x[r, t] + y[r, t]) * gamma + beta     (layer 23's second LayerNorm)
//   e[r] = sum over t with mask[r, t] >= 1 of h[t] / count,  or h[0] in CLS mode
//   e[r] /= |e[r]|_2                                        unless the row's flag says no
//
// out fp32 [rows, H].  As torch ops the tail is a LayerNorm, a masked mean
// and a normalize: three launches and three passes over the last hidden state
// ([rows, 384, 1024]: 100 MB at 128 rows in bf16).  The LayerNorm already
// holds every value the pooling needs in registers, so here the last hidden
// state is never written: the operands of the LayerNorm are read once, and
// what leaves is 4 KB per row.
//
// Operand forms, the two that the FFN-down route of the last layer produces
// (models/bert.py _proj_add_ln), each in bf16 and in fp32 (the fp32-parity
// model), summed in the order of K11 / K11p (csrc/kernels/bert.hip):
//   * K11's:  x + y, both in the model dtype;
//   * K11p's: x + bias + parts[0] + ... + parts[nparts - 1], bias and the
//     split-K slabs fp32, slab z at parts + z * pstride.
// The statistics are bert_ln.h's ln_stats (two-pass, fp32 registers, wave
// shuffles), shared with K11 and the embedding LayerNorms.  h stays fp32: it is
// not rounded to the model dtype on its way into the sum.
//
// Two launches, both graph-capturable, no atomics, no workgroup waits for
// another:
//   pool_partial  grid P x rows, P = ceil(S / 48) token slices (8 at S = 384:
//     a one-row request still spreads over 8 workgroups).  A workgroup is 4
//     waves; wave w takes the tokens 48 p + w, + 4, ... of its slice, one at
//     a time.  A lane holds 16 columns of H = 1024 as bert_ln.h lays a row
//     out (the 8-column chunks l and l + 64: every load is 16 B and a wave
//     instruction covers whole cache lines).  A token whose mask is below 1 is skipped
//     before any of its bytes are loaded; in CLS mode only slice 0 / wave 0 /
//     token 0 does work, whatever the mask says.  The wave normalises its
//     token in registers and adds it into 16 fp32 accumulators per lane, in
//     ascending t.  The 4 waves' accumulators meet in LDS (16 KB) and thread
//     i sums columns i, i + 256, ... as ((w0 + w1) + w2) + w3.  The slice's
//     partial sum and its token count go to the workspace
//     [rows, P, H + 1] fp32 (count in the last slot), zeros included.
//   pool_finish   one workgroup per row: sums the P partials in ascending
//     slice order, divides by the count, reduces the squared norm by wave
//     shuffles and then over the 4 waves through LDS in wave order, scales and
//     stores the row.
//
// Batch invariance (the property K10c, csrc/kernels/densenet_head.hip,
// established for the DenseNet head): the embedding of a row is the same bits
// at rows = 1 and rows = 128 and at any position of the batch.  The reason:
// no value of another row enters a row's arithmetic, and the decomposition --
// which wave takes which token, the order a wave adds its tokens, the order
// of the LDS sum, the order of the slice sum, the order of the norm
// reduction -- is a function of S alone; rows only picks blockIdx.y.  One
// kernel serves every batch size, so there is no other code path to agree with.
//
// Edge rules (the torch fallback in models/bert.py follows the same ones):
//   * a row with no valid token gives all zeros (count 0 divides nothing);
//   * a row whose norm is 0 is left unscaled;
//   * flags[r] bit 0 selects CLS pooling, bit 1 skips the L2 normalisation, so
//     requests with different settings share a launch (as K27's k_row /
//     len_row do); flags null = all zero;
//   * mask int32 [rows, S] at a row stride, or null = every token valid;
//   * H = 1024 only, S in 1 .. 512: anything else is hipErrorInvalidValue and no launch.
//
// Reference analog: none (the reference client runs no model).

#include <cstddef>
#include <cstdint>

#include "kernels/bert_ln.h"

namespace {

using tcamd_bert::ln_stats;
using tcamd_bert::v4u;

constexpr int kH = 1024;    // hidden size: 64 lanes x 16 columns
constexpr int kE = 16;      // columns per lane
constexpr int kSlice = 48;  // tokens per workgroup of pool_partial
constexpr int kWaves = 4;
constexpr int kMaxS = 512;
constexpr int kCls = 1, kRaw = 2;  // flag bits

// v[8] (+)= 8 columns at p
__device__ __forceinline__ void load8(const uint16_t* p, float* v) {
  const v4u a = *reinterpret_cast<const v4u*>(p);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[2 * q] = __uint_as_float(a[q] << 16);
    v[2 * q + 1] = __uint_as_float(a[q] & 0xffff0000u);
  }
}
__device__ __forceinline__ void load8(const float* p, float* v) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
template <typename T>
__device__ __forceinline__ void add8(const T* p, float* v) {
  float a[8];
  load8(p, a);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] += a[e];
}

// What the LayerNorm sums: K11's form (PARTS = false: y in the model dtype,
// bias / nparts / pstride unused) or K11p's (y = the fp32 slabs).
template <typename T, bool PARTS>
struct Operands {
  const T* x;
  const void* y;
  const float* bias;
  int nparts;
  long long pstride;
};

template <typename T, bool PARTS>
__global__ void __launch_bounds__(64 * kWaves) pool_partial_kernel(Operands<T, PARTS> op, const T* __restrict__ gamma,
                                                                   const T* __restrict__ beta,
                                                                   const int* __restrict__ mask, long long mask_stride,
                                                                   const int* __restrict__ flags,
                                                                   float* __restrict__ ws, int S, int P, float eps) {
  __shared__ __attribute__((aligned(16))) float acc_s[kWaves][kH];
  __shared__ int cnt_s[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x, r = blockIdx.y;
  const bool cls = flags && (flags[r] & kCls);
  const int t0 = p * kSlice, t1 = min(t0 + kSlice, S);
  const int* mrow = mask ? mask + (size_t)r * mask_stride : nullptr;

  float g[kE], bt[kE], acc[kE];
#pragma unroll
  for (int c = 0; c < kE / 8; ++c) {
    load8(gamma + (c * 64 + lane) * 8, g + 8 * c);
    load8(beta + (c * 64 + lane) * 8, bt + 8 * c);
  }
#pragma unroll
  for (int e = 0; e < kE; ++e) acc[e] = 0.f;
  int cnt = 0;

  for (int t = t0 + wave; t < t1; t += kWaves) {
    // wave-uniform: the whole wave skips the token before touching its bytes
    if (cls ? t != 0 : (mrow && mrow[t] < 1)) continue;
    const size_t base = ((size_t)r * S + t) * kH;
    float v[kE];
#pragma unroll
    for (int c = 0; c < kE / 8; ++c) load8(op.x + base + (c * 64 + lane) * 8, v + 8 * c);
    if constexpr (PARTS) {
      if (op.bias)
#pragma unroll
        for (int c = 0; c < kE / 8; ++c) add8(op.bias + (c * 64 + lane) * 8, v + 8 * c);
      for (int z = 0; z < op.nparts; ++z) {
        const float* pz = static_cast<const float*>(op.y) + z * op.pstride + base;
#pragma unroll
        for (int c = 0; c < kE / 8; ++c) add8(pz + (c * 64 + lane) * 8, v + 8 * c);
      }
    } else {
#pragma unroll
      for (int c = 0; c < kE / 8; ++c) add8(static_cast<const T*>(op.y) + base + (c * 64 + lane) * 8, v + 8 * c);
    }
    float mean, rstd;
    ln_stats<kE>(v, eps, mean, rstd);
#pragma unroll
    for (int e = 0; e < kE; ++e) acc[e] += (v[e] - mean) * rstd * g[e] + bt[e];
    ++cnt;
  }

#pragma unroll
  for (int c = 0; c < kE / 8; ++c) {
    float4* d = reinterpret_cast<float4*>(&acc_s[wave][(c * 64 + lane) * 8]);
    d[0] = make_float4(acc[8 * c], acc[8 * c + 1], acc[8 * c + 2], acc[8 * c + 3]);
    d[1] = make_float4(acc[8 * c + 4], acc[8 * c + 5], acc[8 * c + 6], acc[8 * c + 7]);
  }
  if (lane == 0) cnt_s[wave] = cnt;
  __syncthreads();
  float* o = ws + ((size_t)r * P + p) * (kH + 1);
  for (int i = threadIdx.x; i < kH; i += 64 * kWaves)
    o[i] = ((acc_s[0][i] + acc_s[1][i]) + acc_s[2][i]) + acc_s[3][i];
  if (threadIdx.x == 0) o[kH] = (float)(cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3]);
}

__global__ void __launch_bounds__(64 * kWaves) pool_finish_kernel(const float* __restrict__ ws,
                                                                  const int* __restrict__ flags,
                                                                  float* __restrict__ out, int P) {
  __shared__ float sq_s[kWaves];
  const int r = blockIdx.x;
  const float* w = ws + (size_t)r * P * (kH + 1);
  constexpr int kPer = kH / (64 * kWaves);  // columns per thread: i, i + 256, ...
  float e[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) e[k] = 0.f;
  float count = 0.f;
  for (int p = 0; p < P; ++p) {
    const float* wp = w + (size_t)p * (kH + 1);
#pragma unroll
    for (int k = 0; k < kPer; ++k) e[k] += wp[threadIdx.x + k * 64 * kWaves];
    count += wp[kH];
  }
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    e[k] = count > 0.f ? e[k] / count : 0.f;
    sq += e[k] * e[k];
  }
  sq = tcamd_bert::wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sq_s[threadIdx.x >> 6] = sq;
  __syncthreads();
  const float norm = sqrtf(((sq_s[0] + sq_s[1]) + sq_s[2]) + sq_s[3]);
  const bool scale = !(flags && (flags[r] & kRaw)) && norm > 0.f;
#pragma unroll
  for (int k = 0; k < kPer; ++k)
    out[(size_t)r * kH + threadIdx.x + k * 64 * kWaves] = scale ? e[k] / norm : e[k];
}

template <typename T, bool PARTS>
int launch(const void* x, const void* y, int nparts, long long pstride, const float* bias, const void* gamma,
           const void* beta, const int* mask, long long mask_stride, const int* flags, void* workspace, float* out,
           int rows, int S, float eps, hipStream_t s) {
  const int P = (S + kSlice - 1) / kSlice;
  const Operands<T, PARTS> op{static_cast<const T*>(x), y, bias, nparts, pstride};
  hipLaunchKernelGGL((pool_partial_kernel<T, PARTS>), dim3(P, rows), dim3(64 * kWaves), 0, s, op,
                     static_cast<const T*>(gamma), static_cast<const T*>(beta), mask, mask_stride, flags,
                     static_cast<float*>(workspace), S, P, eps);
  hipLaunchKernelGGL(pool_finish_kernel, dim3(rows), dim3(64 * kWaves), 0, s, static_cast<const float*>(workspace),
                     flags, out, P);
  return hipGetLastError();
}

bool bad_common(const void* x, const void* gamma, const void* beta, const int* mask, long long mask_stride,
                const void* workspace, const float* out, int rows, int S, int H) {
  return !x || !gamma || !beta || !workspace || !out || H != kH || S < 1 || S > kMaxS || rows > 65535 ||
         (mask && mask_stride < S) ||
         ((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)workspace | (uintptr_t)out) % 16;
}

}  // namespace

extern "C" {

// Bytes of workspace K32 needs for rows x S tokens: [rows, ceil(S / 48), H + 1] fp32
// (0 for a shape the kernel refuses)
size_t tcamd_pool_layernorm_workspace(int rows, int S) {
  if (rows <= 0 || S < 1 || S > kMaxS) return 0;
  return (size_t)rows * ((S + kSlice - 1) / kSlice) * (kH + 1) * sizeof(float);
}

// K32, K11's operand form: out fp32 [rows][H] = pooled LayerNorm(x + y) * gamma
// + beta over x, y [rows][S][H] (see the file header).  f32 = 0: x / y / gamma
// / beta bf16, 1: fp32.  mask int32 [rows][S] at mask_stride elements per row,
// or null; flags int32 [rows] or null.  H = 1024, 1 <= S <= 512; 16-B aligned
// x, y, gamma, beta, workspace, out.
int tcamd_pool_layernorm(const void* x, const void* y, const void* gamma, const void* beta, const int* mask,
                         long long mask_stride, const int* flags, void* workspace, float* out, int rows, int S, int H,
                         float eps, int f32, void* stream) {
  if (rows <= 0) return hipSuccess;
  if (bad_common(x, gamma, beta, mask, mask_stride, workspace, out, rows, S, H) || !y || (uintptr_t)y % 16)
    return hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  return f32 ? launch<float, false>(x, y, 0, 0, nullptr, gamma, beta, mask, mask_stride, flags, workspace, out, rows,
                                    S, eps, s)
             : launch<uint16_t, false>(x, y, 0, 0, nullptr, gamma, beta, mask, mask_stride, flags, workspace, out,
                                       rows, S, eps, s);
}

// K32, K11p's operand form: the LayerNorm's input is x + bias + the sum of
// nparts fp32 slabs (parts + z * pstride elements, [rows][S][H] each); bias
// fp32 [H] or null.  Everything else as tcamd_pool_layernorm.
int tcamd_pool_layernorm_parts(const void* x, const float* parts, int nparts, long long pstride, const float* bias,
                               const void* gamma, const void* beta, const int* mask, long long mask_stride,
                               const int* flags, void* workspace, float* out, int rows, int S, int H, float eps,
                               int f32, void* stream) {
  if (rows <= 0) return hipSuccess;
  if (bad_common(x, gamma, beta, mask, mask_stride, workspace, out, rows, S, H) || nparts < 0 ||
      (nparts > 0 && (!parts || pstride < (long long)rows * S * H || pstride % 4)) ||
      ((uintptr_t)parts | (uintptr_t)bias) % 16)
    return hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  return f32 ? launch<float, true>(x, parts, nparts, pstride, bias, gamma, beta, mask, mask_stride, flags, workspace,
                                   out, rows, S, eps, s)
             : launch<uint16_t, true>(x, parts, nparts, pstride, bias, gamma, beta, mask, mask_stride, flags,
                                      workspace, out, rows, S, eps, s);
}

}  // extern "C"
