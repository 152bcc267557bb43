// K11 — fused residual add + LayerNorm for the bert_large serving model (gfx950).
//
// BERT's post-LN block ends every sub-layer with LN(x + f(x)).  As two torch
// ops that is an add pass (read 2, write 1) plus a LayerNorm pass (read 1,
// write 1) over [tokens, 1024] bf16: 5 x 50 MB at bs64 x seq384, 48 times per
// forward (rocprofv3 on MI355X: add 24 us + LN 40 us per call, 23% of the
// forward with GELU).  Here one wave owns one row: each lane loads its 16
// elements of x and y (two 16-B loads each), the sum stays in registers, mean
// and variance are exact two-pass reductions over the register copy (wave
// butterfly through DPP-backed shuffles), and the normalised row leaves as
// bf16 — 3 passes over the data instead of 5, one launch instead of two.
// Reference analog: none (the reference client runs no model; this serves the
// `bert_large` perf_analyzer config of BASELINE.json).

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "kernels/bert_ln.h"
#include "kernels/common.h"

namespace {

using tcamd_bert::v4u;
using tcamd_bert::pack2;
using tcamd_bert::wave_sum;
using tcamd_bert::ln_store_row;

// E = elements per lane (H = 64 * E), a multiple of 8.  Lane l owns the 16-B
// chunks l, l + 64, ... of the row (coalesced: a wave instruction covers 1 KB).
template <int E>
__global__ void __launch_bounds__(256) add_layernorm_kernel(const uint16_t* x, const uint16_t* y,  // out may alias
                                                            const uint16_t* __restrict__ gamma,
                                                            const uint16_t* __restrict__ beta, uint16_t* out,
                                                            int rows, float eps) {
  constexpr int H = 64 * E, C = E / 8;  // 16-B chunks per lane
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const size_t base = (size_t)row * H;
  float v[E];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int off = (c * 64 + lane) * 8;
    const v4u a = *reinterpret_cast<const v4u*>(x + base + off);
    const v4u b = *reinterpret_cast<const v4u*>(y + base + off);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[c * 8 + 2 * q] = __uint_as_float(a[q] << 16) + __uint_as_float(b[q] << 16);
      v[c * 8 + 2 * q + 1] = __uint_as_float(a[q] & 0xffff0000u) + __uint_as_float(b[q] & 0xffff0000u);
    }
  }
  ln_store_row<E>(v, gamma, beta, out + base, lane, eps);
}

// ---- K11p: LN(x + bias + sum_z parts[z]) -----------------------------------
// The consumer of a split-K projection (K18, csrc/kernels/gemm_tiles.hip):
// the attention-out / FFN-down GEMM leaves fp32 partial slabs instead of a
// bf16 y, and this pass -- which BERT needs anyway for the residual add +
// LayerNorm -- sums them with the bias on the way in, so the split costs no
// reduce launch and y never exists as its own tensor.  T = uint16_t (bf16
// x / gamma / beta / out: the bf16 model) or float (the fp32-parity model).
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
__device__ __forceinline__ void add8(const float* p, float* v) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] += a.x, v[1] += a.y, v[2] += a.z, v[3] += a.w, v[4] += b.x, v[5] += b.y, v[6] += b.z, v[7] += b.w;
}
__device__ __forceinline__ void store8(uint16_t* p, const float* v) {
  *reinterpret_cast<v4u*>(p) = v4u{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// out3 (fp32 model, or null): the row also as the next bf16x3 GEMM's operand,
// bf16 [rows][3H] = [hi | hi | lo] (x3_cat's layout), so that GEMM needs no
// x3_cat pass over the LayerNorm output.
template <int E, typename T>
__global__ void __launch_bounds__(256) add_ln_parts_kernel(const T* x, const float* parts, int nparts, long long pstride,
                                                           const float* __restrict__ bias, const T* __restrict__ gamma,
                                                           const T* __restrict__ beta, T* out, uint16_t* __restrict__ out3,
                                                           int rows, float eps) {
  constexpr int H = 64 * E, C = E / 8;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const size_t base = (size_t)row * H;
  float v[E];
#pragma unroll
  for (int c = 0; c < C; ++c) load8(x + base + (c * 64 + lane) * 8, v + 8 * c);
  if (bias)
#pragma unroll
    for (int c = 0; c < C; ++c) add8(bias + (c * 64 + lane) * 8, v + 8 * c);
  for (int zz = 0; zz < nparts; ++zz) {
    const float* pz = parts + zz * pstride + base;
#pragma unroll
    for (int c = 0; c < C; ++c) add8(pz + (c * 64 + lane) * 8, v + 8 * c);
  }
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
    float g[8], bt[8], o[8];
    load8(gamma + off, g);
    load8(beta + off, bt);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (v[8 * c + e] - mean) * rstd * g[e] + bt[e];
    store8(out + base + off, o);
    if (out3) {
      v4u hi, lo;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        hi[q] = pack2(o[2 * q], o[2 * q + 1]);
        lo[q] = pack2(o[2 * q] - __uint_as_float(hi[q] << 16), o[2 * q + 1] - __uint_as_float(hi[q] & 0xffff0000u));
      }
      uint16_t* r3 = out3 + 3 * base + off;
      *reinterpret_cast<v4u*>(r3) = hi;
      *reinterpret_cast<v4u*>(r3 + H) = hi;
      *reinterpret_cast<v4u*>(r3 + 2 * H) = lo;
    }
  }
}

// ---- QA head: (start, end)[r] = x[r] . w[0 / 1] + b[0 / 1] -----------------
// BERT's span head is a [2 x H] Linear over every token: as a library GEMM an
// N = 2 launch plus a cast and two strided copies.  One wave per row: each
// lane dots its 8-element chunks with both weight rows, a butterfly sums the
// wave, lane 0 writes the two fp32 logits into their separate [rows] planes.
template <int E, typename T>
__global__ void __launch_bounds__(256) qa_head_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ start,
                                                      float* __restrict__ end, int rows) {
  constexpr int H = 64 * E, C = E / 8;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int off = (c * 64 + lane) * 8;
    float xv[8], w0[8], w1[8];
    load8(x + (size_t)row * H + off, xv);
    load8(w + off, w0);
    load8(w + H + off, w1);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s0 += xv[e] * w0[e];
      s1 += xv[e] * w1[e];
    }
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (lane == 0) {
    start[row] = s0 + b[0];
    end[row] = s1 + b[1];
  }
}

// Embedding sum + LayerNorm: out[r] = LN(word[ids[r]] + pos[r % S] +
// type[types[r]]) in one pass (torch: three gathers, two adds and a LayerNorm,
// six launches and ~5 passes over [tokens, H]).  Ids outside the tables are
// clamped (torch would raise).
template <int E>
__global__ void __launch_bounds__(256) embed_layernorm_kernel(const int64_t* __restrict__ ids,
                                                              const int64_t* __restrict__ types,
                                                              const uint16_t* __restrict__ word,
                                                              const uint16_t* __restrict__ pos,
                                                              const uint16_t* __restrict__ tok,
                                                              const uint16_t* __restrict__ gamma,
                                                              const uint16_t* __restrict__ beta, uint16_t* __restrict__ out,
                                                              int rows, int S, int vocab, int ntypes, float eps) {
  constexpr int H = 64 * E, C = E / 8;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long long id = min(max(ids[row], (int64_t)0), (int64_t)vocab - 1);
  const long long ty = min(max(types[row], (int64_t)0), (int64_t)ntypes - 1);
  const uint16_t* rw = word + (size_t)id * H;
  const uint16_t* rp = pos + (size_t)(row % S) * H;
  const uint16_t* rt = tok + (size_t)ty * H;
  float v[E];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int off = (c * 64 + lane) * 8;
    const v4u a = *reinterpret_cast<const v4u*>(rw + off);
    const v4u b = *reinterpret_cast<const v4u*>(rp + off);
    const v4u t = *reinterpret_cast<const v4u*>(rt + off);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[c * 8 + 2 * q] = __uint_as_float(a[q] << 16) + __uint_as_float(b[q] << 16) + __uint_as_float(t[q] << 16);
      v[c * 8 + 2 * q + 1] = __uint_as_float(a[q] & 0xffff0000u) + __uint_as_float(b[q] & 0xffff0000u) +
                             __uint_as_float(t[q] & 0xffff0000u);
    }
  }
  ln_store_row<E>(v, gamma, beta, out + (size_t)row * H, lane, eps);
}

}  // namespace


namespace {
// ============================================================================
// K12 — fused multi-head attention for bert_large (non-causal, head dim 64,
// additive key-padding mask), straight from the fused QKV GEMM's output.
// ============================================================================
// torch-ROCm's SDPA with a key-padding bias costs 216 us per layer at bs64 x
// seq384 (120 us unmasked) plus a transpose copy of its output; here one block
// owns one (sequence, head):
//   * K [S][64] and V^T [64][S] (bf16) of the head go to LDS once (96 KB at
//     S = 384): K rows 128 B with 16-B chunks XOR-swizzled by (row >> 1) & 7
//     (conflict-free b128 reads by 16 consecutive keys), V transposed while it
//     is staged (pairs of keys -> 32-bit writes), rows padded to S + 4 so the
//     dim-major b64 reads of 32 lanes hit 32 distinct bank pairs;
//   * wave w owns queries [32w, 32w + 32) (S/32 waves, 3 per SIMD at S = 384):
//     its Q^T fragments stay in registers; per 64-key chunk S^T = K Q^T on
//     v_mfma_f32_32x32x16_bf16 (8 MFMAs), an online softmax in the exp2
//     domain (per-lane partial row sums, one cross-half max shuffle per
//     chunk), then O^T += V^T P^T (8 MFMAs) with P^T taken straight from the
//     S^T accumulators: the MFMA k index is permuted so a lane's 8 keys are
//     exactly the 8 scores it already holds, and V^T is read in that order;
//   * exponentials are raw v_exp_f32 (flushed denormals are exactly what a
//     softmax wants; exp2f adds a range fix-up of ~4 VALU per score);
//   * O / l leaves as bf16 in [tokens][heads * 64] — the layout the output
//     projection GEMM reads, so no transpose kernel follows.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef short v4s __attribute__((ext_vector_type(4)));

constexpr int kAD = 64;           // head dim
constexpr int kAMaxS = 384;       // keys / queries per sequence (multiple of 64)

__device__ __forceinline__ bf16x8 as_bf8(v4u v) { return __builtin_bit_cast(bf16x8, v); }

// qkv_bias (may be null): the QKV projection's bias [3 * heads * 64], applied
// here so the projection runs as a plain GEMM (hipBLASLt's bias epilogue cost
// ~20 us per layer at bs64 x 384): q + b_q feeds the scores; the key bias
// adds (q + b_q) . b_k to every score of a query, a constant that softmax
// removes, so it is dropped; the value bias passes through the normalised
// weights unchanged and is added to the output.
//
// The device code is a function of a row geometry, shared by K12 and K12v
// (packed rows, below): the row's first token, the number of keys it stages
// ``S`` (a multiple of 64: LDS rows and chunk count) and its length ``len``.
// It lives in kernels/bert_attention_row.h, which says why it is a text and
// not a function, and why its one barrier is workgroup-uniform.  K12 gives it
// (seq * S, S, S) and PACKED = false, which folds every use of ``len`` away;
// K12v (cu[r], 64 * ceil(len / 64), len).
template <bool MASKED>
__global__ void __launch_bounds__(768, 1) attention_kernel(const uint16_t* __restrict__ qkv, const int* __restrict__ mask,
                                                           uint16_t* __restrict__ out, int S, int heads, float scale,
                                                           const uint16_t* __restrict__ qkv_bias) {
  constexpr bool PACKED = false;
#define TC_ATTN_ROW_GEOMETRY const int seq = blockIdx.x / heads, head = blockIdx.x % heads, len = S;
#define TC_ATTN_ROW_TOK0 ((size_t)seq * S)
#include "kernels/bert_attention_row.h"
#undef TC_ATTN_ROW_GEOMETRY
#undef TC_ATTN_ROW_TOK0
}

// ---- K12v: K12 over packed rows -------------------------------------------
// qkv [t_cap][3 * heads * 64] holds the tokens of rows of different lengths
// back to back (K30 bert_pack_plan, csrc/kernels/bert_pack.hip): block (row r,
// head) attends the queries and keys cu[r] .. cu[r] + row_len[r] - 1 and
// touches no other token, so rows [T, t_cap) of qkv are never read and those
// of out never written.  It stages 64 * ceil(len / 64) keys, the ones at or
// past len as copies of the row's last token under the -10000 bias.  The grid
// is fixed per (rows, heads) -- K12's plan at S = 384 -- so a HIP graph can
// capture it; an empty row's blocks, a block whose query split starts past
// the row's end, and a row that does not fit t_cap (a caller's error) return
// at once, on conditions uniform over the block.
__global__ void __launch_bounds__(768, 1) attention_packed_kernel(const uint16_t* __restrict__ qkv,
                                                                  const int* __restrict__ row_len,
                                                                  const int* __restrict__ cu,
                                                                  uint16_t* __restrict__ out, int t_cap, int heads,
                                                                  float scale, const uint16_t* __restrict__ qkv_bias) {
  constexpr bool MASKED = true, PACKED = true;
  const int row = blockIdx.x / heads, first = cu[row];
  {
    const int len = row_len[row];
    if (len <= 0 || len > kAMaxS || first < 0 || first > t_cap - len) return;
    if (32 * (int)(blockIdx.y * (blockDim.x >> 6)) >= len) return;
  }
  const int* const mask = nullptr;                     // a key's validity is k < len
  const int S = 64 * ((row_len[row] + 63) >> 6);       // keys staged
#define TC_ATTN_ROW_GEOMETRY const int head = blockIdx.x % heads, len = row_len[row];
#define TC_ATTN_ROW_TOK0 ((size_t)first)
#include "kernels/bert_attention_row.h"
#undef TC_ATTN_ROW_GEOMETRY
#undef TC_ATTN_ROW_TOK0
}

// bf16x3 operand of the fp32-parity bert mode: x fp32 [rows][K] -> out bf16
// [rows][3K] = [hi | hi | lo] (hi = bf16_rne(x), lo = bf16_rne(x - hi)), so
// ONE bf16 GEMM against W' = [W_hi | W_lo | W_hi] (K' = 3K) accumulates
// x_hi W_hi + x_hi W_lo + x_lo W_hi in fp32: ~1e-5 of an fp32 GEMM at 3x the
// bf16 MFMA work (gfx950 has no xf32, and its f32-input MFMA runs at 1/16 of
// the bf16 rate).  One thread per 4 elements: a 16-B load, three 8-B stores.
__global__ void __launch_bounds__(256) x3_cat_kernel(const float* __restrict__ x, uint16_t* __restrict__ out,
                                                     long n4, int k4) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long r = i / k4, c = i - r * k4;
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const uint32_t h0 = pack2(v.x, v.y), h1 = pack2(v.z, v.w);
    const uint32_t l0 = pack2(v.x - __uint_as_float(h0 << 16), v.y - __uint_as_float(h0 & 0xffff0000u));
    const uint32_t l1 = pack2(v.z - __uint_as_float(h1 << 16), v.w - __uint_as_float(h1 & 0xffff0000u));
    uint2* row = reinterpret_cast<uint2*>(out) + r * 3 * k4;  // 3 segments of k4 x 8 B
    row[c] = make_uint2(h0, h1);
    row[k4 + c] = make_uint2(h0, h1);
    row[2 * k4 + c] = make_uint2(l0, l1);
  }
}


// ---- K12x: fp32-parity attention (bf16x3 products, fp32 softmax) -----------
// The fp32-parity bert's attention (it ran torch SDPA in fp32, 25 % of that
// forward).  Block = (sequence, head, 16 NW queries), NW waves x 16 queries; keys
// in 64-key chunks staged into LDS split hi / lo (K row-major, V transposed);
// every product is bf16x3 (hi*hi + hi*lo + lo*hi, fp32 accumulate), the
// online softmax is fp32 with exp; masked keys get the reference's additive
// -10000 (so a fully masked row averages like torch's).
//   S^T = K Q^T on 16x16x32 MFMAs: lane (l & 15) = query, reg e -> key 4g + e
//   (g = l >> 4), so the softmax state of a query is lane-local after two
//   xor-shuffles over the lane groups, and the same registers are the B
//   operand of O^T = V^T P^T: k position 8g + i <-> key 4g + i of the chunk's
//   16-key tile 2ks (i < 4) or 2ks + 1 (i >= 4), read from V^T in LDS as two
//   8-B runs.  O^T's C layout: lane = query, reg e -> head dim 16 dt + 4g + e.
constexpr int kXR = 64 * 2 + 16;  // LDS row: 64 bf16 + 16 B (16 rows' b128 reads spread over all banks)
constexpr int kBufAX = 4 * 64 * kXR + 64 * 4;  // one chunk: K hi | K lo | V^T hi | V^T lo | key bias
constexpr int kLdsAX = 2 * kBufAX;             // double-buffered: chunk c + 1 is staged during chunk c

__device__ __forceinline__ void split_pk(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack2(a, b);
  lo = pack2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

__device__ __forceinline__ f32x4 mma_x3(v4u ah, v4u al, v4u bh, v4u bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf8(al), as_bf8(bh), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf8(ah), as_bf8(bl), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf8(ah), as_bf8(bh), c, 0, 0, 0);
}

// out3 (or null): write the output as the out-projection's bf16x3 operand,
// bf16 [tokens][3H] = [hi | hi | lo], instead of fp32 into out.
//
// The device code is a function of a row geometry, shared by K12x and K12xv
// (packed rows, below), and lives in kernels/bert_attention_x3_row.h, which
// says why it is a text and not a function, and why its barriers are
// workgroup-uniform.  K12x gives it (seq * S, S / 64 chunks) and PACKED =
// false, which folds every use of ``len`` away; K12xv (cu[r], ceil(len / 64)).
template <int NW>
__global__ void __launch_bounds__(64 * NW) attention_x3_kernel(const float* __restrict__ qkv,
                                                               const int* __restrict__ mask, float* __restrict__ out,
                                                               uint16_t* __restrict__ out3, int S, int heads,
                                                               float scale) {
  constexpr bool PACKED = false;
#define TC_ATTN_X3_GEOMETRY const int seq = blockIdx.x / heads, h = blockIdx.x - seq * heads, len = S;
#define TC_ATTN_X3_TOK0 ((size_t)seq * S)
#include "kernels/bert_attention_x3_row.h"
#undef TC_ATTN_X3_GEOMETRY
#undef TC_ATTN_X3_TOK0
}

// ---- K12xv: K12x over packed rows -------------------------------------------
// qkv fp32 [t_cap][3 * heads * 64] holds the tokens of rows of different
// lengths back to back (K30 bert_pack_plan): block (row r, head, query block of
// 16 NW) attends queries and keys cu[r] .. cu[r] + row_len[r] - 1 and touches
// no other token, so rows [T, t_cap) of qkv are never read and those of out
// never written.  It runs ceil(len / 64) chunks, the keys at or past len
// staged as copies of the row's last token under the -10000 bias: the chunks
// K12x runs on the same row padded to 384 behind a prefix mask, minus the
// trailing all-masked ones, which change nothing (corr = exp(0) = 1, p =
// exp(-10000 - m) = 0), so the valid tokens get K12x's bits.  The grid is
// fixed per (rows, heads) -- K12x's plan at S = 384 -- so a HIP graph can
// capture it; an empty row's blocks, a row longer than 384 or one that does
// not fit t_cap (a caller's error) and a query block starting at or past the
// row's end return at once, on conditions uniform over the block.  A block
// that stays keeps all its waves to the end: K12x stages every chunk
// cooperatively, so each wave reaches each __syncthreads of the chunk loop
// (kernels/bert_attention_x3_row.h says how waves without a query behave).
template <int NW>
__global__ void __launch_bounds__(64 * NW) attention_x3_packed_kernel(const float* __restrict__ qkv,
                                                                      const int* __restrict__ row_len,
                                                                      const int* __restrict__ cu,
                                                                      float* __restrict__ out,
                                                                      uint16_t* __restrict__ out3, int t_cap, int heads,
                                                                      float scale) {
  constexpr bool PACKED = true;
  constexpr int S = kAMaxS;          // K12x's name; the packed text reads len instead
  const int* const mask = nullptr;   // a key's validity is k < len
  const int row = blockIdx.x / heads, first = cu[row];
  {
    const int len = row_len[row];
    if (len <= 0 || len > kAMaxS || first < 0 || first > t_cap - len) return;
    if ((int)(blockIdx.y * (16 * NW)) >= len) return;
  }
#define TC_ATTN_X3_GEOMETRY const int seq = row, h = blockIdx.x - seq * heads, len = row_len[row];
#define TC_ATTN_X3_TOK0 ((size_t)first)
#include "kernels/bert_attention_x3_row.h"
#undef TC_ATTN_X3_GEOMETRY
#undef TC_ATTN_X3_TOK0
}

}  // namespace

extern "C" {

// fp32-parity bert: out bf16 [rows][3K] = [hi | hi | lo] of x fp32 [rows][K]
// (K % 4 == 0, 16-B aligned x, 8-B aligned out)
int tcamd_x3_cat(const float* x, void* out, int rows, int K, void* stream) {
  if (rows <= 0) return hipSuccess;
  if (!x || !out || K <= 0 || K % 4 || (uintptr_t)x % 16 || (uintptr_t)out % 8) return hipErrorInvalidValue;
  const long n4 = (long)rows * (K / 4);
  const int grid = (int)std::min<long>((n4 + 255) / 256, 256L * 16);
  hipLaunchKernelGGL(x3_cat_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)out, n4, K / 4);
  return hipGetLastError();
}

// out = LayerNorm(x + y) * gamma + beta over rows of H bf16 elements
// (H in {512, 1024, 2048, 4096}); x, y, out, gamma, beta 16-B aligned; out may alias x or y.
int tcamd_add_layernorm(const void* x, const void* y, const void* gamma, const void* beta, void* out, int rows, int H,
                        float eps, void* stream) {
  if (rows <= 0) return hipSuccess;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) % 16)
    return hipErrorInvalidValue;
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
  const auto* px = (const uint16_t*)x;
  const auto* py = (const uint16_t*)y;
  const auto* pg = (const uint16_t*)gamma;
  const auto* pb = (const uint16_t*)beta;
  auto* po = (uint16_t*)out;
  switch (H) {
    case 512: hipLaunchKernelGGL(add_layernorm_kernel<8>, grid, block, 0, s, px, py, pg, pb, po, rows, eps); break;
    case 1024: hipLaunchKernelGGL(add_layernorm_kernel<16>, grid, block, 0, s, px, py, pg, pb, po, rows, eps); break;
    case 2048: hipLaunchKernelGGL(add_layernorm_kernel<32>, grid, block, 0, s, px, py, pg, pb, po, rows, eps); break;
    case 4096: hipLaunchKernelGGL(add_layernorm_kernel<64>, grid, block, 0, s, px, py, pg, pb, po, rows, eps); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// K11p: out = LayerNorm(x + bias + sum_{z < nparts} parts[z]) * gamma + beta
// over rows of H elements (H in {512, 1024, 2048, 4096}); parts fp32, slab z
// at parts + z * pstride (elements, [rows][H] each); bias fp32 [H] or null;
// f32 = 0: x / gamma / beta / out bf16, 1: fp32.  16-B aligned pointers;
// out may alias x.
int tcamd_add_layernorm_parts3(const void* x, const float* parts, int nparts, long long pstride, const float* bias,
                               const void* gamma, const void* beta, void* out, void* out3, int rows, int H, float eps,
                               int f32, void* stream) {
  if (rows <= 0) return hipSuccess;
  if (nparts < 0 || (nparts > 0 && (!parts || pstride < (long long)rows * H)) || (out3 && !f32) ||
      ((uintptr_t)x | (uintptr_t)parts | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out |
       (uintptr_t)out3) % 16)
    return hipErrorInvalidValue;
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
#define TC_K11P(E, T)                                                                                            \
  hipLaunchKernelGGL((add_ln_parts_kernel<E, T>), grid, block, 0, s, (const T*)x, parts, nparts, pstride, bias, \
                     (const T*)gamma, (const T*)beta, (T*)out, (uint16_t*)out3, rows, eps)
  switch (H * 2 + (f32 ? 1 : 0)) {
    case 1024: TC_K11P(8, uint16_t); break;
    case 1025: TC_K11P(8, float); break;
    case 2048: TC_K11P(16, uint16_t); break;
    case 2049: TC_K11P(16, float); break;
    case 4096: TC_K11P(32, uint16_t); break;
    case 4097: TC_K11P(32, float); break;
    case 8192: TC_K11P(64, uint16_t); break;
    case 8193: TC_K11P(64, float); break;
    default: return hipErrorInvalidValue;
  }
#undef TC_K11P
  return hipGetLastError();
}

int tcamd_add_layernorm_parts(const void* x, const float* parts, int nparts, long long pstride, const float* bias,
                              const void* gamma, const void* beta, void* out, int rows, int H, float eps, int f32,
                              void* stream) {
  return tcamd_add_layernorm_parts3(x, parts, nparts, pstride, bias, gamma, beta, out, nullptr, rows, H, eps, f32,
                                    stream);
}

// QA head: start[r] = x[r] . w[0] + b[0], end[r] = x[r] . w[1] + b[1] (fp32
// out) over rows of H (512 / 1024 / 2048 / 4096) elements; x / w bf16 (f32 =
// 0) or fp32, b fp32 [2]; 16-B aligned x / w.
int tcamd_qa_head(const void* x, const void* w, const float* b, float* start, float* end, int rows, int H, int f32,
                  void* stream) {
  if (rows <= 0) return hipSuccess;
  if (!x || !w || !b || !start || !end || ((uintptr_t)x | (uintptr_t)w) % 16) return hipErrorInvalidValue;
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
#define TC_QA(E, T) \
  hipLaunchKernelGGL((qa_head_kernel<E, T>), grid, block, 0, s, (const T*)x, (const T*)w, b, start, end, rows)
  switch (H * 2 + (f32 ? 1 : 0)) {
    case 1024: TC_QA(8, uint16_t); break;
    case 1025: TC_QA(8, float); break;
    case 2048: TC_QA(16, uint16_t); break;
    case 2049: TC_QA(16, float); break;
    case 4096: TC_QA(32, uint16_t); break;
    case 4097: TC_QA(32, float); break;
    case 8192: TC_QA(64, uint16_t); break;
    case 8193: TC_QA(64, float); break;
    default: return hipErrorInvalidValue;
  }
#undef TC_QA
  return hipGetLastError();
}

// Embedding sum + LayerNorm (H in {512, 1024, 2048, 4096}): out [rows][H] bf16
// = LN(word[ids] + pos[row % S] + type[types]); ids / types int64 [rows].
int tcamd_embed_layernorm(const int64_t* ids, const int64_t* types, const void* word, const void* pos,
                          const void* type, const void* gamma, const void* beta, void* out, int rows, int S, int H,
                          int vocab, int ntypes, float eps, void* stream) {
  if (rows <= 0) return hipSuccess;
  if (!ids || !types || S <= 0 || vocab <= 0 || ntypes <= 0 ||
      ((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) % 16)
    return hipErrorInvalidValue;
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  const auto *w = (const uint16_t*)word, *p = (const uint16_t*)pos, *t = (const uint16_t*)type;
  const auto *g = (const uint16_t*)gamma, *b = (const uint16_t*)beta;
  auto* o = (uint16_t*)out;
  switch (H) {
    case 512: hipLaunchKernelGGL(embed_layernorm_kernel<8>, grid, block, 0, st, ids, types, w, p, t, g, b, o, rows, S, vocab, ntypes, eps); break;
    case 1024: hipLaunchKernelGGL(embed_layernorm_kernel<16>, grid, block, 0, st, ids, types, w, p, t, g, b, o, rows, S, vocab, ntypes, eps); break;
    case 2048: hipLaunchKernelGGL(embed_layernorm_kernel<32>, grid, block, 0, st, ids, types, w, p, t, g, b, o, rows, S, vocab, ntypes, eps); break;
    case 4096: hipLaunchKernelGGL(embed_layernorm_kernel<64>, grid, block, 0, st, ids, types, w, p, t, g, b, o, rows, S, vocab, ntypes, eps); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// K12's launch plan: one block per (sequence, head) with a wave per 32
// queries; small batches split a head's queries over 3 or 2 blocks (each
// staging the head's K/V) as long as that still fits one block per CU
// (bs1/4/8 x 384: 13/14/~16 us vs torch SDPA 17/17/22 unmasked).  *splits
// blocks per head (grid.y) of *waves waves each.  Host only: the tests ask it
// which path a shape takes.
int tcamd_attention_plan(int seqs, int S, int heads, int* splits, int* waves) {
  if (seqs <= 0 || S <= 0 || S % 64 || S > kAMaxS || heads <= 0 || !splits || !waves) return hipErrorInvalidValue;
  const int nw = S / 32;
  int sp1 = 1;
  for (int sp : {3, 2})
    if (sp1 == 1 && nw % sp == 0 && nw / sp >= 2 && seqs * heads * sp <= 256) sp1 = sp;
  *splits = sp1;
  *waves = nw / sp1;
  return hipSuccess;
}

// K12v's launch plan, fixed per (rows, heads) so a graph can capture it: K12's
// at S = 384 (a row may be that long).  Host only.
int tcamd_attention_packed_plan(int rows, int heads, int* splits, int* waves) {
  return tcamd_attention_plan(rows, kAMaxS, heads, splits, waves);
}

// K12x's launch plan: *waves = 8 (128 queries per block: half the K / V
// staging per query; bs64 x 384: 331 -> 248 us) once that still gives every
// CU a block, else 4 (bs1 keeps 64 queries: 20.5 vs 21.2 us;
// profiles/r6_bert_fp32/k12x_ab*.log).  Host only.
int tcamd_attention_f32_plan(int seqs, int S, int heads, int* waves) {
  if (seqs <= 0 || S <= 0 || S % 64 || heads <= 0 || !waves) return hipErrorInvalidValue;
  *waves = (S % 128 == 0 && seqs * heads * (S / 128) >= 256) ? 8 : 4;
  return hipSuccess;
}

// K12: multi-head attention over qkv [seqs * S][3 * heads * 64] bf16 (the fused
// QKV projection's output: q | k | v, each [heads][64]) -> out [seqs * S][heads *
// 64] bf16.  mask: int32 [seqs][S] key-padding mask (0 = padded) or null.
// S % 64 == 0 and S <= 384; pointers 16-B aligned.
int tcamd_attention_bias(const void* qkv, const void* qkv_bias, const int* mask, void* out, int seqs, int S, int heads,
                         float scale, void* stream) {
  if (seqs <= 0) return hipSuccess;
  if (S <= 0 || S % 64 || S > kAMaxS || heads <= 0 || ((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)qkv_bias) % 16 ||
      (uintptr_t)mask % 16)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)S * kAD * 2 * 2 + (size_t)S * 4;  // K rows | V rows | key bias
  static bool attr = false;
  if (!attr) {
    hipError_t e =
        hipFuncSetAttribute((const void*)attention_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)attention_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    if (e != hipSuccess) return e;
    attr = true;
  }
  // (a streamed variant — 4-wave blocks, K/V in double-buffered 64-key chunks,
  // 35 KB of LDS — measured slower: 98-105 us vs 93 us at bs64 x 384; the
  // kernel is bound by the softmax VALU work, not by staging)
  int splits = 1, qw = S / 32;
  if (const int e = tcamd_attention_plan(seqs, S, heads, &splits, &qw)) return e;
  const dim3 grid(seqs * heads, splits), block(64 * qw);
  if (mask)
    hipLaunchKernelGGL(attention_kernel<true>, grid, block, lds, (hipStream_t)stream, (const uint16_t*)qkv, mask,
                       (uint16_t*)out, S, heads, scale, (const uint16_t*)qkv_bias);
  else
    hipLaunchKernelGGL(attention_kernel<false>, grid, block, lds, (hipStream_t)stream, (const uint16_t*)qkv, mask,
                       (uint16_t*)out, S, heads, scale, (const uint16_t*)qkv_bias);
  return hipGetLastError();
}

// K12v: K12 over packed rows.  qkv [t_cap][3 * heads * 64] bf16, row r's tokens
// at cu[r] .. cu[r] + row_len[r] - 1 (row_len / cu int32 on the device, from
// tcamd_bert_pack_plan; row_len <= 384) -> out [t_cap][heads * 64] bf16, of
// which only the rows' own tokens are written.  qkv_bias as K12's, or null.
// rows <= 128; pointers 16-B aligned.
int tcamd_attention_packed(const void* qkv, const void* qkv_bias, const int* row_len, const int* cu, void* out, int rows,
                           int t_cap, int heads, float scale, void* stream) {
  if (rows <= 0 || t_cap <= 0) return hipSuccess;
  if (!qkv || !out || !row_len || !cu || rows > 128 || heads <= 0 ||
      ((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)qkv_bias) % 16 || ((uintptr_t)row_len | (uintptr_t)cu) % 4)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)kAMaxS * kAD * 2 * 2 + (size_t)kAMaxS * 4;  // as K12 at S = 384
  static std::atomic<bool> attr{false};
  if (!attr.load(std::memory_order_acquire)) {
    const hipError_t e = hipFuncSetAttribute((const void*)attention_packed_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr.store(true, std::memory_order_release);
  }
  int splits = 1, qw = kAMaxS / 32;
  if (const int e = tcamd_attention_packed_plan(rows, heads, &splits, &qw)) return e;
  hipLaunchKernelGGL(attention_packed_kernel, dim3(rows * heads, splits), dim3(64 * qw), lds, (hipStream_t)stream,
                     (const uint16_t*)qkv, row_len, cu, (uint16_t*)out, t_cap, heads, scale,
                     (const uint16_t*)qkv_bias);
  return hipGetLastError();
}

// K12x: fp32-parity attention over qkv [seqs * S][3 * heads * 64] fp32 (bias
// included) -> out [seqs * S][heads * 64] fp32; mask int32 [seqs][S] (0 =
// padded: additive -10000) or null.  S % 64 == 0; pointers 16-B aligned.
// x3: out is the out-projection's bf16x3 operand, bf16 [seqs * S][3 * heads * 64].
int tcamd_attention_f32(const float* qkv, const int* mask, void* out, int seqs, int S, int heads, float scale, int x3,
                        void* stream) {
  if (seqs <= 0) return hipSuccess;
  if (S <= 0 || S % 64 || heads <= 0 || ((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)mask) % 16)
    return hipErrorInvalidValue;
  float* const o32 = x3 ? nullptr : (float*)out;
  uint16_t* const o3 = x3 ? (uint16_t*)out : nullptr;
  static std::atomic<bool> attr{false};  // 72.5 KB of dynamic LDS: past the 64 KB default
  if (!attr.load(std::memory_order_acquire)) {
    for (const void* fn : {(const void*)attention_x3_kernel<4>, (const void*)attention_x3_kernel<8>}) {
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsAX);
      if (e != hipSuccess) return e;
    }
    attr.store(true, std::memory_order_release);
  }
  int waves = 4;
  if (const int e = tcamd_attention_f32_plan(seqs, S, heads, &waves)) return e;
  if (waves == 8)
    hipLaunchKernelGGL(attention_x3_kernel<8>, dim3(seqs * heads, S / 128), dim3(512), kLdsAX, (hipStream_t)stream,
                       qkv, mask, o32, o3, S, heads, scale);
  else
    hipLaunchKernelGGL(attention_x3_kernel<4>, dim3(seqs * heads, S / 64), dim3(256), kLdsAX, (hipStream_t)stream,
                       qkv, mask, o32, o3, S, heads, scale);
  return hipGetLastError();
}

// K12xv's launch plan, fixed per (rows, heads) so a graph can capture it:
// K12x's at S = 384 (a row may be that long).  Host only.
int tcamd_attention_f32_packed_plan(int rows, int heads, int* waves) {
  return tcamd_attention_f32_plan(rows, kAMaxS, heads, waves);
}

// K12xv: K12x over packed rows.  qkv [t_cap][3 * heads * 64] fp32 (bias
// included), row r's tokens at cu[r] .. cu[r] + row_len[r] - 1 (row_len / cu
// int32 on the device, from tcamd_bert_pack_plan; row_len <= 384) -> out
// [t_cap][heads * 64] fp32 or, with x3, the out-projection's bf16x3 operand,
// bf16 [t_cap][3 * heads * 64]; only the rows' own tokens are written.
// rows <= 128; qkv / out 16-B aligned.
int tcamd_attention_f32_packed(const float* qkv, const int* row_len, const int* cu, void* out, int rows, int t_cap,
                               int heads, float scale, int x3, void* stream) {
  if (rows <= 0 || t_cap <= 0) return hipSuccess;
  if (!qkv || !out || !row_len || !cu || rows > 128 || heads <= 0 || ((uintptr_t)qkv | (uintptr_t)out) % 16 ||
      ((uintptr_t)row_len | (uintptr_t)cu) % 4)
    return hipErrorInvalidValue;
  float* const o32 = x3 ? nullptr : (float*)out;
  uint16_t* const o3 = x3 ? (uint16_t*)out : nullptr;
  static std::atomic<bool> attr{false};  // its own flag: these are other functions than K12x's
  if (!attr.load(std::memory_order_acquire)) {
    for (const void* fn : {(const void*)attention_x3_packed_kernel<4>, (const void*)attention_x3_packed_kernel<8>}) {
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsAX);
      if (e != hipSuccess) return e;
    }
    attr.store(true, std::memory_order_release);
  }
  int waves = 4;
  if (const int e = tcamd_attention_f32_packed_plan(rows, heads, &waves)) return e;
  if (waves == 8)
    hipLaunchKernelGGL(attention_x3_packed_kernel<8>, dim3(rows * heads, kAMaxS / 128), dim3(512), kLdsAX,
                       (hipStream_t)stream, qkv, row_len, cu, o32, o3, t_cap, heads, scale);
  else
    hipLaunchKernelGGL(attention_x3_packed_kernel<4>, dim3(rows * heads, kAMaxS / 64), dim3(256), kLdsAX,
                       (hipStream_t)stream, qkv, row_len, cu, o32, o3, t_cap, heads, scale);
  return hipGetLastError();
}

// K12 without a bias (the projection's output already holds it)
int tcamd_attention(const void* qkv, const int* mask, void* out, int seqs, int S, int heads, float scale,
                    void* stream) {
  return tcamd_attention_bias(qkv, nullptr, mask, out, seqs, S, heads, scale, stream);
}

}  // extern "C"
