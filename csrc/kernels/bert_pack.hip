// K30 — the pack plan of a padding-free bert_large forward, with the packed
// embedding LayerNorm in front of the layers and the logit unpack behind them
// (gfx950).
//
// A served BERT row is 384 tokens of which a question plus a paragraph fills
// 100-250; every projection, LayerNorm, GELU and the QA head cost the same
// for a padding token as for a real one.  The packed forward keeps only the
// tokens whose attention_mask is >= 1, back to back in row order, runs every
// per-token operator over that dense list of t_cap tokens and attends within
// each row's own tokens (K12v, csrc/kernels/bert.hip).  Three kernels here:
//
//   bert_pack_plan          mask [rows][S] -> row_len, cu (exclusive scan),
//                           tok_src (packed token -> r * S + p) and tok_of
//                           (r * S + p -> packed token or -1): a stable
//                           compaction.  ONE workgroup: a wave per row takes
//                           the row's 64-position ballots and popcounts, one
//                           scan over the <= 128 row lengths in LDS, then the
//                           same waves write the indices.  No workgroup waits
//                           on another and nothing is atomic.
//   embed_layernorm_packed  token t: LN(word[wrap(ids[src])] + pos[src % S] +
//                           type[clamp(tt[src])]), src = tok_src[t], straight
//                           from the int32 request tensors; a pad token
//                           (src = -1) is id 0, position 0, type 0, so it is
//                           finite.  The bits of embed_layernorm for the same
//                           (row, position): the same sum, the same
//                           ln_store_row (kernels/bert_ln.h).  An fp32 form
//                           for the fp32-parity model: fp32 tables and
//                           output, optionally also the first QKV
//                           projection's bf16x3 operand.
//   unpack_logits           out[r][p] = tok_of >= 0 ? packed[tok_of] :
//                           PAD_LOGIT for both logit planes in one launch.
// Reference analog: none (the reference client runs no model).

#include <algorithm>

#include "kernels/bert_ln.h"
#include "kernels/common.h"

namespace {

using tcamd_bert::ln_store_row;
using tcamd_bert::v4u;

constexpr int kPackMaxRows = 128;
constexpr int kPackMaxS = 384;
constexpr int kPackThreads = 1024;  // 16 waves
constexpr float kPadLogit = -10000.0f;  // the model's additive mask constant

// Barriers: two, both at the top level of the kernel, between loops whose
// trip counts depend on the wave index alone -- no wave returns or branches
// around one.
__global__ void __launch_bounds__(kPackThreads) bert_pack_plan_kernel(const int* __restrict__ mask, long long mask_stride,
                                                                      int rows, int S, int t_cap,
                                                                      int* __restrict__ row_len, int* __restrict__ cu,
                                                                      int* __restrict__ tok_src,
                                                                      int* __restrict__ tok_of) {
  __shared__ int len_s[kPackMaxRows];
  __shared__ int cu_s[kPackMaxRows + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kPackThreads / 64;
  const int nch = (S + 63) >> 6;
  // 1. a wave per row: the row's length from its ballots
  for (int r = wave; r < rows; r += nw) {
    int n = 0;
    for (int c = 0; c < nch; ++c) {
      const int p = 64 * c + lane;
      const bool v = p < S && mask[r * mask_stride + p] >= 1;
      n += __popcll(__ballot(v));
    }
    if (lane == 0) len_s[r] = n;
  }
  __syncthreads();
  // 2. the exclusive scan over the rows (<= 128 LDS reads per thread)
  if (tid <= rows) {
    int s = 0;
    for (int i = 0; i < tid; ++i) s += len_s[i];
    cu_s[tid] = s;
    cu[tid] = s;
    if (tid < rows) row_len[tid] = len_s[tid];
  }
  __syncthreads();
  // 3. the same waves write the indices: positions ascending within a row
  for (int r = wave; r < rows; r += nw) {
    int t0 = cu_s[r];
    for (int c = 0; c < nch; ++c) {
      const int p = 64 * c + lane;
      const bool v = p < S && mask[r * mask_stride + p] >= 1;
      const unsigned long long bal = __ballot(v);
      const int t = t0 + __popcll(bal & ((1ull << lane) - 1ull));
      const bool fits = v && t < t_cap;
      if (fits) tok_src[t] = r * S + p;
      if (p < S) tok_of[r * S + p] = fits ? t : -1;
      t0 += __popcll(bal);
    }
  }
  // 4. the pad tokens [T, t_cap)
  for (int t = cu_s[rows] + tid; t < t_cap; t += kPackThreads) tok_src[t] = -1;
}

template <int E>
__global__ void __launch_bounds__(256) embed_layernorm_packed_kernel(
    const int* __restrict__ ids, const int* __restrict__ types, const int* __restrict__ tok_src,
    const uint16_t* __restrict__ word, const uint16_t* __restrict__ pos, const uint16_t* __restrict__ tok,
    const uint16_t* __restrict__ gamma, const uint16_t* __restrict__ beta, uint16_t* __restrict__ out, int t_cap, int n_src,
    int S, int vocab, int ntypes, float eps) {
  constexpr int H = 64 * E, C = E / 8;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= t_cap) return;
  const int src = tok_src[t];
  int id = 0, ty = 0, p = 0;
  if (src >= 0 && src < n_src) {  // else a pad token: id 0, position 0, type 0
    id = ids[src] % vocab;  // the served model's remainder(vocab): non-negative
    if (id < 0) id += vocab;
    ty = min(max(types[src], 0), ntypes - 1);
    p = src % S;
  }
  const uint16_t* rw = word + (size_t)id * H;
  const uint16_t* rp = pos + (size_t)p * H;
  const uint16_t* rt = tok + (size_t)ty * H;
  float v[E];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int off = (c * 64 + lane) * 8;
    const v4u a = *reinterpret_cast<const v4u*>(rw + off);
    const v4u b = *reinterpret_cast<const v4u*>(rp + off);
    const v4u tt = *reinterpret_cast<const v4u*>(rt + off);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[c * 8 + 2 * q] = __uint_as_float(a[q] << 16) + __uint_as_float(b[q] << 16) + __uint_as_float(tt[q] << 16);
      v[c * 8 + 2 * q + 1] = __uint_as_float(a[q] & 0xffff0000u) + __uint_as_float(b[q] & 0xffff0000u) +
                             __uint_as_float(tt[q] & 0xffff0000u);
    }
  }
  ln_store_row<E>(v, gamma, beta, out + (size_t)t * H, lane, eps);
}

// The fp32-parity model's form: fp32 tables, the fp32 sum in the bf16 kernel's
// order, ln_store_row's fp32 form; out3 (or null) is the first QKV
// projection's bf16x3 operand [t_cap][3H], so the packed graph runs no x3_cat.
template <int E>
__global__ void __launch_bounds__(256) embed_layernorm_packed_f32_kernel(
    const int* __restrict__ ids, const int* __restrict__ types, const int* __restrict__ tok_src,
    const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ tok,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out,
    uint16_t* __restrict__ out3, int t_cap, int n_src, int S, int vocab, int ntypes, float eps) {
  constexpr int H = 64 * E, C = E / 8;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= t_cap) return;
  const int src = tok_src[t];
  int id = 0, ty = 0, p = 0;
  if (src >= 0 && src < n_src) {  // else a pad token: id 0, position 0, type 0
    id = ids[src] % vocab;
    if (id < 0) id += vocab;
    ty = min(max(types[src], 0), ntypes - 1);
    p = src % S;
  }
  const float* rw = word + (size_t)id * H;
  const float* rp = pos + (size_t)p * H;
  const float* rt = tok + (size_t)ty * H;
  float v[E];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int off = (c * 64 + lane) * 8;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float4 a = *reinterpret_cast<const float4*>(rw + off + 4 * hf);
      const float4 b = *reinterpret_cast<const float4*>(rp + off + 4 * hf);
      const float4 tt = *reinterpret_cast<const float4*>(rt + off + 4 * hf);
      v[c * 8 + 4 * hf] = a.x + b.x + tt.x;
      v[c * 8 + 4 * hf + 1] = a.y + b.y + tt.y;
      v[c * 8 + 4 * hf + 2] = a.z + b.z + tt.z;
      v[c * 8 + 4 * hf + 3] = a.w + b.w + tt.w;
    }
  }
  ln_store_row<E>(v, gamma, beta, out + (size_t)t * H, out3 ? out3 + (size_t)t * 3 * H : nullptr, lane, eps);
}

__global__ void __launch_bounds__(256) unpack_logits_kernel(const float* __restrict__ ps, const float* __restrict__ pe,
                                                            const int* __restrict__ tok_of, float* __restrict__ os,
                                                            float* __restrict__ oe, int n, int t_cap) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int t = tok_of[i];
    const bool real = t >= 0 && t < t_cap;
    os[i] = real ? ps[t] : kPadLogit;
    oe[i] = real ? pe[t] : kPadLogit;
  }
}

}  // namespace

extern "C" {

// The logit the unpack writes where attention_mask < 1.
float tcamd_bert_pad_logit(void) { return kPadLogit; }

// K30: mask int32 [rows][S] at a row stride of mask_stride elements (any mask,
// not only a prefix; valid = mask >= 1), rows <= 128, S <= 384 ->
//   row_len [rows]      valid positions per row
//   cu [rows + 1]       exclusive scan of row_len; cu[rows] = T
//   tok_src [t_cap]     r * S + p of packed token t (rows in order, positions
//                       ascending); -1 for T <= t < t_cap
//   tok_of [rows * S]   the packed token of (r, p), or -1 (mask < 1, or a
//                       token that did not fit t_cap)
// all int32 on the device.  With T > t_cap nothing past t_cap is written and
// cu[rows] still holds the true T: the caller checks it.
int tcamd_bert_pack_plan(const int* mask, long long mask_stride, int rows, int S, int t_cap, int* row_len, int* cu,
                         int* tok_src, int* tok_of, void* stream) {
  if (rows <= 0) return hipSuccess;
  if (!mask || !row_len || !cu || !tok_src || !tok_of || rows > kPackMaxRows || S <= 0 || S > kPackMaxS || t_cap < 0 ||
      mask_stride < S)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bert_pack_plan_kernel, dim3(1), dim3(kPackThreads), 0, (hipStream_t)stream, mask, mask_stride, rows,
                     S, t_cap, row_len, cu, tok_src, tok_of);
  return hipGetLastError();
}

// Packed embedding sum + LayerNorm (H in {512, 1024, 2048, 4096}): out
// [t_cap][H] bf16; ids / types int32 [rows * S] (n_src = rows * S elements),
// tok_src int32 [t_cap] from tcamd_bert_pack_plan.  ids wrap (remainder
// vocab), types clamp to [0, ntypes - 1], as the served model applies them.
int tcamd_embed_layernorm_packed(const int* ids, const int* types, const int* tok_src, const void* word, const void* pos,
                                 const void* type, const void* gamma, const void* beta, void* out, int t_cap, int n_src,
                                 int S, int H, int vocab, int ntypes, float eps, void* stream) {
  if (t_cap <= 0) return hipSuccess;
  if (!ids || !types || !tok_src || n_src <= 0 || S <= 0 || vocab <= 0 || ntypes <= 0 ||
      ((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) % 16)
    return hipErrorInvalidValue;
  const dim3 grid((t_cap + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  const auto *w = (const uint16_t*)word, *p = (const uint16_t*)pos, *t = (const uint16_t*)type;
  const auto *g = (const uint16_t*)gamma, *b = (const uint16_t*)beta;
  auto* o = (uint16_t*)out;
#define TC_EMBP(E)                                                                                                 \
  hipLaunchKernelGGL(embed_layernorm_packed_kernel<E>, grid, block, 0, st, ids, types, tok_src, w, p, t, g, b, o, \
                     t_cap, n_src, S, vocab, ntypes, eps)
  switch (H) {
    case 512: TC_EMBP(8); break;
    case 1024: TC_EMBP(16); break;
    case 2048: TC_EMBP(32); break;
    case 4096: TC_EMBP(64); break;
    default: return hipErrorInvalidValue;
  }
#undef TC_EMBP
  return hipGetLastError();
}

// The fp32-parity form: fp32 tables / gamma / beta, out fp32 [t_cap][H]; out3
// (or null): bf16 [t_cap][3H] = [hi | hi | lo], bitwise x3_cat of out.  The
// same gather rule.  16-B aligned pointers.
int tcamd_embed_layernorm_packed_f32(const int* ids, const int* types, const int* tok_src, const float* word,
                                     const float* pos, const float* type, const float* gamma, const float* beta,
                                     float* out, void* out3, int t_cap, int n_src, int S, int H, int vocab, int ntypes,
                                     float eps, void* stream) {
  if (t_cap <= 0) return hipSuccess;
  if (!ids || !types || !tok_src || !word || !pos || !type || !gamma || !beta || !out || n_src <= 0 || S <= 0 ||
      vocab <= 0 || ntypes <= 0 ||
      ((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out |
       (uintptr_t)out3) % 16)
    return hipErrorInvalidValue;
  const dim3 grid((t_cap + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
#define TC_EMBPF(E)                                                                                                \
  hipLaunchKernelGGL(embed_layernorm_packed_f32_kernel<E>, grid, block, 0, st, ids, types, tok_src, word, pos, type, \
                     gamma, beta, out, (uint16_t*)out3, t_cap, n_src, S, vocab, ntypes, eps)
  switch (H) {
    case 512: TC_EMBPF(8); break;
    case 1024: TC_EMBPF(16); break;
    case 2048: TC_EMBPF(32); break;
    case 4096: TC_EMBPF(64); break;
    default: return hipErrorInvalidValue;
  }
#undef TC_EMBPF
  return hipGetLastError();
}

// out_start / out_end fp32 [n] (n = rows * S): the packed logits of the tokens
// tok_of names, PAD_LOGIT (-10000) elsewhere.
int tcamd_unpack_logits(const float* packed_start, const float* packed_end, const int* tok_of, float* out_start,
                        float* out_end, int n, int t_cap, void* stream) {
  if (n <= 0) return hipSuccess;
  if (!packed_start || !packed_end || !tok_of || !out_start || !out_end || t_cap < 0) return hipErrorInvalidValue;
  const int grid = std::min((n + 255) / 256, 1024);
  hipLaunchKernelGGL(unpack_logits_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, packed_start, packed_end,
                     tok_of, out_start, out_end, n, t_cap);
  return hipGetLastError();
}

}  // extern "C"
