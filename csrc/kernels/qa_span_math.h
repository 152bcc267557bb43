// The rule by which the n best answer spans of a question-answering row are
// picked, shared by K27 qa_spans (csrc/kernels/qa_spans.hip) and its host twin
// (csrc/host/qa_spans.cc) so that the two agree on every span and on the bits of
// every score.  tests/qa_span_cases.py implements it a third time in numpy.
//
// A row has start[S] and end[S] (fp32), attention_mask[S] and token_type_ids[S]
// (int32), an answer count k and a longest answer L.
//
// Token t is eligible when attention_mask[t] >= 1 and token_type_ids[t] == 1
// (the context segment).  A candidate is a pair (s, e) of eligible tokens with
// s <= e and e - s < L; nothing is asked of the tokens in between.  Its score
// is start[s] + end[e], one fp32 addition.  A NaN score is reported as the
// canonical quiet NaN 0x7fc00000, whatever NaN the adder of the machine made
// (inf + -inf is 0xffc00000 on x86 and 0x7fc00000 on the GPU).
//
// The order is K19's (csrc/kernels/topk.hip) with s * S + e for the element
// index: scores descend, equal scores go to the lower s and then to the lower e,
// -0.0 ties with +0.0, infinities order as values, a NaN score ranks below every
// number and NaNs keep index order.  As a key,
//   monotone_u32(score) << 32 | (0xFFFFFFFF - (s * S + e)),
// and "largest key first" is the whole contract.  S <= 1024 keeps the index
// below 2^20, so no candidate's key is 0, which stands for "none".
//
// Per row: the k best spans and their scores, and null_score = start[0] + end[0]
// (canonical when NaN), whatever the eligibility of token 0.  A row with fewer
// than k candidates fills the remaining ranks with span (-1, -1) and score
// -FLT_MAX.  L above S is S; L below 1 leaves no candidate.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TCAMD_QA_HD __host__ __device__ __forceinline__
#else
#define TCAMD_QA_HD inline
#endif

namespace tcamd_qa {

constexpr int kMaxSeq = 1024;  // S
constexpr int kKMax = 64;      // kmax
constexpr uint32_t kCanonNan = 0x7fc00000u;
constexpr uint32_t kFillerBits = 0xff7fffffu;  // -FLT_MAX
constexpr int32_t kFillerIndex = -1;

TCAMD_QA_HD uint32_t f32_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

TCAMD_QA_HD float bits_f32(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

TCAMD_QA_HD bool eligible(int32_t attention_mask, int32_t token_type) { return attention_mask >= 1 && token_type == 1; }

// the bits of start + end, a NaN made canonical
TCAMD_QA_HD uint32_t score_bits(uint32_t start_bits, uint32_t end_bits) {
  const uint32_t b = f32_bits(bits_f32(start_bits) + bits_f32(end_bits));
  return (b & 0x7fffffffu) > 0x7f800000u ? kCanonNan : b;
}

TCAMD_QA_HD uint64_t span_key(uint32_t bits, uint32_t idx) {
  uint32_t m;
  if ((bits & 0x7fffffffu) > 0x7f800000u) {
    m = 0u;  // NaN: below -inf (whose image is 0x007fffff)
  } else {
    if (bits == 0x80000000u) bits = 0u;  // -0.0 ties with +0.0
    m = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return ((uint64_t)m << 32) | (uint64_t)(0xFFFFFFFFu - idx);
}

TCAMD_QA_HD uint32_t key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// the longest answer of a row: above S it is S, below 1 there is no candidate (0)
TCAMD_QA_HD int clamp_len(int32_t L, int S) { return L < 1 ? 0 : (L > S ? S : (int)L); }

// the ranks a row gets: min(k_row, kmax), 0 = the row is skipped
TCAMD_QA_HD int clamp_k(int32_t k, int kmax) { return k < 1 ? 0 : (k > kmax ? kmax : (int)k); }

// What both entry points refuse before touching anything: S outside [1, 1024],
// kmax outside [1, 64], negative rows, a null pointer, a pointer that is not
// 4-byte aligned, a row stride that is no multiple of 4 or, with more than one
// row, shorter than a row.
inline bool args_valid(const void* start, const void* end, uint64_t logit_stride, const void* mask, const void* ttype,
                       uint64_t ids_stride, int32_t rows, int32_t S, const void* k_row, const void* len_row,
                       int32_t kmax, const void* spans, const void* scores, const void* null_score) {
  if (rows < 0 || S < 1 || S > kMaxSeq || kmax < 1 || kmax > kKMax) return false;
  const void* ptrs[] = {start, end, mask, ttype, k_row, len_row, spans, scores, null_score};
  for (const void* p : ptrs)
    if (!p || ((uintptr_t)p & 3)) return false;
  if ((logit_stride & 3) || (ids_stride & 3)) return false;
  if (rows > 1 && (logit_stride < (uint64_t)S * 4 || ids_stride < (uint64_t)S * 4)) return false;
  return true;
}

}  // namespace tcamd_qa
