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
// With a start mask (tcamd_qa_spans_masked; start_ok[S] int32 per row, the
// start_mask of K28w) a candidate (s, e) additionally needs start_ok[s] >= 1;
// the end needs eligibility only, as in run_squad, where a window may end an
// answer on a piece another window owns but may not start one there.  Without
// a mask every eligible token may start.
//
// Per row: the k best spans and their scores, and null_score = start[0] + end[0]
// (canonical when NaN), whatever the eligibility of token 0.  A row with fewer
// than k candidates fills the remaining ranks with span (-1, -1) and score
// -FLT_MAX.  L above S is S; L below 1 leaves no candidate.
//
// The merge across the windows of a document (K29 qa_merge,
// csrc/kernels/qa_merge.hip, host twin csrc/host/qa_merge.cc).  Document d owns
// rows first_d .. first_d + W_d - 1 of such per-row lists (doc_info of K28w:
// {first row, W, P, status}; a document whose status is not 0 has no rows), and
// row r has window_info[r] = {document, first context piece, context pieces,
// token index of the first context piece}.  A listed span (s, e) of row r starts
// at document piece doc_start = first piece + s - first context token.  The
// document's k best are the k largest of the union of its rows' first k ranks by
//   monotone_u32(score) << 32 | (0xFFFFFFFF - (doc_start * 1024 + (e - s))):
// scores descend, equal scores go to the lower document start and then to the
// shorter span; doc_start < 65,536 and e - s < 1024 keep the low word above 0.
// The start mask gives every document start to exactly one window, so a row's
// list is already sorted by this key (within a row, lower s is lower doc_start
// and lower e the shorter span) and no two rows list the same (doc_start,
// length): the top k of the union of all candidates lies in the union of the
// lists, and a merge of list heads finds it.  Filler ranks of a row end its
// list.  Outputs per document: spans [kmax][2] (tokens of the window's row),
// windows [kmax] (the row; filler -1), scores [kmax], and null_score = the
// minimum of its rows' null scores by the key order (the lowest image; a NaN in
// any row gives the canonical NaN).  Ranks past the candidates hold (-1, -1),
// -1 and -FLT_MAX; a document without rows is all filler and its null_score is
// -FLT_MAX.  k <  1 skips the document.
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

// bits of the per-token byte K27 keeps: eligible, and allowed to start a span
constexpr uint8_t kTokOk = 1, kTokStart = 2;
TCAMD_QA_HD uint8_t token_bits(int32_t attention_mask, int32_t token_type, bool masked, int32_t start_ok) {
  if (!eligible(attention_mask, token_type)) return 0;
  return (uint8_t)(kTokOk | ((!masked || start_ok >= 1) ? kTokStart : 0));
}

// ---- the merge (K29) -------------------------------------------------------------
constexpr int kMergeMaxRows = 128;  // windows of one document, one thread each
constexpr int kMergeSpan = 1024;    // (e - s) < kMergeSpan
constexpr uint32_t kMergeMaxStart = 65536;

// the merge key of rank (s, e, score bits) of a row with window_info wi; 0 for a
// filler rank or one the key cannot hold (which ends the row's list)
TCAMD_QA_HD uint64_t merge_key(int32_t s, int32_t e, uint32_t bits, const int32_t* wi) {
  if (s < 0 || e < s || e - s >= kMergeSpan) return 0;
  const int64_t doc_start = (int64_t)wi[1] + s - wi[3];
  if (doc_start < 0 || doc_start >= (int64_t)kMergeMaxStart) return 0;
  return span_key(bits, (uint32_t)doc_start * (uint32_t)kMergeSpan + (uint32_t)(e - s));
}

// the order of null scores: the image alone (NaN lowest)
TCAMD_QA_HD uint32_t null_image(uint32_t bits) { return (uint32_t)(span_key(bits, 0) >> 32); }

inline bool merge_args_valid(const void* spans, const void* scores, const void* null_score, int32_t rows,
                             const void* window_info, const void* doc_info, int32_t docs, const void* k_doc,
                             int32_t kmax, const void* out_spans, const void* out_windows, const void* out_scores,
                             const void* out_null) {
  if (rows < 0 || docs < 0 || kmax < 1 || kmax > kKMax) return false;
  const void* ptrs[] = {spans, scores, null_score, window_info, doc_info, k_doc, out_spans, out_windows, out_scores,
                        out_null};
  for (const void* p : ptrs)
    if (!p || ((uintptr_t)p & 3)) return false;
  return true;
}

// the rows of document d that the merge reads: none unless its status is 0 and
// they lie inside [0, rows) and are at most kMergeMaxRows
TCAMD_QA_HD int merge_rows(const uint32_t* doc_info, int d, int32_t rows, int* first) {
  const uint32_t f = doc_info[4 * d], w = doc_info[4 * d + 1], st = doc_info[4 * d + 3];
  *first = 0;
  if (st != 0 || w == 0 || w > (uint32_t)kMergeMaxRows || f > (uint32_t)rows || w > (uint32_t)rows - f) return 0;
  *first = (int)f;
  return (int)w;
}

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
