// The host twin of K27 qa_spans (csrc/kernels/qa_spans.hip): the same
// arguments on host pointers, the same spans and score bits, by the rule both
// compile from kernels/qa_span_math.h.  It keeps the k largest keys of a row in
// a min-heap while it walks the candidates once, where the kernel selects by
// rounds; "largest key first" makes the two agree.
#include <algorithm>
#include <functional>

#include "../kernels/qa_span_math.h"

namespace {

// start_ok null: every eligible token may start a span
int qa_spans_host(const float* start, const float* end, uint64_t logit_stride_bytes, const int32_t* mask,
                  const int32_t* ttype, const int32_t* start_ok, uint64_t ids_stride_bytes, int32_t rows, int32_t S,
                  const int32_t* k_row, const int32_t* len_row, int32_t kmax, int32_t* spans, float* scores,
                  float* null_score) {
  using namespace tcamd_qa;
  const auto row = [](const void* base, int64_t r, uint64_t stride) {
    return static_cast<const uint8_t*>(base) + r * stride;
  };
  const auto put = [](float* dst, uint32_t bits) { __builtin_memcpy(dst, &bits, 4); };
  uint64_t heap[kKMax];
  for (int64_t r = 0; r < rows; ++r) {
    const int k = clamp_k(k_row[r], kmax);
    if (k == 0) continue;
    const float* st = reinterpret_cast<const float*>(row(start, r, logit_stride_bytes));
    const float* en = reinterpret_cast<const float*>(row(end, r, logit_stride_bytes));
    const int32_t* mk = reinterpret_cast<const int32_t*>(row(mask, r, ids_stride_bytes));
    const int32_t* tt = reinterpret_cast<const int32_t*>(row(ttype, r, ids_stride_bytes));
    const int32_t* so = start_ok ? reinterpret_cast<const int32_t*>(row(start_ok, r, ids_stride_bytes)) : nullptr;
    put(null_score + r, score_bits(f32_bits(st[0]), f32_bits(en[0])));
    const int L = clamp_len(len_row[r], S);
    int n = 0;  // keys in the heap, the smallest on top
    for (int s = 0; s < S && L > 0; ++s) {
      if (!eligible(mk[s], tt[s]) || (so && so[s] < 1)) continue;
      const int hi = std::min(s + L, (int)S);
      for (int e = s; e < hi; ++e) {
        if (!eligible(mk[e], tt[e])) continue;
        const uint64_t key =
            span_key(score_bits(f32_bits(st[s]), f32_bits(en[e])), (uint32_t)s * (uint32_t)S + (uint32_t)e);
        if (n < k) {
          heap[n++] = key;
          std::push_heap(heap, heap + n, std::greater<uint64_t>());
        } else if (key > heap[0]) {
          std::pop_heap(heap, heap + n, std::greater<uint64_t>());
          heap[n - 1] = key;
          std::push_heap(heap, heap + n, std::greater<uint64_t>());
        }
      }
    }
    std::sort(heap, heap + n, std::greater<uint64_t>());
    int32_t* sp = spans + r * (int64_t)kmax * 2;
    float* sc = scores + r * (int64_t)kmax;
    for (int j = 0; j < k; ++j) {
      if (j < n) {
        const uint32_t idx = key_index(heap[j]);
        const int s = (int)(idx / (uint32_t)S), e = (int)(idx % (uint32_t)S);
        sp[2 * j] = s;
        sp[2 * j + 1] = e;
        put(sc + j, score_bits(f32_bits(st[s]), f32_bits(en[e])));
      } else {
        sp[2 * j] = sp[2 * j + 1] = kFillerIndex;
        put(sc + j, kFillerBits);
      }
    }
  }
  return 0;
}

}  // namespace

extern "C" {

// Returns 0, or 1 (the value of hipErrorInvalidValue) for what the device entry
// refuses too; then nothing is written.
int tcamd_host_qa_spans(const float* start, const float* end, uint64_t logit_stride_bytes, const int32_t* mask,
                        const int32_t* ttype, uint64_t ids_stride_bytes, int32_t rows, int32_t S, const int32_t* k_row,
                        const int32_t* len_row, int32_t kmax, int32_t* spans, float* scores, float* null_score) {
  if (!tcamd_qa::args_valid(start, end, logit_stride_bytes, mask, ttype, ids_stride_bytes, rows, S, k_row, len_row,
                            kmax, spans, scores, null_score))
    return 1;
  return qa_spans_host(start, end, logit_stride_bytes, mask, ttype, nullptr, ids_stride_bytes, rows, S, k_row, len_row,
                       kmax, spans, scores, null_score);
}

// The host twin of tcamd_qa_spans_masked: a span may start only where start_ok >= 1.
int tcamd_host_qa_spans_masked(const float* start, const float* end, uint64_t logit_stride_bytes, const int32_t* mask,
                               const int32_t* ttype, const int32_t* start_ok, uint64_t ids_stride_bytes, int32_t rows,
                               int32_t S, const int32_t* k_row, const int32_t* len_row, int32_t kmax, int32_t* spans,
                               float* scores, float* null_score) {
  if (!tcamd_qa::args_valid(start, end, logit_stride_bytes, mask, ttype, ids_stride_bytes, rows, S, k_row, len_row,
                            kmax, spans, scores, null_score) ||
      !start_ok || ((uintptr_t)start_ok & 3))
    return 1;
  return qa_spans_host(start, end, logit_stride_bytes, mask, ttype, start_ok, ids_stride_bytes, rows, S, k_row, len_row,
                       kmax, spans, scores, null_score);
}

}  // extern "C"
