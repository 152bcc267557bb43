// The host twin of K29 qa_merge (csrc/kernels/qa_merge.hip): the same arguments
// on host pointers, the same spans, rows and score bits, by the rule both
// compile from kernels/qa_span_math.h.  It sorts the union of a document's
// lists, where the kernel merges list heads; on lists that are sorted by the
// merge key, as K27 leaves them, the two agree.
#include <algorithm>
#include <vector>

#include "../kernels/qa_span_math.h"

extern "C" {

// Returns 0, or 1 (the value of hipErrorInvalidValue) for what the device entry
// refuses too; then nothing is written.
int tcamd_host_qa_merge(const int32_t* spans, const float* scores, const float* null_score, int32_t rows,
                        const int32_t* window_info, const uint32_t* doc_info, int32_t docs, const int32_t* k_doc,
                        int32_t kmax, int32_t* out_spans, int32_t* out_windows, float* out_scores, float* out_null) {
  using namespace tcamd_qa;
  if (!merge_args_valid(spans, scores, null_score, rows, window_info, doc_info, docs, k_doc, kmax, out_spans,
                        out_windows, out_scores, out_null))
    return 1;
  const auto put = [](float* dst, uint32_t bits) { __builtin_memcpy(dst, &bits, 4); };
  const auto canon = [](uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u ? kCanonNan : b; };
  struct Cand {
    uint64_t key;
    int32_t row, rank;
  };
  std::vector<Cand> all;
  for (int d = 0; d < docs; ++d) {
    const int k = clamp_k(k_doc[d], kmax);
    if (k == 0) continue;
    int first;
    const int W = merge_rows(doc_info, d, rows, &first);
    all.clear();
    uint32_t null_bits = kFillerBits, null_img = 0;
    for (int w = 0; w < W; ++w) {
      const int64_t r = first + w;
      const uint32_t nb = f32_bits(null_score[r]);
      if (w == 0 || null_image(nb) < null_img) null_bits = canon(nb), null_img = null_image(nb);
      for (int h = 0; h < k; ++h) {
        const int32_t* sp = spans + (r * kmax + h) * 2;
        const uint64_t key = merge_key(sp[0], sp[1], f32_bits(scores[r * kmax + h]), window_info + 4 * r);
        if (key == 0) break;  // a filler rank ends the list
        all.push_back({key, (int32_t)r, h});
      }
    }
    std::sort(all.begin(), all.end(), [](const Cand& a, const Cand& b) {
      return a.key != b.key ? a.key > b.key : a.row != b.row ? a.row < b.row : a.rank < b.rank;
    });
    put(out_null + d, null_bits);
    int32_t* sp = out_spans + (int64_t)d * kmax * 2;
    int32_t* wn = out_windows + (int64_t)d * kmax;
    float* sc = out_scores + (int64_t)d * kmax;
    for (int j = 0; j < k; ++j) {
      if (j < (int)all.size()) {
        const Cand& c = all[j];
        sp[2 * j] = spans[((int64_t)c.row * kmax + c.rank) * 2];
        sp[2 * j + 1] = spans[((int64_t)c.row * kmax + c.rank) * 2 + 1];
        wn[j] = c.row;
        put(sc + j, canon(f32_bits(scores[(int64_t)c.row * kmax + c.rank])));
      } else {
        sp[2 * j] = sp[2 * j + 1] = wn[j] = kFillerIndex;
        put(sc + j, kFillerBits);
      }
    }
  }
  return 0;
}

}  // extern "C"
