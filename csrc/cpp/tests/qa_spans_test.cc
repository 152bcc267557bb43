// The host twin of K27 qa_spans (csrc/host/qa_spans.cc) on its edge cases, as a
// stand-alone program meant for a sanitizer build too (`make asan` builds it as
// build-asan/bin/qa_spans_test):
//
//   qa_spans_test
//
// Every input and output is a heap block of exactly its size, rows at a stride
// above S * 4 from a base that is 4-byte but not 16-byte aligned, so a read or a
// write past an end is an AddressSanitizer report.  Outputs start as a canary
// and are compared whole with a reference that orders the candidates by a
// comparator on (score, s, e) written out here, not by the header's key: ranks
// past k_row[r], skipped rows and the guard words must still hold the canary.
// Covered: S in 1, 2, 63, 64, 65, 255, 256, 257, 384, 1024; L in 1, 2, S - 1, S
// and above S, 0 and below; k in 1, 20, 64, above kmax, 0 and below; no / one /
// holed eligibility, mask values above 1, token types above 1; equal, integer
// and special-valued logits (NaNs of several payloads, both infinities and
// their sum, -0.0, denormals, +-FLT_MAX); 1, 5 and 129 rows; and everything
// the entry refuses.  Exits 0 when all held.

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../host/qa_spans.cc"

namespace {

constexpr uint32_t kCanary = 0x5A5A5A5Au;
constexpr int kGuard = 8;
int g_failures = 0;
int g_calls = 0;

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

const uint32_t kSpecials[] = {0x7FC00000u, 0xFFC12345u, 0x7FA00001u, 0x7F800000u, 0xFF800000u, 0x80000000u, 0x00000000u,
                              0x00000001u, 0x80000001u, 0x007FFFFFu, 0x7F7FFFFFu, 0xFF7FFFFFu, 0x3F800000u,
                              0xBF800000u};

float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

uint32_t to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

struct Cand {
  float score;
  int s, e;
};

// scores descend, NaN below every number, then the lower s, then the lower e
bool before(const Cand& a, const Cand& b) {
  const bool an = std::isnan(a.score), bn = std::isnan(b.score);
  if (an != bn) return bn;
  if (!an && a.score != b.score) return a.score > b.score;  // -0.0 == +0.0
  if (a.s != b.s) return a.s < b.s;
  return a.e < b.e;
}

uint32_t canon(float f) { return std::isnan(f) ? 0x7FC00000u : to_bits(f); }

struct Call {
  int rows, S, kmax;
  int logits, elig;  // kinds
  std::vector<int32_t> k_row, len_row;
};

void run(const Call& c, Rng& rng) {
  ++g_calls;
  const int rows = c.rows, S = c.S, kmax = c.kmax;
  const int off = 1, stride = S + 3;  // elements
  const size_t in_n = (size_t)off + (size_t)rows * stride - 3;  // the last row ends the block
  std::unique_ptr<float[]> st(new float[in_n]), en(new float[in_n]);
  std::unique_ptr<int32_t[]> mk(new int32_t[in_n]), tt(new int32_t[in_n]);
  for (size_t i = 0; i < in_n; ++i) {
    st[i] = en[i] = from_bits(0x7FC00000u);
    mk[i] = tt[i] = 1;
  }
  for (int r = 0; r < rows; ++r) {
    float* a = st.get() + off + (size_t)r * stride;
    float* b = en.get() + off + (size_t)r * stride;
    int32_t* m = mk.get() + off + (size_t)r * stride;
    int32_t* t = tt.get() + off + (size_t)r * stride;
    const int lk = c.logits < 0 ? r % 4 : c.logits, ek = c.elig < 0 ? (r / 2) % 5 : c.elig;
    for (int i = 0; i < S; ++i) {
      float x = (float)(rng.below(5) - 2), y = (float)(rng.below(5) - 2);
      if (lk == 0) {
        x = (float)(rng.below(2001) - 1000) / 64.0f;
        y = (float)(rng.below(2001) - 1000) / 64.0f;
      } else if (lk == 2) {
        x = y = 1.5f;
      } else if (lk == 3) {
        if (rng.below(10) < 3) x = from_bits(kSpecials[rng.below(14)]);
        if (rng.below(10) < 3) y = from_bits(kSpecials[rng.below(14)]);
      }
      a[i] = x;
      b[i] = y;
      m[i] = t[i] = 1;
      if (ek == 1) t[i] = 0;                                  // none (one below)
      if (ek == 2) { m[i] = rng.below(2); t[i] = rng.below(3); }   // holes
      if (ek == 3) { m[i] = rng.below(3); t[i] = rng.below(5) ? 1 : 2; }  // mask 2, type 2
      if (ek == 4) t[i] = i >= S / 3 ? 1 : 0, m[i] = i < S - S / 4 ? 1 : 0;  // question, context, padding
    }
    if (ek == 1 && r % 2) t[rng.below(S)] = 1;  // one eligible token
  }
  const int o_spans = kGuard, o_scores = o_spans + rows * kmax * 2 + kGuard, o_null = o_scores + rows * kmax + kGuard;
  const int total = o_null + rows + kGuard;
  std::unique_ptr<uint32_t[]> got(new uint32_t[total]), want(new uint32_t[total]);
  std::fill(got.get(), got.get() + total, kCanary);
  std::fill(want.get(), want.get() + total, kCanary);
  std::unique_ptr<int32_t[]> kr(new int32_t[rows]), lr(new int32_t[rows]);
  for (int r = 0; r < rows; ++r) {
    kr[r] = c.k_row[r % c.k_row.size()];
    lr[r] = c.len_row[r % c.len_row.size()];
  }
  // the reference
  for (int r = 0; r < rows; ++r) {
    const int k = std::min(kr[r], kmax);
    if (k < 1) continue;
    const float* a = st.get() + off + (size_t)r * stride;
    const float* b = en.get() + off + (size_t)r * stride;
    const int32_t* m = mk.get() + off + (size_t)r * stride;
    const int32_t* t = tt.get() + off + (size_t)r * stride;
    const int L = std::min(std::max(lr[r], 0), S);
    std::vector<Cand> cs;
    for (int s = 0; s < S; ++s)
      for (int e = s; e < std::min(s + L, S); ++e)
        if (m[s] >= 1 && t[s] == 1 && m[e] >= 1 && t[e] == 1) cs.push_back({a[s] + b[e], s, e});
    const size_t top = std::min((size_t)k, cs.size());
    std::partial_sort(cs.begin(), cs.begin() + top, cs.end(), before);
    for (int j = 0; j < k; ++j) {
      const bool have = (size_t)j < cs.size();
      want[o_spans + (r * kmax + j) * 2] = have ? (uint32_t)cs[j].s : 0xFFFFFFFFu;
      want[o_spans + (r * kmax + j) * 2 + 1] = have ? (uint32_t)cs[j].e : 0xFFFFFFFFu;
      want[o_scores + r * kmax + j] = have ? canon(cs[j].score) : 0xFF7FFFFFu;
    }
    want[o_null + r] = canon(a[0] + b[0]);
  }
  const int rc = tcamd_host_qa_spans(st.get() + off, en.get() + off, (uint64_t)stride * 4, mk.get() + off,
                                     tt.get() + off, (uint64_t)stride * 4, rows, S, kr.get(), lr.get(), kmax,
                                     reinterpret_cast<int32_t*>(got.get() + o_spans),
                                     reinterpret_cast<float*>(got.get() + o_scores),
                                     reinterpret_cast<float*>(got.get() + o_null));
  if (rc != 0) {
    std::printf("FAIL rows %d S %d kmax %d: refused (%d)\n", rows, S, kmax, rc);
    ++g_failures;
    return;
  }
  for (int w = 0; w < total; ++w)
    if (got[w] != want[w]) {
      std::printf("FAIL rows %d S %d kmax %d logits %d elig %d: word %d (spans at %d, scores at %d, null at %d) is "
                  "0x%08x, want 0x%08x\n",
                  rows, S, kmax, c.logits, c.elig, w, o_spans, o_scores, o_null, got[w], want[w]);
      ++g_failures;
      return;
    }
}

// the arguments of one call; a bad-argument check changes one field of a good set
struct Args {
  const float *start, *end;
  uint64_t logit_stride;
  const int32_t *mask, *ttype;
  uint64_t ids_stride;
  int32_t rows, S;
  const int32_t *k_row, *len_row;
  int32_t kmax;
  int32_t* spans;
  float *scores, *null_score;
  int call() const {
    return tcamd_host_qa_spans(start, end, logit_stride, mask, ttype, ids_stride, rows, S, k_row, len_row, kmax, spans,
                               scores, null_score);
  }
};

template <typename T>
T* misaligned(T* p) {
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + 2);
}

void bad_arguments() {
  const int rows = 3, S = 16, kmax = 4;
  std::vector<float> st(rows * S, 1.0f), en(rows * S, 2.0f);
  std::vector<int32_t> mk(rows * S, 1), tt(rows * S, 1), kr(rows, 4), lr(rows, 8);
  std::vector<uint32_t> out(rows * kmax * 3 + rows + 2, kCanary);
  const Args good{st.data(), en.data(), S * 4, mk.data(), tt.data(), S * 4, rows, S, kr.data(), lr.data(), kmax,
                  reinterpret_cast<int32_t*>(out.data()), reinterpret_cast<float*>(out.data() + rows * kmax * 2),
                  reinterpret_cast<float*>(out.data() + rows * kmax * 3)};
  const auto expect = [&](const char* what, int want, Args a) {
    const int rc = a.call();
    const bool clean = std::all_of(out.begin(), out.end(), [](uint32_t w) { return w == kCanary; });
    if (rc != want || !clean) {
      std::printf("FAIL %s: returned %d, canaries %s\n", what, rc, clean ? "intact" : "overwritten");
      ++g_failures;
    }
  };
  Args a = good;
#define QA_BAD(what, field, value) \
  a = good;                        \
  a.field = value;                 \
  expect(what, 1, a)
  QA_BAD("S 0", S, 0);
  QA_BAD("S 1025", S, 1025);
  QA_BAD("kmax 0", kmax, 0);
  QA_BAD("kmax 65", kmax, 65);
  QA_BAD("rows -1", rows, -1);
  QA_BAD("logit stride no multiple of 4", logit_stride, S * 4 + 2);
  QA_BAD("logit stride below a row", logit_stride, S * 4 - 4);
  QA_BAD("ids stride no multiple of 4", ids_stride, S * 4 + 1);
  QA_BAD("ids stride below a row", ids_stride, 0);
  QA_BAD("start null", start, nullptr);
  QA_BAD("end null", end, nullptr);
  QA_BAD("mask null", mask, nullptr);
  QA_BAD("token types null", ttype, nullptr);
  QA_BAD("k_row null", k_row, nullptr);
  QA_BAD("len_row null", len_row, nullptr);
  QA_BAD("spans null", spans, nullptr);
  QA_BAD("scores null", scores, nullptr);
  QA_BAD("null_score null", null_score, nullptr);
  QA_BAD("start misaligned", start, misaligned(good.start));
  QA_BAD("end misaligned", end, misaligned(good.end));
  QA_BAD("mask misaligned", mask, misaligned(good.mask));
  QA_BAD("token types misaligned", ttype, misaligned(good.ttype));
  QA_BAD("k_row misaligned", k_row, misaligned(good.k_row));
  QA_BAD("len_row misaligned", len_row, misaligned(good.len_row));
  QA_BAD("spans misaligned", spans, misaligned(good.spans));
  QA_BAD("scores misaligned", scores, misaligned(good.scores));
  QA_BAD("null_score misaligned", null_score, misaligned(good.null_score));
#undef QA_BAD
  // rows == 0 is success and writes nothing
  a = good;
  a.rows = 0;
  expect("rows 0", 0, a);
}

}  // namespace

int main() {
  Rng rng{20240917};
  for (int S : {1, 2, 63, 64, 65, 255, 256, 257, 384, 1024}) {
    Call c{15, S, 64, -1, -1, {}, {}};
    for (int L : {1, 2, S - 1, S, S + 5})
      for (int k : {1, 20, 64}) {
        c.k_row.push_back(k);
        c.len_row.push_back(L);
      }
    run(c, rng);
  }
  for (int elig = 0; elig < 5; ++elig)
    for (int logits = 0; logits < 4; ++logits) run(Call{6, 65, 64, logits, elig, {64, 20, 1}, {30, 65, 3, 1}}, rng);
  const std::vector<int32_t> lens = {30, 39, 0, 1, 100, -4, 7, 38};
  for (int rows : {1, 5, 129}) run(Call{rows, 39, 64, -1, -1, {20, 0, 64, 3, -1, 100, 1}, lens}, rng);
  run(Call{5, 39, 7, -1, -1, {7, 0, 9, 2, 5}, lens}, rng);
  bad_arguments();
  std::printf("%d calls, %d failures\n", g_calls, g_failures);
  return g_failures ? 1 : 0;
}
