// The host twins of K29 qa_merge (csrc/host/qa_merge.cc) and of K27 with a start
// mask (csrc/host/qa_spans.cc tcamd_host_qa_spans_masked), chained as the
// `qa_doc_spans` model chains them, as a stand-alone program meant for a
// sanitizer build too (`make asan` builds it as build-asan/bin/qa_merge_test):
//
//   qa_merge_test
//
// Every input and output is a heap block of exactly its size, so a read or a
// write past an end is an AddressSanitizer report.  Outputs start as a canary
// and are compared whole with a reference written out here that never builds a
// window's list: it orders every (window, s, e) candidate of a document by a
// comparator on (score, document start, length), so it also checks that the
// top k of the union lie in the union of the windows' top k.  Ranks past
// k_doc[d], skipped documents and the guard words must still hold the canary.
// Covered: 1, 2, 64 and 128 windows a document, k in 1, 20 and 64, S in 8 and
// 64, integer logits (ties within and across windows) and special values (NaN,
// both infinities, -0.0), a document without candidates, a refused document, a
// document whose rows lie outside the lists, and everything the entry refuses.
// Exits 0 when all held.

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../host/qa_merge.cc"
#include "../../host/qa_spans.cc"

namespace {

using namespace tcamd_qa;

constexpr uint32_t kCanary = 0x5A5A5A5Au;
constexpr int kGuard = 8;
int g_failures = 0;
int g_checks = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    ++g_checks;                                   \
    if (!(cond)) {                                \
      ++g_failures;                               \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
    }                                             \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

const uint32_t kSpecials[] = {0x7FC00000u, 0xFFC12345u, 0x7F800000u, 0xFF800000u, 0x80000000u, 0x00000000u, 0x3F800000u};

template <class T>
std::unique_ptr<T[]> block(size_t n, uint32_t fill) {
  std::unique_ptr<T[]> p(new T[n ? n : 1]);
  for (size_t i = 0; i < n; ++i) std::memcpy(&p[i], &fill, 4);
  return p;
}

// the order of two scores by value: NaN lowest, -0.0 == +0.0
int rank_of(uint32_t b, double* v) {
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0;
  float f;
  std::memcpy(&f, &b, 4);
  *v = f;
  return 1;
}
bool score_above(uint32_t a, uint32_t b) {
  double x = 0, y = 0;
  const int ra = rank_of(a, &x), rb = rank_of(b, &y);
  if (ra != rb) return ra > rb;
  return ra == 1 && x > y;
}
bool score_same(uint32_t a, uint32_t b) { return !score_above(a, b) && !score_above(b, a); }

struct Doc {
  int W, P;
};

// One call over documents laid out as K28w lays them: cap context pieces a window, stride apart.
void run_case(Rng* rng, const std::vector<Doc>& docs, int S, int k, int L, bool specials, const char* what) {
  const int qn = 1, first_tok = 2 + qn, cap = S - 3 - qn, stride = cap > 1 ? cap / 2 : 1;
  int rows = 0;
  for (const Doc& d : docs) rows += d.W;
  const int D = (int)docs.size() + 2, kmax = k;  // two more: a refused one, and one whose rows lie outside
  auto start = block<float>((size_t)rows * S, 0), end = block<float>((size_t)rows * S, 0);
  auto mask = block<int32_t>((size_t)rows * S, 0), tt = block<int32_t>((size_t)rows * S, 0);
  auto sm = block<int32_t>((size_t)rows * S, 0), winfo = block<int32_t>((size_t)rows * 4, 0);
  auto dinfo = block<uint32_t>((size_t)D * 4, 0);
  auto k_row = block<int32_t>(rows, 0), len_row = block<int32_t>(rows, 0), k_doc = block<int32_t>(D, 0);
  int r = 0;
  for (size_t d = 0; d < docs.size(); ++d) {
    const int W = docs[d].W, P = docs[d].P;
    dinfo[4 * d] = (uint32_t)r, dinfo[4 * d + 1] = (uint32_t)W, dinfo[4 * d + 2] = (uint32_t)P, dinfo[4 * d + 3] = 0;
    k_doc[d] = k;
    for (int w = 0; w < W; ++w, ++r) {
      const int st = w * stride, len = std::min(cap, P - st);
      winfo[4 * r] = (int32_t)d, winfo[4 * r + 1] = st, winfo[4 * r + 2] = len, winfo[4 * r + 3] = first_tok;
      k_row[r] = k, len_row[r] = L;
      for (int i = 0; i < S; ++i) {
        uint32_t a = 0, b = 0;
        float fa = (float)(rng->below(7) - 3), fb = (float)(rng->below(7) - 3);
        std::memcpy(&a, &fa, 4), std::memcpy(&b, &fb, 4);
        if (specials && rng->below(6) == 0) a = kSpecials[rng->below(7)];
        if (specials && rng->below(6) == 0) b = kSpecials[rng->below(7)];
        std::memcpy(&start[(size_t)r * S + i], &a, 4), std::memcpy(&end[(size_t)r * S + i], &b, 4);
        mask[(size_t)r * S + i] = i < first_tok + len + 1;
        const bool ctx = i >= first_tok && i < first_tok + len;
        tt[(size_t)r * S + i] = ctx;
        // piece p is owned by the window whose first stride pieces hold it, the last window owning its
        // whole tail: any rule that gives each piece one owner among the windows holding it will do here
        if (ctx) {
          const int p = st + i - first_tok;
          const int owner = std::min(p / stride, W - 1);
          sm[(size_t)r * S + i] = owner == w;
        }
      }
    }
  }
  const size_t refused = docs.size(), outside = docs.size() + 1;
  dinfo[4 * refused] = 0, dinfo[4 * refused + 1] = 3, dinfo[4 * refused + 2] = 99, dinfo[4 * refused + 3] = 6;
  dinfo[4 * outside] = (uint32_t)rows, dinfo[4 * outside + 1] = 1, dinfo[4 * outside + 2] = 1, dinfo[4 * outside + 3] = 0;
  k_doc[refused] = k, k_doc[outside] = k;
  if (D > 3) k_doc[1] = 0;  // a skipped document

  auto l_spans = block<int32_t>((size_t)rows * kmax * 2, kCanary);
  auto l_scores = block<float>((size_t)rows * kmax, kCanary);
  auto l_null = block<float>((size_t)rows, kCanary);
  CHECK(tcamd_host_qa_spans_masked(start.get(), end.get(), (uint64_t)S * 4, mask.get(), tt.get(), sm.get(),
                                   (uint64_t)S * 4, rows, S, k_row.get(), len_row.get(), kmax, l_spans.get(),
                                   l_scores.get(), l_null.get()) == 0,
        "%s: qa_spans_masked refused", what);
  auto o_spans = block<int32_t>((size_t)D * kmax * 2 + kGuard, kCanary);
  auto o_windows = block<int32_t>((size_t)D * kmax + kGuard, kCanary);
  auto o_scores = block<float>((size_t)D * kmax + kGuard, kCanary);
  auto o_null = block<float>((size_t)D + kGuard, kCanary);
  CHECK(tcamd_host_qa_merge(l_spans.get(), l_scores.get(), l_null.get(), rows, winfo.get(), dinfo.get(), D, k_doc.get(),
                            kmax, o_spans.get(), o_windows.get(), o_scores.get(), o_null.get()) == 0,
        "%s: qa_merge refused", what);

  struct Cand {
    uint32_t bits;
    int doc_start, len, row, s, e;
  };
  for (int d = 0; d < D; ++d) {
    const int32_t* sp = o_spans.get() + (size_t)d * kmax * 2;
    uint32_t nb;
    std::memcpy(&nb, &o_null[d], 4);
    if (k_doc[d] < 1) {
      CHECK((uint32_t)sp[0] == kCanary && (uint32_t)o_windows[(size_t)d * kmax] == kCanary && nb == kCanary,
            "%s: a skipped document was written", what);
      continue;
    }
    std::vector<Cand> all;
    const bool has_rows = (size_t)d < docs.size();
    uint32_t want_null = kFillerBits;
    if (has_rows)
      for (uint32_t w = 0; w < dinfo[4 * d + 1]; ++w) {
        const int row = (int)dinfo[4 * d] + (int)w;
        const uint32_t* st = reinterpret_cast<const uint32_t*>(start.get()) + (size_t)row * S;
        const uint32_t* en = reinterpret_cast<const uint32_t*>(end.get()) + (size_t)row * S;
        const uint32_t n0 = score_bits(st[0], en[0]);
        if (w == 0 || score_above(want_null, n0)) want_null = n0;
        for (int s = 0; s < S; ++s)
          for (int e = s; e < S && e - s < L; ++e)
            if (tt[(size_t)row * S + s] == 1 && tt[(size_t)row * S + e] == 1 && sm[(size_t)row * S + s] >= 1)
              all.push_back({score_bits(st[s], en[e]), winfo[4 * row + 1] + s - first_tok, e - s, row, s, e});
      }
    std::sort(all.begin(), all.end(), [](const Cand& a, const Cand& b) {
      if (!score_same(a.bits, b.bits)) return score_above(a.bits, b.bits);
      if (a.doc_start != b.doc_start) return a.doc_start < b.doc_start;
      return a.len < b.len;
    });
    CHECK(score_same(nb, want_null) && (nb == want_null || (nb & 0x7fffffffu) == 0), "%s document %d: null %#x, want %#x",
          what, d, nb, want_null);
    for (int j = 0; j < k; ++j) {
      uint32_t sb;
      std::memcpy(&sb, &o_scores[(size_t)d * kmax + j], 4);
      const int win = o_windows[(size_t)d * kmax + j];
      if (j < (int)all.size()) {
        const Cand& c = all[j];
        CHECK(win == c.row && sp[2 * j] == c.s && sp[2 * j + 1] == c.e && sb == c.bits,
              "%s document %d rank %d: (%d, %d, %d) %#x, want (%d, %d, %d) %#x", what, d, j, win, sp[2 * j],
              sp[2 * j + 1], sb, c.row, c.s, c.e, c.bits);
      } else {
        CHECK(win == -1 && sp[2 * j] == -1 && sp[2 * j + 1] == -1 && sb == kFillerBits, "%s document %d rank %d: filler",
              what, d, j);
      }
    }
  }
  bool guards = true;
  for (int g = 0; g < kGuard; ++g) {
    uint32_t a, b;
    std::memcpy(&a, &o_scores[(size_t)D * kmax + g], 4), std::memcpy(&b, &o_null[(size_t)D + g], 4);
    guards = guards && (uint32_t)o_spans[(size_t)D * kmax * 2 + g] == kCanary &&
             (uint32_t)o_windows[(size_t)D * kmax + g] == kCanary && a == kCanary && b == kCanary;
  }
  CHECK(guards, "%s: a guard word changed", what);
}

void refusals() {
  auto p = block<int32_t>(64, 0);
  auto f = block<float>(64, 0);
  auto u = block<uint32_t>(64, 0);
  const auto call = [&](const int32_t* spans, int rows, int docs, int kmax, int32_t* out) {
    return tcamd_host_qa_merge(spans, f.get(), f.get(), rows, p.get(), u.get(), docs, p.get(), kmax, out, p.get(), f.get(),
                               f.get());
  };
  CHECK(call(p.get(), 1, 1, 1, p.get()) == 0, "a good call");
  CHECK(call(nullptr, 1, 1, 1, p.get()) == 1 && call(p.get(), 1, 1, 1, nullptr) == 1, "null pointers");
  CHECK(call(p.get(), -1, 1, 1, p.get()) == 1 && call(p.get(), 1, -1, 1, p.get()) == 1, "negative counts");
  CHECK(call(p.get(), 1, 1, 0, p.get()) == 1 && call(p.get(), 1, 1, 65, p.get()) == 1, "kmax out of range");
  CHECK(call(reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.get()) + 2), 1, 1, 1, p.get()) == 1,
        "a misaligned pointer");
  CHECK(tcamd_host_qa_spans_masked(f.get(), f.get(), 32, p.get(), p.get(), nullptr, 32, 1, 8, p.get(), p.get(), 1, p.get(),
                                   f.get(), f.get()) == 1,
        "a null start mask");
}

}  // namespace

int main() {
  Rng rng{29};
  for (int S : {8, 64})
    for (int k : {1, 20, 64}) {
      const int cap = S - 4, stride = cap > 1 ? cap / 2 : 1;
      std::vector<Doc> docs;
      for (int W : {1, 2, 64, 128}) docs.push_back({W, (W - 1) * stride + 1 + rng.below(cap)});
      docs.push_back({1, 0});  // no candidate at all
      char what[64];
      std::snprintf(what, sizeof what, "S %d k %d", S, k);
      run_case(&rng, docs, S, k, S == 8 ? 3 : 30, false, what);
      std::snprintf(what, sizeof what, "S %d k %d specials", S, k);
      run_case(&rng, docs, S, k, S, true, what);
    }
  refusals();
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
