// The host twins of K28w wordpiece_windows (csrc/host/wordpiece.cc:
// tcamd_host_wordpiece_windows, the front-to-back walk, and
// tcamd_host_wordpiece_windows_emulate, the kernel's phases over
// kernels/wordpiece_core.h) as a stand-alone program meant for a sanitizer build
// too (`make asan` builds it as build-asan/bin/wordpiece_window_test):
//
//   wordpiece_window_test
//
// Host code only; nothing of it runs on a GPU.  The texts, the tables, the
// vocabulary image, the workspace (exactly tcamd_host_wordpiece_windows_workspace
// bytes) and every output are heap blocks of exactly their size, so a read or a
// write past an end is an AddressSanitizer report; outputs carry canary words
// behind them.  Checked: windows spelled out by hand at S = 12 (starts, lengths,
// the start mask with its tie to the lower window, the row of each window); the
// walk against the phases on random documents of up to several chunks, 1 to 128
// a call, over every stride and row capacity, with invalid documents, refused
// parameters, too many windows and a full call among them; that every context
// piece is owned by exactly one window; everything the entry refuses.
// Exits 0 when all held.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../host/wordpiece.cc"

namespace {

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
  uint32_t below(uint32_t n) { return next() % n; }
};

// The image utils/wordpiece.py builds, for pieces of ASCII: the layout of wordpiece_core.h.
std::unique_ptr<uint32_t[]> make_vocab(const std::vector<std::string>& pieces, uint64_t* words) {
  uint32_t slots = 16;
  while (slots < 2 * pieces.size()) slots *= 2;
  std::vector<uint32_t> table(slots * 4, 0), cps;
  for (uint32_t i = 0; i < slots; ++i) table[4 * i + 3] = kNone;
  uint32_t longest = 0;
  for (uint32_t id = 4; id < pieces.size(); ++id) {
    const std::string& p = pieces[id];
    const bool cont = p.size() > 2 && p[0] == '#' && p[1] == '#';
    const std::string body = cont ? p.substr(2) : p;
    uint32_t h = cont ? kHashCont : kHashFirst;
    for (unsigned char x : body) h = hash_step(h, x);
    uint32_t i = slot_of(h, slots);
    while (table[4 * i + 3] != kNone) i = (i + 1) & (slots - 1);
    table[4 * i] = h, table[4 * i + 1] = (uint32_t)cps.size();
    table[4 * i + 2] = (uint32_t)body.size() | (cont ? 0x80000000u : 0u), table[4 * i + 3] = id;
    for (unsigned char x : body) cps.push_back(x);
    if (body.size() > longest) longest = (uint32_t)body.size();
  }
  *words = kVocabHeaderWords + table.size() + cps.size();
  std::unique_ptr<uint32_t[]> v(new uint32_t[*words]);
  const uint32_t head[kVocabHeaderWords] = {kVocabMagic, (uint32_t)pieces.size(), slots, (uint32_t)kVocabHeaderWords,
                                            (uint32_t)(kVocabHeaderWords + table.size()), (uint32_t)cps.size(),
                                            (uint32_t)*words, 0, 1, 2, 3, longest};
  std::memcpy(v.get(), head, sizeof head);
  std::memcpy(v.get() + kVocabHeaderWords, table.data(), table.size() * 4);
  std::memcpy(v.get() + kVocabHeaderWords + table.size(), cps.data(), cps.size() * 4);
  return v;
}

const std::vector<std::string> kPieces = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "b", "##b", "ab", "##c", "c", "."};

struct Outputs {
  int out_rows, docs, S;
  std::unique_ptr<int32_t[]> ids, mask, tt, sm, offsets, winfo, n_rows;
  std::unique_ptr<uint32_t[]> dinfo;
  Outputs(int out_rows_, int docs_, int S_) : out_rows(out_rows_), docs(docs_), S(S_) {
    const size_t n = (size_t)out_rows * S;
    for (std::unique_ptr<int32_t[]>* a : {&ids, &mask, &tt, &sm}) fill(a, n);
    fill(&offsets, 2 * n), fill(&winfo, 4 * (size_t)out_rows), fill(&n_rows, 1);
    dinfo.reset(new uint32_t[4 * docs + kGuard]);
    for (int i = 0; i < 4 * docs + kGuard; ++i) dinfo[i] = kCanary;
  }
  static void fill(std::unique_ptr<int32_t[]>* a, size_t n) {
    a->reset(new int32_t[n + kGuard]);
    for (size_t i = 0; i < n + kGuard; ++i) (*a)[i] = (int32_t)kCanary;
  }
  bool guards_hold() const {
    const size_t n = (size_t)out_rows * S;
    for (int g = 0; g < kGuard; ++g)
      if (ids[n + g] != (int32_t)kCanary || mask[n + g] != (int32_t)kCanary || tt[n + g] != (int32_t)kCanary ||
          sm[n + g] != (int32_t)kCanary || offsets[2 * n + g] != (int32_t)kCanary ||
          winfo[4 * out_rows + g] != (int32_t)kCanary || n_rows[1 + g] != (int32_t)kCanary ||
          dinfo[4 * docs + g] != kCanary)
        return false;
    return true;
  }
  bool same(const Outputs& o) const {
    const size_t n = (size_t)out_rows * S;
    return !std::memcmp(ids.get(), o.ids.get(), n * 4) && !std::memcmp(mask.get(), o.mask.get(), n * 4) &&
           !std::memcmp(tt.get(), o.tt.get(), n * 4) && !std::memcmp(sm.get(), o.sm.get(), n * 4) &&
           !std::memcmp(offsets.get(), o.offsets.get(), n * 8) &&
           !std::memcmp(winfo.get(), o.winfo.get(), (size_t)out_rows * 16) &&
           !std::memcmp(dinfo.get(), o.dinfo.get(), (size_t)docs * 16) && n_rows[0] == o.n_rows[0];
  }
};

struct Call {
  std::unique_ptr<uint8_t[]> text;
  uint64_t text_bytes = 0;
  std::unique_ptr<uint32_t[]> table;
  std::unique_ptr<int32_t[]> maxq, stride, maxw;
  int docs = 0;
  Call(const std::vector<std::string>& qs, const std::vector<std::string>& cs, const std::vector<int>& mq,
       const std::vector<int>& ds, const std::vector<int>& mw) {
    docs = (int)qs.size();
    for (int r = 0; r < docs; ++r) text_bytes += qs[r].size() + cs[r].size();
    text.reset(new uint8_t[text_bytes ? text_bytes : 1]);
    table.reset(new uint32_t[4 * (docs ? docs : 1)]);
    maxq.reset(new int32_t[docs ? docs : 1]), stride.reset(new int32_t[docs ? docs : 1]);
    maxw.reset(new int32_t[docs ? docs : 1]);
    uint32_t at = 0;
    for (int r = 0; r < docs; ++r) {
      const std::string* f[2] = {&qs[r], &cs[r]};
      for (int k = 0; k < 2; ++k) {
        table[4 * r + 2 * k] = at, table[4 * r + 2 * k + 1] = (uint32_t)f[k]->size();
        std::memcpy(text.get() + at, f[k]->data(), f[k]->size());
        at += (uint32_t)f[k]->size();
      }
      maxq[r] = mq[r], stride[r] = ds[r], maxw[r] = mw[r];
    }
  }
  int walk(const uint32_t* vocab, uint64_t words, Outputs* o) const {
    return tcamd_host_wordpiece_windows(text.get(), text_bytes, table.get(), maxq.get(), stride.get(), maxw.get(), docs,
                                        o->S, vocab, words, o->out_rows, o->ids.get(), o->mask.get(), o->tt.get(),
                                        o->sm.get(), o->offsets.get(), o->winfo.get(), o->dinfo.get(), o->n_rows.get());
  }
  int phases(const uint32_t* vocab, uint64_t words, Outputs* o, int64_t ws_bytes = -1) const {
    const uint64_t need = ws_bytes < 0 ? tcamd_host_wordpiece_windows_workspace(docs, text_bytes) : (uint64_t)ws_bytes;
    std::unique_ptr<uint32_t[]> ws(new uint32_t[need / 4 + 1]);
    return tcamd_host_wordpiece_windows_emulate(text.get(), text_bytes, table.get(), maxq.get(), stride.get(),
                                                maxw.get(), docs, o->S, vocab, words, ws.get(), need, o->out_rows,
                                                o->ids.get(), o->mask.get(), o->tt.get(), o->sm.get(), o->offsets.get(),
                                                o->winfo.get(), o->dinfo.get(), o->n_rows.get());
  }
};

std::string letters(int n) {
  std::string s;
  for (int i = 0; i < n; ++i) s += i % 2 ? "b " : "a ";
  return s;
}

void hand_cases(const uint32_t* vocab, uint64_t words) {
  const int CLS = 2, SEP = 3, a = 4, b = 5;
  // S = 12, a question of two pieces: cap = 7.  Ten context pieces at stride 3: windows at 0 and 3, W = 2.
  Call call({"a b"}, {letters(10)}, {9}, {3}, {128});
  Outputs o(4, 1, 12), p(4, 1, 12);
  CHECK(call.walk(vocab, words, &o) == 0 && call.phases(vocab, words, &p) == 0, "hand case refused");
  CHECK(o.same(p) && o.guards_hold() && p.guards_hold(), "hand case: the walk and the phases differ");
  CHECK(o.n_rows[0] == 2 && o.dinfo[0] == 0 && o.dinfo[1] == 2 && o.dinfo[2] == 10 && o.dinfo[3] == kStOk, "doc_info");
  const int want0[12] = {CLS, a, b, SEP, a, b, a, b, a, b, a, SEP};
  const int want1[12] = {CLS, a, b, SEP, b, a, b, a, b, a, b, SEP};
  // piece k: window 0 scores 100 * min(k, 6 - k) + 7, window 1 100 * min(k - 3, 9 - k) + 7: 0..4 go to
  // window 0 (4: 207 against 107), 5 and 6 to window 1 (5: 107 against 207), as do 7..9
  const int mask0[12] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0};
  const int mask1[12] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0};
  for (int i = 0; i < 12; ++i) {
    CHECK(o.ids[i] == want0[i] && o.ids[12 + i] == want1[i], "ids[%d] = %d, %d", i, o.ids[i], o.ids[12 + i]);
    CHECK(o.sm[i] == mask0[i] && o.sm[12 + i] == mask1[i], "start_mask[%d] = %d, %d", i, o.sm[i], o.sm[12 + i]);
    CHECK(o.mask[i] == 1 && o.mask[12 + i] == 1, "mask[%d]", i);
    CHECK(o.tt[i] == (i >= 4 && i < 11) && o.tt[12 + i] == (i >= 4 && i < 11), "type[%d]", i);
  }
  CHECK(o.offsets[2 * 4] == 0 && o.offsets[2 * 4 + 1] == 1 && o.offsets[2 * (12 + 4)] == 6 &&
            o.offsets[2 * (12 + 10) + 1] == 19,
        "offsets are bytes of the whole context");
  CHECK(o.winfo[0] == 0 && o.winfo[1] == 0 && o.winfo[2] == 7 && o.winfo[3] == 4 && o.winfo[4] == 0 && o.winfo[5] == 3 &&
            o.winfo[6] == 7 && o.winfo[7] == 4,
        "window_info");
  for (int i = 24; i < 48; ++i) CHECK(o.ids[i] == 0 && o.mask[i] == 0 && o.sm[i] == 0, "rows past n_rows are zero");
  // a tie: nine pieces at stride 2 are windows at 0 and 2; piece 4 scores 100 * 2 + 7 in both and the
  // lower window keeps it, piece 5 scores 107 in window 0 and 307 in window 1
  Call tie({"a b"}, {letters(9)}, {9}, {2}, {128});
  Outputs t(2, 1, 12);
  CHECK(tie.walk(vocab, words, &t) == 0 && t.n_rows[0] == 2, "tie refused");
  CHECK(t.sm[4 + 4] == 1 && t.sm[12 + 4 + 2] == 0 && t.sm[12 + 4 + 3] == 1 && t.sm[4 + 5] == 0, "the tie goes to window 0");
  // no context piece: one window all the same
  Call none({"a"}, {"  "}, {9}, {3}, {1});
  Outputs e(1, 1, 12);
  CHECK(none.walk(vocab, words, &e) == 0 && e.n_rows[0] == 1 && e.dinfo[1] == 1 && e.dinfo[2] == 0, "P == 0");
  CHECK(e.ids[0] == CLS && e.ids[2] == SEP && e.ids[3] == SEP && e.ids[4] == 0 && e.winfo[2] == 0, "P == 0: the row");
}

void random_cases(const uint32_t* vocab, uint64_t words) {
  Rng rng{2029};
  const int doc_counts[] = {1, 2, 3, 17, 128};
  const int seqs[] = {12, 32, 384};
  for (int round = 0; round < 45; ++round) {
    const int docs = doc_counts[round % 5], S = seqs[round % 3];
    const int out_rows = round % 4 == 3 ? 1 + (int)rng.below(40) : 128;
    std::vector<std::string> qs, cs;
    std::vector<int> mq, ds, mw;
    for (int d = 0; d < docs; ++d) {
      qs.push_back(letters((int)rng.below(6)));
      std::string c = letters((int)rng.below(docs > 17 ? 30 : 1500));
      const uint32_t kind = rng.below(25);
      if (kind == 0) c.insert(rng.below((uint32_t)c.size() + 1), "\xed\xa0\x80");
      if (kind == 1) c.clear();
      if (kind == 2) c += "abc. ab.c " + std::string(101, 'a');
      cs.push_back(c);
      mq.push_back(kind == 3 ? 0 : 1 + (int)rng.below(S - 3));
      ds.push_back(kind == 4 ? (rng.below(2) ? 0 : S - 2) : 1 + (int)rng.below(S - 3));
      mw.push_back(kind == 5 ? 129 : kind < 12 ? 1 + (int)rng.below(8) : 128);
    }
    Call call(qs, cs, mq, ds, mw);
    Outputs o(out_rows, docs, S), p(out_rows, docs, S);
    CHECK(call.walk(vocab, words, &o) == 0 && call.phases(vocab, words, &p) == 0, "round %d refused", round);
    CHECK(o.guards_hold() && p.guards_hold(), "round %d: a guard word changed", round);
    CHECK(o.same(p), "round %d (%d documents, S %d): the walk and the phases differ", round, docs, S);
    int rows = 0;
    for (int d = 0; d < docs; ++d) {
      const uint32_t* di = o.dinfo.get() + 4 * d;
      if (di[3] != kStOk) continue;
      CHECK((int)di[0] == rows && di[1] >= 1 && di[1] <= (uint32_t)mw[d], "round %d document %d: rows", round, d);
      rows += (int)di[1];
      // every context piece is owned by exactly one window
      std::vector<int> owners(di[2], 0);
      for (uint32_t w = 0; w < di[1]; ++w) {
        const int32_t* wi = o.winfo.get() + 4 * (di[0] + w);
        CHECK(wi[0] == d && wi[1] + wi[2] <= (int)di[2], "round %d document %d window %u: window_info", round, d, w);
        for (int j = 0; j < wi[2]; ++j) owners[wi[1] + j] += o.sm[(size_t)(di[0] + w) * S + wi[3] + j];
      }
      bool once = true;
      for (int x : owners) once = once && x == 1;
      CHECK(once, "round %d document %d: a piece without exactly one owner", round, d);
    }
    CHECK(rows == o.n_rows[0] && rows <= out_rows, "round %d: n_rows %d, documents own %d", round, o.n_rows[0], rows);
  }
}

void refusals(const uint32_t* vocab, uint64_t words) {
  // "ab" is one piece, so cap = 8: thirty pieces at stride 3 need ceil(22 / 3) + 1 = 9 windows
  Call call({"ab", "ab"}, {"c", letters(30)}, {9, 9}, {3, 3}, {128, 8});
  Outputs o(128, 2, 12);
  CHECK(call.walk(vocab, words, &o) == 0 && o.dinfo[3] == kStOk && o.dinfo[7] == kStWindows && o.dinfo[5] == 9 &&
            o.n_rows[0] == 1,
        "one below W: %u windows, status %u", o.dinfo[5], o.dinfo[7]);
  Outputs small(128, 2, 12);
  CHECK(call.phases(vocab, words, &small, 64) == 1, "a workspace below the fixed part is refused");
  for (int bad_rows : {0, 129, -1}) {
    Outputs r(1, 2, 12);
    r.out_rows = bad_rows;
    CHECK(call.walk(vocab, words, &r) == 1 && call.phases(vocab, words, &r) == 1, "out_rows %d", bad_rows);
    r.out_rows = 1;
    CHECK(r.guards_hold() && r.ids[0] == (int32_t)kCanary, "a refused call writes nothing");
  }
  Outputs s3(128, 2, 3);
  CHECK(call.walk(vocab, words, &s3) == 1, "S out of range");
  CHECK(tcamd_host_wordpiece_windows(call.text.get(), call.text_bytes, call.table.get(), call.maxq.get(), nullptr,
                                     call.maxw.get(), 2, 12, vocab, words, 128, o.ids.get(), o.mask.get(), o.tt.get(),
                                     o.sm.get(), o.offsets.get(), o.winfo.get(), o.dinfo.get(), o.n_rows.get()) == 1,
        "a null doc_stride array");
  CHECK(tcamd_host_wordpiece_windows(call.text.get(), call.text_bytes, call.table.get(), call.maxq.get(),
                                     call.stride.get(), call.maxw.get(), 129, 12, vocab, words, 128, o.ids.get(),
                                     o.mask.get(), o.tt.get(), o.sm.get(), o.offsets.get(), o.winfo.get(), o.dinfo.get(),
                                     o.n_rows.get()) == 1,
        "129 documents");
  // a broken header: every document says so
  std::unique_ptr<uint32_t[]> bad(new uint32_t[words]);
  std::memcpy(bad.get(), vocab, words * 4);
  bad[0] = 0;
  Outputs w(128, 2, 12), e(128, 2, 12);
  CHECK(call.walk(bad.get(), words, &w) == 0 && call.phases(bad.get(), words, &e) == 0 && w.same(e), "broken header");
  CHECK(w.dinfo[3] == kStVocab && w.dinfo[7] == kStVocab && w.n_rows[0] == 0 && w.mask[0] == 0, "broken header: %#x",
        w.dinfo[3]);
}

}  // namespace

int main() {
  uint64_t words = 0;
  const std::unique_ptr<uint32_t[]> vocab = make_vocab(kPieces, &words);
  if (!tcamd_host_wordpiece_vocab_check(vocab.get(), words)) {
    std::printf("FAIL: the vocabulary image built here does not pass its own check\n");
    return 1;
  }
  hand_cases(vocab.get(), words);
  random_cases(vocab.get(), words);
  refusals(vocab.get(), words);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
