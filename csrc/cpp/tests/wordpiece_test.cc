// The host twin of K28 wordpiece (csrc/host/wordpiece.cc) and the kernel's
// phases (kernels/wordpiece_core.h, run by tcamd_host_wordpiece_emulate) as a
// stand-alone program meant for a sanitizer build too (`make asan` builds it as
// build-asan/bin/wordpiece_test):
//
//   wordpiece_test
//
// Host code only; nothing of it runs on a GPU.  The texts, the row table, the
// vocabulary image, the workspace (exactly tcamd_host_wordpiece_workspace
// bytes) and every output are heap blocks of exactly their size, so a read or a
// write past an end is an AddressSanitizer report; outputs carry canary words
// behind them.  Checked: rows spelled out by hand against a vocabulary built
// here (greedy longest match, "##" pieces, a tail without a match, a word of
// 100 and of 101, punctuation and CJK as words of their own, the cut at
// max_query_length and at the row's end, overflow, offsets in bytes); UTF-8
// decoding byte by byte against a front-to-back decoder written out here, on
// every 1- and 2-byte string and on random strings of well- and ill-formed
// sequences; the walk against the phases on random texts up to several chunks,
// 1 to 128 rows a call, with invalid and over-long rows among them; a workspace
// that is too small; a broken vocabulary header; everything the entry refuses.
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

std::string utf8(uint32_t c) {
  std::string s;
  if (c < 0x80) s += (char)c;
  else if (c < 0x800) s += (char)(0xC0 | (c >> 6)), s += (char)(0x80 | (c & 63));
  else if (c < 0x10000) s += (char)(0xE0 | (c >> 12)), s += (char)(0x80 | ((c >> 6) & 63)), s += (char)(0x80 | (c & 63));
  else
    s += (char)(0xF0 | (c >> 18)), s += (char)(0x80 | ((c >> 12) & 63)), s += (char)(0x80 | ((c >> 6) & 63)),
        s += (char)(0x80 | (c & 63));
  return s;
}

std::vector<uint32_t> code_points(const std::string& s) {
  std::vector<uint32_t> out;
  for (uint32_t i = 0; i < s.size();) {
    uint32_t c = 0, sl = 0;
    if (decode_at(reinterpret_cast<const uint8_t*>(s.data()), (uint32_t)s.size(), i, &c, &sl) != 1) std::abort();
    out.push_back(c);
    i += sl;
  }
  return out;
}

// The image utils/wordpiece.py builds, built here: the layout of wordpiece_core.h.
std::unique_ptr<uint32_t[]> make_vocab(const std::vector<std::string>& pieces, uint64_t* words) {
  uint32_t slots = 16;
  while (slots < 2 * pieces.size()) slots *= 2;
  std::vector<uint32_t> table(slots * 4, 0), cps;
  for (uint32_t i = 0; i < slots; ++i) table[4 * i + 3] = kNone;
  uint32_t special[4] = {0, 0, 0, 0}, longest = 0;
  const char* names[4] = {"[PAD]", "[UNK]", "[CLS]", "[SEP]"};
  for (uint32_t id = 0; id < pieces.size(); ++id) {
    const std::string& p = pieces[id];
    for (int k = 0; k < 4; ++k)
      if (p == names[k]) special[k] = id;
    const bool cont = p.size() > 2 && p[0] == '#' && p[1] == '#';
    const std::vector<uint32_t> c = code_points(cont ? p.substr(2) : p);
    if (c.empty()) continue;
    uint32_t h = cont ? kHashCont : kHashFirst;
    for (uint32_t x : c) h = hash_step(h, x);
    uint32_t i = slot_of(h, slots);
    while (table[4 * i + 3] != kNone) i = (i + 1) & (slots - 1);
    table[4 * i] = h, table[4 * i + 1] = (uint32_t)cps.size();
    table[4 * i + 2] = (uint32_t)c.size() | (cont ? 0x80000000u : 0u), table[4 * i + 3] = id;
    cps.insert(cps.end(), c.begin(), c.end());
    if (c.size() > longest) longest = (uint32_t)c.size();
  }
  *words = kVocabHeaderWords + table.size() + cps.size();
  std::unique_ptr<uint32_t[]> v(new uint32_t[*words]);
  const uint32_t head[kVocabHeaderWords] = {kVocabMagic, (uint32_t)pieces.size(), slots, (uint32_t)kVocabHeaderWords,
                                            (uint32_t)(kVocabHeaderWords + table.size()), (uint32_t)cps.size(),
                                            (uint32_t)*words, special[0], special[1], special[2], special[3], longest};
  std::memcpy(v.get(), head, sizeof head);
  std::memcpy(v.get() + kVocabHeaderWords, table.data(), table.size() * 4);
  if (!cps.empty()) std::memcpy(v.get() + kVocabHeaderWords + table.size(), cps.data(), cps.size() * 4);
  return v;
}

struct Outputs {
  int rows, S;
  std::unique_ptr<int32_t[]> ids, mask, tt, offsets, overflow;
  std::unique_ptr<uint32_t[]> status;
  Outputs(int rows_, int S_) : rows(rows_), S(S_) {
    const size_t n = (size_t)rows * S;
    ids.reset(new int32_t[n + kGuard]), mask.reset(new int32_t[n + kGuard]), tt.reset(new int32_t[n + kGuard]);
    offsets.reset(new int32_t[2 * n + kGuard]), overflow.reset(new int32_t[rows + kGuard]);
    status.reset(new uint32_t[rows + kGuard]);
    for (size_t i = 0; i < n + kGuard; ++i) ids[i] = mask[i] = tt[i] = (int32_t)kCanary;
    for (size_t i = 0; i < 2 * n + kGuard; ++i) offsets[i] = (int32_t)kCanary;
    for (int i = 0; i < rows + kGuard; ++i) overflow[i] = (int32_t)kCanary, status[i] = kCanary;
  }
  bool guards_hold() const {
    const size_t n = (size_t)rows * S;
    for (int g = 0; g < kGuard; ++g)
      if (ids[n + g] != (int32_t)kCanary || mask[n + g] != (int32_t)kCanary || tt[n + g] != (int32_t)kCanary ||
          offsets[2 * n + g] != (int32_t)kCanary || overflow[rows + g] != (int32_t)kCanary || status[rows + g] != kCanary)
        return false;
    return true;
  }
  bool same(const Outputs& o) const {
    const size_t n = (size_t)rows * S;
    return !std::memcmp(ids.get(), o.ids.get(), n * 4) && !std::memcmp(mask.get(), o.mask.get(), n * 4) &&
           !std::memcmp(tt.get(), o.tt.get(), n * 4) && !std::memcmp(offsets.get(), o.offsets.get(), n * 8) &&
           !std::memcmp(overflow.get(), o.overflow.get(), (size_t)rows * 4) &&
           !std::memcmp(status.get(), o.status.get(), (size_t)rows * 4);
  }
};

struct Call {
  std::unique_ptr<uint8_t[]> text;
  uint64_t text_bytes = 0;
  std::unique_ptr<uint32_t[]> table;
  std::unique_ptr<int32_t[]> maxq;
  int rows = 0;
  Call(const std::vector<std::string>& qs, const std::vector<std::string>& cs, const std::vector<int>& mq) {
    rows = (int)qs.size();
    for (int r = 0; r < rows; ++r) text_bytes += qs[r].size() + cs[r].size();
    text.reset(new uint8_t[text_bytes ? text_bytes : 1]);
    table.reset(new uint32_t[4 * (rows ? rows : 1)]);
    maxq.reset(new int32_t[rows ? rows : 1]);
    uint32_t at = 0;
    for (int r = 0; r < rows; ++r) {
      const std::string* f[2] = {&qs[r], &cs[r]};
      for (int k = 0; k < 2; ++k) {
        table[4 * r + 2 * k] = at, table[4 * r + 2 * k + 1] = (uint32_t)f[k]->size();
        std::memcpy(text.get() + at, f[k]->data(), f[k]->size());
        at += (uint32_t)f[k]->size();
      }
      maxq[r] = mq[r];
    }
  }
  int walk(const uint32_t* vocab, uint64_t words, Outputs* o, int S = 384) const {
    return tcamd_host_wordpiece_tokenize(text.get(), text_bytes, table.get(), maxq.get(), rows, S, vocab, words,
                                         o->ids.get(), o->mask.get(), o->tt.get(), o->offsets.get(), o->overflow.get(),
                                         o->status.get());
  }
  int phases(const uint32_t* vocab, uint64_t words, Outputs* o, int S = 384, int64_t ws_bytes = -1) const {
    const uint64_t need = ws_bytes < 0 ? tcamd_host_wordpiece_workspace(rows, text_bytes) : (uint64_t)ws_bytes;
    std::unique_ptr<uint32_t[]> ws(new uint32_t[need / 4 + 1]);
    return tcamd_host_wordpiece_emulate(text.get(), text_bytes, table.get(), maxq.get(), rows, S, vocab, words, ws.get(),
                                        need, o->ids.get(), o->mask.get(), o->tt.get(), o->offsets.get(),
                                        o->overflow.get(), o->status.get());
  }
};

const std::vector<std::string> kPieces = {
    "[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "b", "##b", "ab", "##c", "un", "##aff", "##able", ".", ",", "?",
    std::string(100, 'x'), "\xe4\xb8\xad" /* U+4E2D */, "e", "##e", "\xcf\x83" /* sigma */, "##\xcf\x83",
    "\xe1\x84\x92\xe1\x85\xa1" /* jamo h a */, "##\xe1\x86\xab" /* jamo n */, "c", "##a", "d"};

int id_of(const char* p) {
  for (size_t i = 0; i < kPieces.size(); ++i)
    if (kPieces[i] == p) return (int)i;
  std::abort();
}

void expect_row(const Outputs& o, int r, const std::vector<int>& ids, int first_ctx, const std::vector<int>& begins,
                const std::vector<int>& ends, int overflow, const char* what) {
  const int S = o.S;
  CHECK(o.status[r] == kStOk, "%s: status %#x", what, o.status[r]);
  for (int i = 0; i < S; ++i) {
    const int want = i < (int)ids.size() ? ids[i] : 0;
    CHECK(o.ids[r * S + i] == want, "%s: id[%d] = %d, expected %d", what, i, o.ids[r * S + i], want);
    CHECK(o.mask[r * S + i] == (i < (int)ids.size() ? 1 : 0), "%s: mask[%d]", what, i);
    const int k = i - first_ctx;
    const bool ctx = k >= 0 && k < (int)begins.size();
    CHECK(o.tt[r * S + i] == (ctx ? 1 : 0), "%s: type[%d]", what, i);
    CHECK(o.offsets[2 * (r * S + i)] == (ctx ? begins[k] : 0) && o.offsets[2 * (r * S + i) + 1] == (ctx ? ends[k] : 0),
          "%s: offsets[%d] = (%d, %d)", what, i, o.offsets[2 * (r * S + i)], o.offsets[2 * (r * S + i) + 1]);
  }
  CHECK(o.overflow[r] == overflow, "%s: overflow %d, expected %d", what, o.overflow[r], overflow);
}

void hand_cases(const uint32_t* vocab, uint64_t words) {
  const int CLS = 2, SEP = 3, UNK = 1;
  const int a = id_of("a"), b = id_of("b"), hb = id_of("##b"), ab = id_of("ab"), hc = id_of("##c"), un = id_of("un"),
            aff = id_of("##aff"), able = id_of("##able"), dot = id_of("."), q = id_of("?"), x100 = id_of(kPieces[15].c_str()),
            zh = id_of("\xe4\xb8\xad"), e = id_of("e"), sg = id_of("\xcf\x83"), hsg = id_of("##\xcf\x83"),
            ha = id_of("\xe1\x84\x92\xe1\x85\xa1"), hn = id_of("##\xe1\x86\xab"), c = id_of("c"), hA = id_of("##a");
  std::vector<std::string> qs = {
      "A b?", "", "abc", "a a a", std::string(100, 'x'), "\xce\xa3\xcf\x83" /* Sigma sigma */, "a"};
  std::vector<std::string> cs = {
      "Unaffable. abz ab",                                  // un ##aff ##able . [UNK] ab
      " \t ",                                               // nothing
      "a\xe4\xb8\xad" "b \xc3\x89 e\xcc\x81",               // a U+4E2D b, E-acute (2 bytes), e + combining acute
      "b b b b",                                            // cut by the row of S = 8
      std::string(101, 'x') + " " + std::string(100, 'x'),  // [UNK] and the piece of 100
      "\xed\x95\x9c" "a",                                   // U+D55C: three jamo from three bytes, then a
      "ca\xc2\xad" "b\xe2\x80\x8b",                         // soft hyphen and zero-width space are dropped: c ##a ##b
  };
  std::vector<int> mq = {64, 64, 64, 2, 64, 64, 64};
  Call call(qs, cs, mq);
  {
    Outputs o(call.rows, 384), p(call.rows, 384);
    CHECK(call.walk(vocab, words, &o) == 0 && call.phases(vocab, words, &p) == 0, "hand cases refused");
    CHECK(o.same(p) && o.guards_hold() && p.guards_hold(), "hand cases: the walk and the phases differ");
    expect_row(o, 0, {CLS, a, b, q, SEP, un, aff, able, dot, UNK, ab, SEP}, 5, {0, 2, 5, 9, 11, 15}, {2, 5, 9, 10, 14, 17},
               0, "row 0");
    expect_row(o, 1, {CLS, SEP, SEP}, 2, {}, {}, 0, "row 1");
    expect_row(o, 2, {CLS, ab, hc, SEP, a, zh, b, e, e, SEP}, 4, {0, 1, 4, 6, 9}, {1, 4, 5, 8, 10}, 0, "row 2");
    expect_row(o, 4, {CLS, x100, SEP, UNK, x100, SEP}, 3, {0, 102}, {101, 202}, 0, "row 4");
    expect_row(o, 5, {CLS, sg, hsg, SEP, ha, hn, hA, SEP}, 4, {0, 0, 3}, {3, 3, 4}, 0, "row 5");
    expect_row(o, 6, {CLS, a, SEP, c, hA, hb, SEP}, 3, {0, 1, 4}, {1, 2, 5}, 0, "row 6");
  }
  {
    // S = 8: [CLS] a a [SEP] b b b [SEP], one context piece left over
    std::vector<std::string> q1 = {qs[3]}, c1 = {cs[3]};
    Call one(q1, c1, {2});
    Outputs o(1, 8), p(1, 8);
    CHECK(one.walk(vocab, words, &o, 8) == 0 && one.phases(vocab, words, &p, 8) == 0, "S = 8 refused");
    CHECK(o.same(p) && o.guards_hold() && p.guards_hold(), "S = 8: the walk and the phases differ");
    expect_row(o, 0, {CLS, a, a, SEP, b, b, b, SEP}, 4, {0, 2, 4}, {1, 3, 5}, 1, "S = 8");
  }
  (void)hb;
}

// a front-to-back decoder written out again: the byte at which a text stops decoding, or -1
int64_t first_invalid(const std::string& s) {
  const size_t n = s.size();
  for (size_t i = 0; i < n;) {
    const uint32_t b = (uint8_t)s[i];
    size_t len;
    uint32_t c, lo;
    if (b < 0x80) {
      ++i;
      continue;
    } else if (b >= 0xC0 && b < 0xE0) len = 2, c = b & 0x1F, lo = 0x80;
    else if (b >= 0xE0 && b < 0xF0) len = 3, c = b & 0x0F, lo = 0x800;
    else if (b >= 0xF0 && b < 0xF8) len = 4, c = b & 0x07, lo = 0x10000;
    else return (int64_t)i;
    if (i + len > n) return (int64_t)i;
    for (size_t k = 1; k < len; ++k) {
      const uint32_t x = (uint8_t)s[i + k];
      if ((x & 0xC0) != 0x80) return (int64_t)i;
      c = (c << 6) | (x & 0x3F);
    }
    if (c < lo || c > 0x10FFFF || (c >= 0xD800 && c <= 0xDFFF)) return (int64_t)i;
    i += len;
  }
  return -1;
}

void check_status(const uint32_t* vocab, uint64_t words, const std::vector<std::string>& texts, const char* what) {
  for (size_t first = 0; first < texts.size(); first += kMaxRows) {
    const size_t n = texts.size() - first < (size_t)kMaxRows ? texts.size() - first : (size_t)kMaxRows;
    std::vector<std::string> qs(n, "a"), cs(texts.begin() + first, texts.begin() + first + n);
    Call call(qs, cs, std::vector<int>(n, 5));  // S = 16 takes a max_query_length of at most 13
    Outputs o((int)n, 16), p((int)n, 16);
    CHECK(call.walk(vocab, words, &o, 16) == 0 && call.phases(vocab, words, &p, 16) == 0, "%s refused", what);
    CHECK(o.same(p) && o.guards_hold() && p.guards_hold(), "%s: the walk and the phases differ", what);
    for (size_t r = 0; r < n; ++r) {
      const int64_t bad = first_invalid(cs[r]);
      const uint32_t want = bad < 0 ? kStOk : kStInvalid | (1u << 8) | ((uint32_t)bad << 12);
      CHECK(o.status[r] == want, "%s, text %zu: status %#x, expected %#x", what, first + r, o.status[r], want);
    }
  }
}

void utf8_cases(const uint32_t* vocab, uint64_t words) {
  std::vector<std::string> texts;
  for (int b0 = 0; b0 < 256; ++b0) texts.push_back(std::string(1, (char)b0));
  for (int b0 = 0x70; b0 < 256; b0 += 3)
    for (int b1 = 0x70; b1 < 256; b1 += 5) texts.push_back(std::string(1, (char)b0) + (char)b1);
  check_status(vocab, words, texts, "short strings");
  texts.clear();
  Rng rng{28};
  const uint32_t edge[] = {0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFD, 0xFFFF, 0x10000, 0x10FFFF, 0x4E2D, 0xD55C};
  const char* ill[] = {"\xc0\xaf", "\xe0\x80\xaf", "\xf0\x80\x80\xaf", "\xed\xa0\x80", "\xed\xbf\xbf", "\xf4\x90\x80\x80",
                       "\xf8\x88\x80\x80\x80", "\x80", "\xbf", "\xc3", "\xe2\x82", "\xf0\x9f\x98", "\xc1\xbf", "\xf5\x80",
                       "\xe2\x28\xa1", "\xf0\x28\x8c\xbc", "\xfe", "\xff"};
  for (int t = 0; t < 600; ++t) {
    std::string s;
    const int parts = 1 + (int)rng.below(12);
    for (int k = 0; k < parts; ++k) {
      const uint32_t kind = rng.below(10);
      if (kind < 5) s += (char)(0x20 + rng.below(0x5F));
      else if (kind < 8) s += utf8(edge[rng.below(sizeof edge / sizeof *edge)]);
      else if (kind < 9) s += ill[rng.below(sizeof ill / sizeof *ill)];
      else s = s.substr(0, s.size() - (s.empty() ? 0 : 1));  // cuts a sequence short now and then
    }
    texts.push_back(s);
  }
  check_status(vocab, words, texts, "random sequences");
}

std::string random_text(Rng* rng, uint32_t max_parts) {
  static const char* words[] = {"a", "b", "ab", "abc", "unaffable", "Unaff", "abz", ".", "?", ",", " ", " ", "  ", "\t",
                                "\xe4\xb8\xad", "\xed\x95\x9c", "\xce\xa3", "\xc3\x89", "e\xcc\x81", "\xc2\xad",
                                "\xe2\x80\x8b", "\xe3\x80\x80", "\xf0\x9f\x98\x80", "d", "ca"};
  std::string s;
  const uint32_t parts = rng->below(max_parts + 1);
  for (uint32_t k = 0; k < parts; ++k) {
    const uint32_t kind = rng->below(40);
    if (kind == 0) s += std::string(99 + rng->below(4), 'x');
    else s += words[rng->below(sizeof words / sizeof *words)];
  }
  return s;
}

void random_cases(const uint32_t* vocab, uint64_t words) {
  Rng rng{2028};
  const int row_counts[] = {1, 2, 3, 17, 128};
  for (int round = 0; round < 40; ++round) {
    const int rows = row_counts[round % 5];
    std::vector<std::string> qs, cs;
    std::vector<int> mq;
    for (int r = 0; r < rows; ++r) {
      qs.push_back(random_text(&rng, 20));
      // up to a few chunks; now and then an ill-formed byte, an over-long text, an empty one
      std::string c = random_text(&rng, rows > 17 ? 300 : 2500);
      const uint32_t kind = rng.below(30);
      if (kind == 0) c.insert(rng.below((uint32_t)c.size() + 1), "\xed\xa0\x80");
      if (kind == 1) c = std::string(kMaxTextBytes + 1, 'a');
      if (kind == 2) c.clear();
      if (kind == 3) c = std::string(kMaxTextBytes - 3, 'b') + "\xe4\xb8\xad";
      cs.push_back(c);
      const int choices[] = {64, 64, 1, 5, 381, 0, 382};
      mq.push_back(choices[rng.below(kind < 20 ? 5 : 7)]);
    }
    Call call(qs, cs, mq);
    Outputs o(rows, 384), p(rows, 384);
    CHECK(call.walk(vocab, words, &o) == 0 && call.phases(vocab, words, &p) == 0, "round %d refused", round);
    CHECK(o.guards_hold() && p.guards_hold(), "round %d: a guard word changed", round);
    CHECK(o.same(p), "round %d (%d rows): the walk and the phases differ", round, rows);
    for (int r = 0; r < rows; ++r) {
      const uint32_t st = o.status[r];
      const bool param = mq[r] < 1 || mq[r] > 381;
      CHECK((st == kStParam) == param, "round %d row %d: status %#x for max_query_length %d", round, r, st, mq[r]);
      if (!param) CHECK(((st & 0xff) == kStTooLong) == (cs[r].size() > kMaxTextBytes), "round %d row %d: %#x", round, r, st);
    }
  }
}

void refusals(const uint32_t* vocab, uint64_t words) {
  std::vector<std::string> qs = {"ab", "ab"}, cs = {"cd", "cd"};
  Call call(qs, cs, {64, 64});
  Outputs o(2, 384);
  // a workspace that holds the first row only: the second is refused in its status word
  CHECK(call.phases(vocab, words, &o, 384, (int64_t)tcamd_host_wordpiece_workspace(2, 6)) == 0, "short workspace");
  CHECK(o.status[0] == kStOk && (o.status[1] & 0xff) == kStRange && o.mask[384] == 0 && o.guards_hold(), "short workspace");
  CHECK(call.phases(vocab, words, &o, 384, 64) == 1, "a workspace below the fixed part is refused");
  CHECK(call.walk(vocab, words, &o, 3) == 1 && call.walk(vocab, words, &o, 1025) == 1, "S out of range");
  CHECK(call.walk(vocab, 8, &o) == 1, "an image shorter than its header");
  CHECK(tcamd_host_wordpiece_tokenize(call.text.get(), call.text_bytes, call.table.get(), call.maxq.get(), 129, 384, vocab,
                                      words, o.ids.get(), o.mask.get(), o.tt.get(), o.offsets.get(), o.overflow.get(),
                                      o.status.get()) == 1, "129 rows");
  CHECK(tcamd_host_wordpiece_tokenize(call.text.get(), call.text_bytes, nullptr, call.maxq.get(), 2, 384, vocab, words,
                                      o.ids.get(), o.mask.get(), o.tt.get(), o.offsets.get(), o.overflow.get(),
                                      o.status.get()) == 1, "a null row table");
  // a text that points outside the buffer
  call.table[3] = 100;
  Outputs r(2, 384), s(2, 384);
  CHECK(call.walk(vocab, words, &r) == 0 && call.phases(vocab, words, &s) == 0 && r.same(s), "out of range text");
  CHECK(r.status[0] == (kStRange | (1u << 8)) && r.status[1] == kStOk, "out of range text: %#x", r.status[0]);
  call.table[3] = 2;
  // a broken header: every row says so, nothing is read through it
  std::unique_ptr<uint32_t[]> bad(new uint32_t[words]);
  std::memcpy(bad.get(), vocab, words * 4);
  const uint32_t breaks[][2] = {{0, 0}, {2, 24}, {3, (uint32_t)words}, {4, (uint32_t)words + 1}, {6, (uint32_t)words - 1},
                                {8, 1u << 21}, {2, 1u << 23}};
  for (const auto& br : breaks) {
    const uint32_t keep = bad[br[0]];
    bad[br[0]] = br[1];
    CHECK(!tcamd_host_wordpiece_vocab_check(bad.get(), words), "header word %u = %u passed", br[0], br[1]);
    Outputs w(2, 384), e(2, 384);
    CHECK(call.walk(bad.get(), words, &w) == 0 && call.phases(bad.get(), words, &e) == 0 && w.same(e), "broken header");
    CHECK(w.status[0] == kStVocab && w.status[1] == kStVocab && w.mask[0] == 0, "broken header: %#x", w.status[0]);
    bad[br[0]] = keep;
  }
  CHECK(tcamd_host_wordpiece_vocab_check(bad.get(), words), "the restored header is valid");
  // slots that point outside the code points are never followed
  for (uint32_t i = 0; i < bad[2]; ++i) bad[bad[3] + 4 * i + 1] = 0xFFFFFFF0u;
  Outputs w(2, 384), e(2, 384);
  CHECK(call.walk(bad.get(), words, &w) == 0 && call.phases(bad.get(), words, &e) == 0 && w.same(e), "wild slots");
  CHECK(w.status[0] == kStOk && w.ids[1] == 1, "wild slots: every word is [UNK]");
  // zero rows
  Call none({}, {}, {});
  Outputs z(0, 384);
  CHECK(none.walk(vocab, words, &z) == 0 && none.phases(vocab, words, &z) == 0 && z.guards_hold(), "zero rows");
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
  utf8_cases(vocab.get(), words);
  random_cases(vocab.get(), words);
  refusals(vocab.get(), words);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
