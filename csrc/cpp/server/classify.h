// Host side of the KServe `classification` extension: top-K selection of an
// fp32 row, the "score:index[:label]" strings and their BYTES wire form.
//
// TopKRow orders exactly as K19 (csrc/kernels/topk.hip) and as the Python
// server's core.classify, i.e. np.argsort(-row, kind="stable")[:k]: scores
// descend, equal scores go to the lower index first, -0.0 == +0.0, +/-inf
// order as values, every NaN ranks below every number and NaNs keep index
// order.  Both sides sort the same unique 64-bit key.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace tcserve {

/// One selected class: the score's fp32 bit pattern (NaN payload included) and its index.
struct ClassPair {
  uint32_t score_bits;
  int32_t index;
};
static_assert(sizeof(ClassPair) == 8, "pairs travel as {float score; int32 index}");

inline uint64_t TopKKey(uint32_t bits, uint32_t idx)
{
  uint32_t m;
  if ((bits & 0x7fffffffu) > 0x7f800000u) {
    m = 0u;  // NaN: below -inf (whose image is 0x007fffff)
  } else {
    if (bits == 0x80000000u) bits = 0u;  // -0.0 ties with +0.0
    m = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return (static_cast<uint64_t>(m) << 32) | static_cast<uint64_t>(0xFFFFFFFFu - idx);
}

/// The min(k, C) best entries of row[0..C) into out; returns how many.
inline int64_t TopKRow(const float* row, int64_t C, int64_t k, ClassPair* out)
{
  if (C < 1 || k < 1) return 0;
  if (k > C) k = C;
  std::vector<uint64_t> keys(static_cast<size_t>(C));
  for (int64_t i = 0; i < C; ++i) {
    uint32_t bits;
    memcpy(&bits, row + i, 4);
    keys[i] = TopKKey(bits, static_cast<uint32_t>(i));
  }
  std::partial_sort(keys.begin(), keys.begin() + k, keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
  for (int64_t j = 0; j < k; ++j) {
    const uint32_t idx = 0xFFFFFFFFu - static_cast<uint32_t>(keys[j]);
    out[j].index = static_cast<int32_t>(idx);
    memcpy(&out[j].score_bits, row + idx, 4);
  }
  return k;
}

/// "%f:%d" plus ":label" when the index has one (Python's "%f" of the fp32
/// value widened to double; NaN prints as "nan" whatever its sign bit).
inline void FormatClass(const ClassPair& p, const std::vector<std::string>* labels, std::string* out)
{
  char buf[96];
  if ((p.score_bits & 0x7fffffffu) > 0x7f800000u) {
    snprintf(buf, sizeof(buf), "nan:%d", p.index);
  } else {
    float f;
    memcpy(&f, &p.score_bits, 4);
    snprintf(buf, sizeof(buf), "%f:%d", static_cast<double>(f), p.index);
  }
  out->append(buf);
  if (labels && p.index >= 0 && static_cast<size_t>(p.index) < labels->size()) {
    out->push_back(':');
    out->append((*labels)[p.index]);
  }
}

/// BYTES wire form of n pairs: per element a 4-byte little-endian length, then the string.
inline void SerializeClasses(const ClassPair* pairs, int64_t n, const std::vector<std::string>* labels,
                             std::string* out)
{
  std::string s;
  for (int64_t i = 0; i < n; ++i) {
    s.clear();
    FormatClass(pairs[i], labels, &s);
    const uint32_t len = static_cast<uint32_t>(s.size());
    const char le[4] = {static_cast<char>(len & 0xff), static_cast<char>((len >> 8) & 0xff),
                        static_cast<char>((len >> 16) & 0xff), static_cast<char>((len >> 24) & 0xff)};
    out->append(le, 4);
    out->append(s);
  }
}

}  // namespace tcserve
