// The host twin of K26 compare_expected (csrc/kernels/compare.hip): the same
// table of pairs, host pointers, the same records, by the rule both compile from
// kernels/compare_math.h.
#include "../kernels/compare_math.h"

extern "C" {

// pairs / records: n_pairs (0..64) entries.  Returns 0, or 1 for what the device
// entry refuses too: a null or misaligned pointer, an unknown dtype, a negative
// or non-finite tolerance, more than 64 pairs.
int tcamd_host_compare_expected(const TcamdComparePair* pairs, int n_pairs, double atol, double rtol,
                                TcamdCompareRecord* records) {
  using namespace tcamd_cmp;
  if (n_pairs < 0 || n_pairs > kMaxPairs || !tol_valid(atol, rtol)) return 1;
  if (n_pairs == 0) return 0;
  if (!pairs || !records) return 1;
  const Tol t = make_tol(atol, rtol);
  for (int i = 0; i < n_pairs; ++i) {
    const TcamdComparePair& q = pairs[i];
    const int kind = kind_of(q.dtype);
    if (kind == kBadKind) return 1;
    const uint64_t w = (uint64_t)kind_width(kind);
    if (q.count > (~0ull >> 4) / w) return 1;
    if (q.count && (!q.got || !q.expected)) return 1;
    if (((uintptr_t)q.got | (uintptr_t)q.expected) % w) return 1;
  }
  for (int i = 0; i < n_pairs; ++i) compare_host(pairs[i], t, records + i);
  return 0;
}

}  // extern "C"
