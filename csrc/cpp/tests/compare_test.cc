// The compare rule of the host library (csrc/host/compare.cc, from
// kernels/compare_math.h) as a stand-alone program meant for a sanitizer build
// (`make asan` builds it as build-asan/bin/compare_test).  No arguments.
//
// Every buffer is a heap block that ends with its last element, at every
// element-aligned start within 16 bytes, so a read past an end is an
// AddressSanitizer report.  Checked:
//   layout   widths 1, 2, 4, 8 at counts 0, 1, 15, 16, 17, 255, 256, 257, 4099 and
//            every pair of starts: a clean pair, and one flipped bit at each index
//            (at the first, middle and last when count > 64) gives exactly that index, its
//            bits, and one mismatch
//   floats   FP16, BF16, FP32 and FP64 special values in exact and in tolerance
//            mode against verdicts written out by hand below: NaNs of equal and of
//            different bits, NaN against a number, the two zeros, the infinities
//            against each other and the largest finite value, subnormals, a
//            difference at the bound (passes) and one ulp beyond it (fails)
//   refusals what the entry must return 1 for
// Exits 0 when all held, and prints the number of checks.

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../host/compare.cc"

namespace {

long g_checks = 0, g_failed = 0;

void expect(bool ok, const char* what, long a = 0, long b = 0, long c = 0) {
  ++g_checks;
  if (!ok && g_failed++ < 20) std::fprintf(stderr, "FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
}

// n elements of width w, the first `off` elements past a 16-byte boundary, the block ending with the last
struct Block {
  uint8_t* raw;
  uint8_t* p;
  Block(size_t n, int w, int off, const uint8_t* src) {
    const size_t lead = (size_t)off * w;
    void* m = nullptr;
    if (posix_memalign(&m, 16, lead + n * w + (lead + n * w == 0)) != 0) std::abort();
    raw = static_cast<uint8_t*>(m);
    p = raw + lead;
    if (n) std::memcpy(p, src, n * w);
  }
  ~Block() { std::free(raw); }
};

TcamdCompareRecord run(int dtype, const Block& g, const Block& e, uint64_t n, double atol, double rtol) {
  TcamdComparePair pr = {g.p, e.p, n, dtype, 0};
  TcamdCompareRecord r;
  std::memset(&r, 0xa5, sizeof(r));
  expect(tcamd_host_compare_expected(&pr, 1, atol, rtol, &r) == 0, "entry accepts", dtype, (long)n);
  return r;
}

void layout() {
  const int widths[] = {1, 2, 4, 8};
  const int dtypes[] = {5, 2, 3, 4};  // UINT8 INT16 INT32 INT64
  const size_t counts[] = {0, 1, 15, 16, 17, 255, 256, 257, 4099};
  for (int k = 0; k < 4; ++k) {
    const int w = widths[k];
    for (size_t n : counts) {
      std::vector<uint8_t> base(n * w + 1);
      for (size_t i = 0; i < n * w; ++i) base[i] = (uint8_t)(i * 131 + 7);
      for (int go = 0; go < 16 / w; go += (w == 1 ? 5 : 1))
        for (int eo = 0; eo < 16 / w; eo += (w == 1 ? 3 : 1)) {
          Block e(n, w, eo, base.data());
          {
            Block g(n, w, go, base.data());
            const TcamdCompareRecord r = run(dtypes[k], g, e, n, 0, 0);
            expect(r.mismatches == 0 && r.first_index == tcamd_cmp::kNoIndex && r.max_abs_diff == 0 && !r.got_bits &&
                       !r.expected_bits, "clean pair", w, (long)n, go * 16 + eo);
          }
          std::vector<size_t> at;
          if (n <= 64) for (size_t i = 0; i < n; ++i) at.push_back(i);
          else at = {0, n / 2, n - 1};
          for (size_t i : at) {
            std::vector<uint8_t> bad(base);
            bad[i * w + w - 1] ^= 0x40;
            Block g(n, w, go, bad.data());
            const TcamdCompareRecord r = run(dtypes[k], g, e, n, 0.5, 0.5);  // integers ignore the tolerance
            expect(r.mismatches == 1 && r.first_index == i && r.max_abs_diff == 0 &&
                       r.got_bits == tcamd_cmp::load_bits(bad.data() + i * w, w) &&
                       r.expected_bits == tcamd_cmp::load_bits(base.data() + i * w, w),
                   "one flipped bit", w, (long)n, (long)i);
          }
        }
    }
  }
}

struct Fmt {
  int dtype, w;
  uint64_t one, two, at, half, inf, ninf, big, nz, nan0, nan1, sub;  // at = 3.25, half = 0.5; sub: smallest subnormal
};

// bits of 1, 2, 3.25, 0.5, +inf, -inf, the largest finite value, -0, two NaNs, the smallest subnormal
const Fmt kFmts[] = {
    {9, 2, 0x3c00, 0x4000, 0x4280, 0x3800, 0x7c00, 0xfc00, 0x7bff, 0x8000, 0x7e00, 0x7e01, 0x0001},
    {12, 2, 0x3f80, 0x4000, 0x4050, 0x3f00, 0x7f80, 0xff80, 0x7f7f, 0x8000, 0x7fc0, 0x7fc1, 0x0001},
    {10, 4, 0x3f800000, 0x40000000, 0x40500000, 0x3f000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0x80000000, 0x7fc00000,
     0x7fc00001, 0x00000001},
    {11, 8, 0x3ff0000000000000ull, 0x4000000000000000ull, 0x400a000000000000ull, 0x3fe0000000000000ull,
     0x7ff0000000000000ull, 0xfff0000000000000ull, 0x7fefffffffffffffull, 0x8000000000000000ull, 0x7ff8000000000000ull,
     0x7ff8000000000001ull, 0x0000000000000001ull},
};

void floats() {
  for (const Fmt& f : kFmts) {
    // {got, expected, passes in exact mode, passes with atol 0.25 and rtol 0.5}
    const struct { uint64_t g, e; bool exact, tol; } rows[] = {
        {f.nan0, f.nan0, true, true},   {f.nan0, f.nan1, false, true},  {f.nan0, f.one, false, false},
        {f.one, f.nan0, false, false},  {0, f.nz, false, true},         {f.nz, 0, false, true},
        {f.inf, f.inf, true, true},     {f.inf, f.ninf, false, false},  {f.inf, f.big, false, false},
        {f.big, f.inf, false, false},   {f.ninf, f.ninf, true, true},   {f.at, f.two, false, true},
        {f.at + 1, f.two, false, false}, {f.at - 1, f.two, false, true}, {f.half, f.two, false, false},
        {f.sub, 0, false, true},        {f.sub | f.nz, f.sub, false, true}, {f.one, f.one, true, true},
        {f.big, f.big ^ f.nz, false, false},  // two finite values whose difference overflows (FP16: 2 * big in fp32)
    };
    const size_t n = sizeof(rows) / sizeof(rows[0]);
    std::vector<uint8_t> g(n * f.w), e(n * f.w);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(g.data() + i * f.w, &rows[i].g, f.w);  // little-endian hosts only, as the library
      std::memcpy(e.data() + i * f.w, &rows[i].e, f.w);
    }
    for (int mode = 0; mode < 2; ++mode) {
      // one at a time: the verdict, the index and the bits
      for (size_t i = 0; i < n; ++i) {
        Block bg(1, f.w, (int)(i % (16 / f.w)), g.data() + i * f.w);
        Block be(1, f.w, (int)((3 * i) % (16 / f.w)), e.data() + i * f.w);
        const TcamdCompareRecord r = run(f.dtype, bg, be, 1, mode ? 0.25 : 0, mode ? 0.5 : 0);
        const bool want = mode ? rows[i].tol : rows[i].exact;
        expect((r.mismatches == 0) == want, "float verdict", f.dtype, mode, (long)i);
        expect(want ? (r.first_index == tcamd_cmp::kNoIndex && !r.got_bits && !r.expected_bits)
                    : (r.first_index == 0 && r.got_bits == rows[i].g && r.expected_bits == rows[i].e),
               "float index and bits", f.dtype, mode, (long)i);
      }
      // all together: the count, the lowest index, the largest finite difference
      Block bg(n, f.w, 1, g.data()), be(n, f.w, 3 % (16 / f.w), e.data());
      const TcamdCompareRecord r = run(f.dtype, bg, be, n, mode ? 0.25 : 0, mode ? 0.5 : 0);
      uint64_t bad = 0, first = tcamd_cmp::kNoIndex;
      for (size_t i = 0; i < n; ++i)
        if (!(mode ? rows[i].tol : rows[i].exact)) {
          ++bad;
          if (first == tcamd_cmp::kNoIndex) first = i;
        }
      expect(r.mismatches == bad && r.first_index == first, "float count and lowest index", f.dtype, mode);
      // big - (-big) overflows to inf, but for FP16, whose largest value doubles to a finite fp32
      const double top = f.dtype == 9 ? 2 * 65504.0 : INFINITY;
      expect(r.max_abs_diff == top, "largest difference", f.dtype, mode);
    }
  }
}

void refusals() {
  uint32_t a[4] = {0, 1, 2, 3};
  TcamdCompareRecord r[2];
  TcamdComparePair ok = {a, a, 4, 10, 0};
  expect(tcamd_host_compare_expected(&ok, 1, 0, 0, r) == 0, "plain call");
  expect(tcamd_host_compare_expected(nullptr, 0, 0, 0, nullptr) == 0, "no pairs");
  expect(tcamd_host_compare_expected(&ok, 65, 0, 0, r) == 1, "too many pairs");
  expect(tcamd_host_compare_expected(&ok, 1, -1, 0, r) == 1, "negative atol");
  expect(tcamd_host_compare_expected(&ok, 1, 0, NAN, r) == 1, "NaN rtol");
  expect(tcamd_host_compare_expected(&ok, 1, INFINITY, 0, r) == 1, "infinite atol");
  TcamdComparePair bad = ok;
  bad.dtype = 15;
  expect(tcamd_host_compare_expected(&bad, 1, 0, 0, r) == 1, "unknown dtype");
  bad = ok;
  bad.got = reinterpret_cast<uint8_t*>(a) + 2;
  expect(tcamd_host_compare_expected(&bad, 1, 0, 0, r) == 1, "misaligned got");
  bad = ok;
  bad.expected = nullptr;
  expect(tcamd_host_compare_expected(&bad, 1, 0, 0, r) == 1, "null expected");
  bad.count = 0;
  expect(tcamd_host_compare_expected(&bad, 1, 0, 0, r) == 0 && r[0].first_index == tcamd_cmp::kNoIndex,
         "null is fine at count 0");
}

}  // namespace

int main() {
  layout();
  floats();
  refusals();
  std::printf("compare_test: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
