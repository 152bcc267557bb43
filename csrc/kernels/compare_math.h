// The rule by which an output is compared with its expectation, shared by the
// host (csrc/host/compare.cc, the perf engine) and K26 compare_expected
// (csrc/kernels/compare.hip) so that the two agree on every record field.  The
// contract is written out in tests/compare_cases.py, which implements it a third
// time in numpy.
//
// Exact mode (atol == 0 and rtol == 0, and always for the integer types, BOOL
// and the FP8 types; BYTES goes in as UINT8 over its serialized bytes): an
// element passes iff its bytes are identical, so -0.0 against +0.0 fails and a
// NaN passes only against the same bits.
//
// Tolerance mode (FP16, BF16, FP32, FP64 with atol > 0 or rtol > 0): an element
// passes when its bits are equal, or both values are NaN, or both are finite and
// |got - exp| <= atol + rtol * |exp|.  FP16 and BF16 are widened to fp32 (exact)
// and everything is evaluated in fp32, FP64 in fp64, each operation rounded on
// its own: the product and the sum are never fused.  A non-finite value never
// goes through the inequality: inf fails against a finite value and against -inf.
//
// A record holds, per pair: the mismatches, the lowest mismatching element index
// (kNoIndex when there is none), the largest |got - exp| over the pairs of finite
// values of a float type (in both modes; 0 for the other types and when there is
// no such pair; fp32 differences widened to fp64), and the bits of got and exp
// at the lowest mismatching index, zero-extended (0 when there is none).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TCAMD_CMP_HD __host__ __device__ __forceinline__
#else
#define TCAMD_CMP_HD inline
#endif

// The bound's product and sum round separately, whatever the compiler's default
// for contraction is (hipcc fuses by default, numpy never does).
#if defined(__clang__)
#define TCAMD_CMP_BOUND_FN TCAMD_CMP_HD
#define TCAMD_CMP_NO_CONTRACT _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define TCAMD_CMP_BOUND_FN __attribute__((optimize("fp-contract=off"))) inline
#define TCAMD_CMP_NO_CONTRACT
#else
#define TCAMD_CMP_BOUND_FN inline
#define TCAMD_CMP_NO_CONTRACT
#endif

struct TcamdComparePair {
  const void* got;       // element-aligned, any offset
  const void* expected;  // element-aligned, any offset (need not match got's)
  uint64_t count;        // elements; 0 is legal
  int32_t dtype;         // tcamd::DType code (kernels/common.h)
  int32_t reserved;
};

struct TcamdCompareRecord {
  uint64_t mismatches;
  uint64_t first_index;  // kNoIndex: none
  double max_abs_diff;
  uint64_t got_bits, expected_bits;  // at first_index
};

namespace tcamd_cmp {

constexpr int kMaxPairs = 64;
constexpr uint64_t kNoIndex = ~0ull;

// How the elements of a dtype are compared.
enum Kind : int { kBytes1 = 0, kBytes2, kBytes4, kBytes8, kF16, kB16, kF32, kF64, kBadKind = -1 };

// dtype codes of kernels/common.h (repeated here: the host library does not see HIP headers)
TCAMD_CMP_HD int kind_of(int dtype) {
  switch (dtype) {
    case 0: case 1: case 5: case 13: case 14: return kBytes1;  // BOOL INT8 UINT8 FP8_E4M3 FP8_E5M2
    case 2: case 6: return kBytes2;                            // INT16 UINT16
    case 3: case 7: return kBytes4;                            // INT32 UINT32
    case 4: case 8: return kBytes8;                            // INT64 UINT64
    case 9: return kF16;
    case 12: return kB16;
    case 10: return kF32;
    case 11: return kF64;
    default: return kBadKind;
  }
}

TCAMD_CMP_HD int kind_width(int kind) {
  switch (kind) {
    case kBytes1: return 1;
    case kBytes2: case kF16: case kB16: return 2;
    case kBytes4: case kF32: return 4;
    default: return 8;
  }
}

TCAMD_CMP_HD bool is_float_kind(int kind) { return kind >= kF16; }

// The tolerances of a call: what every element of a float type is held against.
struct Tol {
  bool on;  // tolerance mode
  float atol32, rtol32;
  double atol64, rtol64;
};

TCAMD_CMP_HD bool tol_valid(double atol, double rtol) {
  return atol >= 0 && rtol >= 0 && atol <= 1.7976931348623157e308 && rtol <= 1.7976931348623157e308;
}

TCAMD_CMP_HD Tol make_tol(double atol, double rtol) {
  Tol t;
  t.on = atol > 0 || rtol > 0;
  t.atol32 = (float)atol;
  t.rtol32 = (float)rtol;
  t.atol64 = atol;
  t.rtol64 = rtol;
  return t;
}

TCAMD_CMP_HD float f32_of(uint32_t b) {
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}
TCAMD_CMP_HD double f64_of(uint64_t b) {
  double f;
  __builtin_memcpy(&f, &b, 8);
  return f;
}

// fp16 bits -> fp32 bits, exact (subnormals become normal fp32 values)
TCAMD_CMP_HD uint32_t f16_to_f32_bits(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16;
  const uint32_t exp = (h >> 10) & 0x1fu;
  uint32_t man = h & 0x3ffu;
  if (exp == 0x1fu) return sign | 0x7f800000u | (man << 13);
  if (exp != 0) return sign | ((exp + 112u) << 23) | (man << 13);
  if (man == 0) return sign;
  uint32_t e = 113;  // the subnormal's leading one moves up to the implicit bit
  while (!(man & 0x400u)) {
    man <<= 1;
    --e;
  }
  return sign | (e << 23) | ((man & 0x3ffu) << 13);
}

TCAMD_CMP_BOUND_FN float bound32(float atol, float rtol, float abs_exp) {
  TCAMD_CMP_NO_CONTRACT
  const float prod = rtol * abs_exp;
  return atol + prod;
}

TCAMD_CMP_BOUND_FN double bound64(double atol, double rtol, double abs_exp) {
  TCAMD_CMP_NO_CONTRACT
  const double prod = rtol * abs_exp;
  return atol + prod;
}

// One element of FP32 (or of FP16 / BF16 widened to fp32 bits).  *diff is
// |got - exp| when both are finite, else 0.
TCAMD_CMP_HD bool pass32(uint32_t g, uint32_t e, const Tol& t, float* diff) {
  const bool gfin = (g & 0x7f800000u) != 0x7f800000u, efin = (e & 0x7f800000u) != 0x7f800000u;
  const float d = f32_of(g) - f32_of(e);
  uint32_t db;
  __builtin_memcpy(&db, &d, 4);
  *diff = gfin && efin ? f32_of(db & 0x7fffffffu) : 0.f;
  if (g == e) return true;
  if (!t.on) return false;
  if (!gfin || !efin) return (g & 0x7fffffffu) > 0x7f800000u && (e & 0x7fffffffu) > 0x7f800000u;
  return *diff <= bound32(t.atol32, t.rtol32, f32_of(e & 0x7fffffffu));
}

TCAMD_CMP_HD bool pass64(uint64_t g, uint64_t e, const Tol& t, double* diff) {
  const uint64_t em = 0x7ff0000000000000ull, am = 0x7fffffffffffffffull;
  const bool gfin = (g & em) != em, efin = (e & em) != em;
  const double d = f64_of(g) - f64_of(e);
  uint64_t db;
  __builtin_memcpy(&db, &d, 8);
  *diff = gfin && efin ? f64_of(db & am) : 0.0;
  if (g == e) return true;
  if (!t.on) return false;
  if (!gfin || !efin) return (g & am) > em && (e & am) > em;
  return *diff <= bound64(t.atol64, t.rtol64, f64_of(e & am));
}

// One element of `kind` from its zero-extended bits: does it pass, and what it
// adds to max_abs_diff (fp64; 0 for the byte kinds).
template <int KIND>
TCAMD_CMP_HD bool pass_bits(uint64_t g, uint64_t e, const Tol& t, double* diff) {
  if (KIND == kF64) return pass64(g, e, t, diff);
  if (KIND == kF32 || KIND == kF16 || KIND == kB16) {
    uint32_t g32 = (uint32_t)g, e32 = (uint32_t)e;
    if (KIND == kF16) {
      g32 = f16_to_f32_bits(g32);
      e32 = f16_to_f32_bits(e32);
    } else if (KIND == kB16) {
      g32 <<= 16;
      e32 <<= 16;
    }
    float d;
    const bool ok = pass32(g32, e32, t, &d);
    *diff = (double)d;
    return ok;
  }
  *diff = 0.0;
  return g == e;
}

// A running record: elements may be folded in any order.
TCAMD_CMP_HD void record_clear(TcamdCompareRecord* r) {
  r->mismatches = 0;
  r->first_index = kNoIndex;
  r->max_abs_diff = 0.0;
  r->got_bits = r->expected_bits = 0;
}

TCAMD_CMP_HD uint64_t load_bits(const uint8_t* p, int width) {
  uint64_t v = 0;
  for (int k = 0; k < width; ++k) v |= (uint64_t)p[k] << (8 * k);
  return v;
}

// The whole rule, one element after the other: the host's implementation, and
// what the kernel's record must equal.
template <int KIND>
inline void compare_span(const uint8_t* got, const uint8_t* exp, uint64_t count, const Tol& t, TcamdCompareRecord* r) {
  const int w = kind_width(KIND);
  record_clear(r);
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t g = load_bits(got + i * w, w), e = load_bits(exp + i * w, w);
    double d;
    if (!pass_bits<KIND>(g, e, t, &d)) {
      if (r->mismatches++ == 0) {
        r->first_index = i;
        r->got_bits = g;
        r->expected_bits = e;
      }
    }
    if (d > r->max_abs_diff) r->max_abs_diff = d;
  }
}

inline bool compare_host(const TcamdComparePair& p, const Tol& t, TcamdCompareRecord* r) {
  const uint8_t* g = static_cast<const uint8_t*>(p.got);
  const uint8_t* e = static_cast<const uint8_t*>(p.expected);
  switch (kind_of(p.dtype)) {
    case kBytes1: compare_span<kBytes1>(g, e, p.count, t, r); return true;
    case kBytes2: compare_span<kBytes2>(g, e, p.count, t, r); return true;
    case kBytes4: compare_span<kBytes4>(g, e, p.count, t, r); return true;
    case kBytes8: compare_span<kBytes8>(g, e, p.count, t, r); return true;
    case kF16: compare_span<kF16>(g, e, p.count, t, r); return true;
    case kB16: compare_span<kB16>(g, e, p.count, t, r); return true;
    case kF32: compare_span<kF32>(g, e, p.count, t, r); return true;
    case kF64: compare_span<kF64>(g, e, p.count, t, r); return true;
    default: return false;
  }
}

}  // namespace tcamd_cmp
