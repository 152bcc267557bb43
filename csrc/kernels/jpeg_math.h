// The per-sample arithmetic of the baseline JPEG decode, shared by the host
// decoder (csrc/host/jpeg.cc) and K22 jpeg_decode (csrc/kernels/jpeg.hip) so
// that the two agree bit for bit.  Integers only; the contract is written out
// in tests/jpeg_cases.py, which implements it a second time in numpy.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TCAMD_HD __host__ __device__ __forceinline__
#define TCAMD_UNROLL _Pragma("unroll")
#else
#define TCAMD_HD inline
#define TCAMD_UNROLL
#endif

namespace tcamd_jpeg {

constexpr int kDeqMin = -2048, kDeqMax = 2047;
constexpr int kC1Bits = 13, kC2Bits = 12, kPass1Bits = 2;

// round(sqrt(2) * cos(k pi / 16) * 2^BITS), k = 1..7; k = 4 is 2^BITS, the DC weight
template <int BITS>
struct IdctK;
template <>
struct IdctK<13> {
  static constexpr int c1 = 11363, c2 = 10703, c3 = 9633, c4 = 8192, c5 = 6436, c6 = 4433, c7 = 2260;
};
template <>
struct IdctK<12> {
  static constexpr int c1 = 5681, c2 = 5352, c3 = 4816, c4 = 4096, c5 = 3218, c6 = 2217, c7 = 1130;
};

TCAMD_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

TCAMD_HD int dequantise(int coef, int q) { return clampi(coef * q, kDeqMin, kDeqMax); }

// out[x] = sum_u M[u][x] * in[u] with M = round(s(u) cos((2x+1) u pi / 16) * 2^BITS), split into
// the even and odd rows (M[u][7-x] = (-1)^u M[u][x]); integer sums, so the order does not matter
template <int BITS>
TCAMD_HD void idct8(const int* in, int* out) {
  using K = IdctK<BITS>;
  const int a = K::c4 * (in[0] + in[4]), b = K::c4 * (in[0] - in[4]);
  const int p = K::c2 * in[2] + K::c6 * in[6], q = K::c6 * in[2] - K::c2 * in[6];
  const int e0 = a + p, e3 = a - p, e1 = b + q, e2 = b - q;
  const int o0 = K::c1 * in[1] + K::c3 * in[3] + K::c5 * in[5] + K::c7 * in[7];
  const int o1 = K::c3 * in[1] - K::c7 * in[3] - K::c1 * in[5] - K::c5 * in[7];
  const int o2 = K::c5 * in[1] - K::c1 * in[3] + K::c7 * in[5] + K::c3 * in[7];
  const int o3 = K::c7 * in[1] - K::c5 * in[3] + K::c3 * in[5] - K::c1 * in[7];
  out[0] = e0 + o0;
  out[7] = e0 - o0;
  out[1] = e1 + o1;
  out[6] = e1 - o1;
  out[2] = e2 + o2;
  out[5] = e2 - o2;
  out[3] = e3 + o3;
  out[4] = e3 - o3;
}

// one row of dequantised coefficients -> one row of the workspace
TCAMD_HD void idct_row(const int* v, int* ws) {
  idct8<kC1Bits>(v, ws);
  TCAMD_UNROLL
  for (int x = 0; x < 8; ++x) ws[x] = (ws[x] + (1 << (kC1Bits - kPass1Bits - 1))) >> (kC1Bits - kPass1Bits);
}

// one column of the workspace -> one column of samples, level-shifted and clamped to [0, 255]
TCAMD_HD void idct_col(const int* ws, int* s) {
  idct8<kC2Bits>(ws, s);
  TCAMD_UNROLL
  for (int y = 0; y < 8; ++y)
    s[y] = clampi(((s[y] + (1 << (kC2Bits + kPass1Bits + 2))) >> (kC2Bits + kPass1Bits + 3)) + 128, 0, 255);
}

// The chroma sample under luma pixel (X, Y) by the triangle filter.  p(cx, cy)
// reads the chroma plane; cw x ch is its valid extent, where edges replicate.
template <int HS, int VS, class F>
TCAMD_HD int chroma_up(F&& p, int X, int Y, int cw, int ch) {
  if (HS == 1) return p(X, Y);
  const int i = X >> 1, odd = X & 1;
  const int in = odd ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
  if (VS == 1) return (3 * p(i, Y) + p(in, Y) + (odd ? 2 : 1)) >> 2;
  const int j = Y >> 1;
  const int jn = (Y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
  const int r0 = 3 * p(i, j) + p(i, jn), r1 = 3 * p(in, j) + p(in, jn);
  return (3 * r0 + r1 + (odd ? 7 : 8)) >> 4;
}

// JFIF YCbCr -> RGB, 16 fractional bits
TCAMD_HD void ycc_to_rgb(int y, int cb, int cr, int* rgb) {
  cb -= 128;
  cr -= 128;
  rgb[0] = clampi(y + ((91881 * cr + 32768) >> 16), 0, 255);
  rgb[1] = clampi(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
  rgb[2] = clampi(y + ((116130 * cb + 32768) >> 16), 0, 255);
}

}  // namespace tcamd_jpeg
