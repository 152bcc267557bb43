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

// The reduced-size decode (scale 1/2, 1/4, 1/8; contract: tests/jpeg_scaled_cases.py) keeps the
// N lowest frequencies of an axis and runs an N-point pass with the same bit widths and shifts:
// M[u][x] = round(s(u) cos((2x+1) u pi / (2N)) * 2^BITS).  sqrt(2) cos(k pi / 8) is the 8-point
// c2 (k = 1) and c6 (k = 3), and sqrt(2) cos(pi / 4) = 1 is c4, so no constant is new.
template <int N, int BITS>
TCAMD_HD void idct_n(const int* in, int* out) {
  using K = IdctK<BITS>;
  static_assert(N == 1 || N == 2 || N == 4 || N == 8, "transform size");
  if constexpr (N == 8) {
    idct8<BITS>(in, out);
  } else if constexpr (N == 4) {
    const int a = K::c4 * (in[0] + in[2]), b = K::c4 * (in[0] - in[2]);
    const int p = K::c2 * in[1] + K::c6 * in[3], q = K::c6 * in[1] - K::c2 * in[3];
    out[0] = a + p;
    out[3] = a - p;
    out[1] = b + q;
    out[2] = b - q;
  } else if constexpr (N == 2) {
    out[0] = K::c4 * (in[0] + in[1]);
    out[1] = K::c4 * (in[0] - in[1]);
  } else {
    out[0] = K::c4 * in[0];
  }
}

// idct_row / idct_col for an N-point axis
template <int N>
TCAMD_HD void idct_row_n(const int* v, int* ws) {
  idct_n<N, kC1Bits>(v, ws);
  TCAMD_UNROLL
  for (int x = 0; x < N; ++x) ws[x] = (ws[x] + (1 << (kC1Bits - kPass1Bits - 1))) >> (kC1Bits - kPass1Bits);
}

template <int N>
TCAMD_HD void idct_col_n(const int* ws, int* s) {
  idct_n<N, kC2Bits>(ws, s);
  TCAMD_UNROLL
  for (int y = 0; y < N; ++y)
    s[y] = clampi(((s[y] + (1 << (kC2Bits + kPass1Bits + 2))) >> (kC2Bits + kPass1Bits + 3)) + 128, 0, 255);
}

// The transform size of a component with sampling hc x vc under the maximum hmax x vmax at scale
// 1/s: N = 8/s samples per 8 source pixels of the component, times its subsampling, capped at 8.
// For s >= 2 every component comes out at the output resolution and nothing is upsampled.
TCAMD_HD int scaled_size(int scale, int max_sampling, int sampling) {
  const int n = 8 / scale * max_sampling / sampling;
  return n < 8 ? n : 8;
}

TCAMD_HD bool scale_ok(int scale) { return scale == 1 || scale == 2 || scale == 4 || scale == 8; }

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
