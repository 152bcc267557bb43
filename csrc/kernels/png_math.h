// The per-byte arithmetic of the PNG decode after inflate, shared by the host
// decoder (csrc/host/png.cc) and K25 png_unfilter (csrc/kernels/png.hip) so that
// the two agree bit for bit: the Paeth predictor, the five reconstruction rules,
// the sample conversion to uint8, and the layout of an image's staged bytes.
// The contract is written out in tests/png_cases.py, which implements it a
// second time in Python.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TCAMD_PNG_HD __host__ __device__ __forceinline__
#else
#define TCAMD_PNG_HD inline
#endif

namespace tcamd_png {

constexpr int kMaxDim = 16384;
constexpr int kPaletteBytes = 768;  // 256 x RGB, zero past the end of PLTE

// The decomposition of K25 (csrc/kernels/png.hip): a lane per row, kRowsPerWave
// rows per wave, kRowsPerPass rows per pass of the workgroup, and kColChunk
// units (of bpp bytes) of a row between two workgroup barriers.  The host knows
// kRowsPerPass because an image of more rows than a pass carries one row of
// scratch in its staged bytes (stage_layout).
constexpr int kRowsPerWave = 64;
constexpr int kRowsPerPass = 256;
constexpr int kColChunk = 128;

enum ColourType : int { kGrey = 0, kRgb = 2, kPalette = 3, kGreyAlpha = 4, kRgba = 6 };

// samples per pixel in the file
TCAMD_PNG_HD int file_channels(int ctype) {
  return ctype == kRgb ? 3 : ctype == kGreyAlpha ? 2 : ctype == kRgba ? 4 : 1;
}

// channels of the uint8 output: alpha is dropped, a palette gives RGB
TCAMD_PNG_HD int out_channels(int ctype) { return ctype == kGrey || ctype == kGreyAlpha ? 1 : 3; }

TCAMD_PNG_HD bool pair_ok(int ctype, int depth) {
  const bool d8 = depth == 8, d16 = depth == 16, low = depth == 1 || depth == 2 || depth == 4;
  switch (ctype) {
    case kGrey: return low || d8 || d16;
    case kPalette: return low || d8;
    case kRgb: case kGreyAlpha: case kRgba: return d8 || d16;
    default: return false;
  }
}

// the distance of the unfilter's left neighbour, and the bytes of a scanline without its filter byte
TCAMD_PNG_HD int filter_bpp(int ctype, int depth) {
  const int bits = file_channels(ctype) * depth;
  return bits < 8 ? 1 : bits / 8;
}
TCAMD_PNG_HD uint32_t row_bytes(int w, int ctype, int depth) {
  return ((uint32_t)w * (uint32_t)(file_channels(ctype) * depth) + 7u) / 8u;
}

// An image's staged bytes: h scanlines of 1 + row_bytes; for colour type 3 the
// palette, kPaletteBytes at the next 16-byte boundary; for an image of more
// than kRowsPerPass rows one row of scratch at the next 16-byte boundary, in
// which K25 hands the last row of a pass to the next pass (the host writes
// nothing there and never reads it).
struct StageLayout {
  uint64_t filtered_bytes, palette_off, line_off, stage_bytes;
};
TCAMD_PNG_HD StageLayout stage_layout(int h, int w, int ctype, int depth) {
  StageLayout s;
  const uint64_t rb = row_bytes(w, ctype, depth);
  s.filtered_bytes = (uint64_t)h * (1 + rb);
  uint64_t end = s.filtered_bytes;
  s.palette_off = s.line_off = 0;
  if (ctype == kPalette) {
    s.palette_off = (end + 15) / 16 * 16;
    end = s.palette_off + kPaletteBytes;
  }
  if (h > kRowsPerPass) {
    s.line_off = (end + 15) / 16 * 16;
    end = s.line_off + rb;
  }
  s.stage_bytes = end;
  return s;
}

// The standard's predictor: the neighbour closest to a + b - c, ties in the order a, b, c.
TCAMD_PNG_HD int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// One byte back from its filtered value x under filter type ft (0 None, 1 Sub,
// 2 Up, 3 Average, 4 Paeth): a is the byte bpp to the left, b the byte above,
// c the byte above a; each 0 where the image has none.  No branch depends on
// ft, so the lanes of a wave, which hold rows of different filters, do not diverge.
TCAMD_PNG_HD int reconstruct(int ft, int x, int a, int b, int c) {
  const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (x + pred) & 0xff;
}

// Sample k (counting from the left, most significant bits first) of a byte of depth 1, 2 or 4.
TCAMD_PNG_HD int low_sample(int byte, int depth, int k) { return (byte >> (8 - depth * (k + 1))) & ((1 << depth) - 1); }
// 255 / 85 / 17: a sample of depth 1 / 2 / 4 on the scale of 8 bits
TCAMD_PNG_HD int low_scale(int depth) { return 255 / ((1 << depth) - 1); }

// The uint8 output of one pixel of depth 8 or 16 from its reconstructed bytes
// px (file_channels * depth / 8 of them): the high byte of a 16-bit sample,
// alpha dropped, a palette index looked up in pal (kPaletteBytes).
TCAMD_PNG_HD void convert_pixel(int ctype, int depth, const uint8_t* px, const uint8_t* pal, uint8_t* out) {
  const int step = depth / 8;
  if (ctype == kPalette) {
    out[0] = pal[3 * px[0]], out[1] = pal[3 * px[0] + 1], out[2] = pal[3 * px[0] + 2];
  } else if (out_channels(ctype) == 1) {
    out[0] = px[0];
  } else {
    out[0] = px[0], out[1] = px[step], out[2] = px[2 * step];
  }
}

// The uint8 output of one sample v of depth 1, 2 or 4 (colour type 0 or 3).
TCAMD_PNG_HD void convert_low(int ctype, int depth, int v, const uint8_t* pal, uint8_t* out) {
  if (ctype == kPalette) {
    out[0] = pal[3 * v], out[1] = pal[3 * v + 1], out[2] = pal[3 * v + 2];
  } else {
    out[0] = (uint8_t)(v * low_scale(depth));
  }
}

}  // namespace tcamd_png
