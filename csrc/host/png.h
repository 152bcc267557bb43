// PNG on the host (libtcamd_host): chunk parse, inflate of the IDAT stream into
// the staged bytes K25 png_unfilter (csrc/kernels/png.hip) reads, the unfilter
// and sample conversion to uint8 HWC pixels, K25's bitwise twin, and the whole
// decode, Adam7 included.  The per-byte arithmetic and the layout of the staged
// bytes are csrc/kernels/png_math.h; the contract is written out in
// tests/png_cases.py.
#pragma once

#include <stdint.h>

extern "C" {

enum { TCAMD_PNG_OK = 0, TCAMD_PNG_UNSUPPORTED = 1, TCAMD_PNG_MALFORMED = 2 };

// h x w, bit depth, colour type and interlace method of IHDR; channels of the
// uint8 output (1 for colour types 0 and 4, 3 for 2, 3 and 6); bpp, the
// unfilter's byte distance; row_bytes of a full-width scanline without its
// filter byte; filtered_bytes, what the IDAT stream inflates to (h * (1 +
// row_bytes), or the sum over the seven Adam7 sub-images); pixel_bytes = h * w
// * channels.  The staged bytes of a non-interlaced image (stage_bytes in all,
// tcamd_png::stage_layout): the scanlines, then for colour type 3 the palette
// at palette_off, then for an image of more rows than a pass of K25 one
// scanline of scratch at line_off; an offset that is 0 means the part is absent.
struct TcamdPngInfo {
  int32_t h, w, depth, ctype, interlace, channels, bpp;
  uint32_t row_bytes;
  uint64_t filtered_bytes, pixel_bytes, palette_off, line_off, stage_bytes;
};

// Each call returns TCAMD_PNG_OK or a code with a message in msg (msg_cap bytes,
// NUL-terminated).  Nothing is read outside [blob, blob + n) and nothing is
// written outside the caller's buffer.
//
// Headers only: walks the chunks to IEND, checks the CRC of IHDR and PLTE, and
// inflates nothing.
int tcamd_host_png_parse(const uint8_t* blob, uint64_t n, TcamdPngInfo* info, char* msg, int msg_cap);
// Inflates the IDAT stream of a non-interlaced file straight into out (at least
// info.stage_bytes; cap is checked), writes the palette of colour type 3 behind
// it, and checks the CRC of every IDAT chunk, the inflated length and the h
// filter-type bytes.  An interlaced file is TCAMD_PNG_UNSUPPORTED here:
// tcamd_host_png_decode takes it.
int tcamd_host_png_inflate(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, char* msg, int msg_cap);
// K25 on the host: the staged bytes tcamd_host_png_inflate wrote for info ->
// info.pixel_bytes of uint8 HWC in out.  Returns 0, or -1 when a size does not
// fit (staged_bytes < info.stage_bytes, cap < info.pixel_bytes) or info is not
// one tcamd_host_png_parse gives for a non-interlaced file.
int tcamd_host_png_unfilter(const uint8_t* staged, uint64_t staged_bytes, const TcamdPngInfo* info, uint8_t* out,
                            uint64_t cap);
// The whole decode, either interlace method: out receives h * w * channels
// bytes, HWC (cap is checked).
int tcamd_host_png_decode(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, char* msg, int msg_cap);

}  // extern "C"
