// Baseline JPEG on the host (libtcamd_host): marker parse, Huffman entropy
// decode into the coefficient buffer K22 jpeg_decode (csrc/kernels/jpeg.hip)
// reads, and the full decode to uint8 HWC pixels, K22's bitwise twin.  The
// arithmetic contract is written out in tests/jpeg_cases.py.
#pragma once

#include <stdint.h>

extern "C" {

enum { TCAMD_JPEG_OK = 0, TCAMD_JPEG_UNSUPPORTED = 1, TCAMD_JPEG_MALFORMED = 2 };

// Coefficient buffer: uint16 q[ncomp][64] (natural order), then component c's
// blocks at coef_off[c], bw[c] x bh[c] blocks in raster order over the
// MCU-padded grid, each 64 int16 in natural order (128 bytes, 128-byte aligned
// relative to the buffer).  hs x vs is the luma sampling; chroma is 1x1.
struct TcamdJpegInfo {
  int32_t h, w, ncomp, hs, vs;
  int32_t bw[3], bh[3];
  uint64_t coef_off[3];
  uint64_t coef_bytes;  // the whole buffer, tables included
};

// Each call returns TCAMD_JPEG_OK or a code with a message in msg (msg_cap
// bytes, NUL-terminated).  Nothing is read outside [blob, blob + n) and
// nothing is written outside the caller's buffer.
int tcamd_host_jpeg_parse(const uint8_t* blob, uint64_t n, TcamdJpegInfo* info, char* msg, int msg_cap);
// buf: at least info.coef_bytes (cap is checked).
int tcamd_host_jpeg_entropy_decode(const uint8_t* blob, uint64_t n, uint8_t* buf, uint64_t cap, char* msg, int msg_cap);
// out: h * w * ncomp bytes, HWC (cap is checked).
int tcamd_host_jpeg_decode(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, char* msg, int msg_cap);

}  // extern "C"
