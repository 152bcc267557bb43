// Baseline JPEG on the host (libtcamd_host): marker parse, Huffman entropy
// decode into the coefficient buffer K22 jpeg_decode (csrc/kernels/jpeg.hip)
// reads, and the full decode to uint8 HWC pixels, K22's bitwise twin.  The
// arithmetic contract is written out in tests/jpeg_cases.py.
#pragma once

#include <stdint.h>

extern "C" {

enum { TCAMD_JPEG_OK = 0, TCAMD_JPEG_UNSUPPORTED = 1, TCAMD_JPEG_MALFORMED = 2, TCAMD_JPEG_NOT_PACKABLE = 3 };

// Coefficient buffer: uint16 q[ncomp][64] (natural order), then component c's
// blocks at coef_off[c], bw[c] x bh[c] blocks in raster order over the
// MCU-padded grid, each 64 int16 in natural order (128 bytes, 128-byte aligned
// relative to the buffer).  hs x vs is the luma sampling; chroma is 1x1.
struct TcamdJpegInfo {
  int32_t h, w, ncomp, hs, vs;
  int32_t bw[3], bh[3];
  uint64_t coef_off[3];
  uint64_t coef_bytes;  // the whole buffer, tables included
  // the reduced-size decode below; 1 and 8 x 8 from the full-size entry points
  int32_t scale;
  int32_t ny[3], nx[3];
};

// Each call returns TCAMD_JPEG_OK or a code with a message in msg (msg_cap
// bytes, NUL-terminated).  Nothing is read outside [blob, blob + n) and
// nothing is written outside the caller's buffer.
int tcamd_host_jpeg_parse(const uint8_t* blob, uint64_t n, TcamdJpegInfo* info, char* msg, int msg_cap);
// buf: at least info.coef_bytes (cap is checked).
int tcamd_host_jpeg_entropy_decode(const uint8_t* blob, uint64_t n, uint8_t* buf, uint64_t cap, char* msg, int msg_cap);
// out: h * w * ncomp bytes, HWC (cap is checked).
int tcamd_host_jpeg_decode(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, char* msg, int msg_cap);

// The reduced-size decode (contract: tests/jpeg_scaled_cases.py): scale is 1, 2,
// 4 or 8, anything else TCAMD_JPEG_UNSUPPORTED "scale ...".  info.h x info.w is
// the output, ceil(H / scale) x ceil(W / scale); component c is transformed
// with an ny[c] x nx[c] inverse DCT of its lowest frequencies (8 / scale, times
// its subsampling, at most 8), so for scale >= 2 every component comes out at
// the output resolution and none is upsampled.  The coefficient buffer is
// compact: uint16 q[ncomp][64] as above, then component c's blocks at the
// 16-byte-aligned coef_off[c], each ny[c] * nx[c] int16, vertical frequency
// major.  At scale 1 the three calls are the three above, byte for byte.  The
// entropy decoder walks the whole stream and only drops what it does not
// store: a blob fails at a scale exactly where, and as, it fails at full size.
int tcamd_host_jpeg_parse_scaled(const uint8_t* blob, uint64_t n, int scale, TcamdJpegInfo* info, char* msg,
                                 int msg_cap);
int tcamd_host_jpeg_entropy_decode_scaled(const uint8_t* blob, uint64_t n, int scale, uint8_t* buf, uint64_t cap,
                                          char* msg, int msg_cap);
int tcamd_host_jpeg_decode_scaled(const uint8_t* blob, uint64_t n, int scale, uint8_t* out, uint64_t cap, char* msg,
                                  int msg_cap);

// The entropy decode on the device, K23 jpeg_huffman (csrc/kernels/jpeg_huff.hip).
// tcamd_host_jpeg_stream_pack parses the blob (info, when not null, is its
// parse) and writes the stream buffer the kernel reads into out (16-byte
// aligned, cap bytes; *used = the bytes written): header, quantisation tables,
// Huffman lookup tables, the segment table and the scan's bytes without FF 00
// stuffing and RSTn markers (layout: csrc/kernels/jpeg_huff_core.h).  One pass
// over the blob, no Huffman work.  A parse error is the code and message of
// tcamd_host_jpeg_parse.  TCAMD_JPEG_NOT_PACKABLE is everything the pack is not
// sure about: an RSTn that is missing, misnumbered or surplus, FF fill
// followed by 00 after the scan, another scan or DNL after this one, a scan of
// more than 2048 subsequences of 128 bytes (what the kernel's workspace holds)
// or than cap, or an out that is not 16-byte aligned; the caller then takes
// tcamd_host_jpeg_entropy_decode, which gives the answer or the error.
// tcamd_host_jpeg_stream_bound(n) is a cap that fits every packable blob of n bytes.
uint64_t tcamd_host_jpeg_stream_bound(uint64_t n);
int tcamd_host_jpeg_stream_pack(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* used,
                                TcamdJpegInfo* info, char* msg, int msg_cap);
// K23 run on the host, thread by thread and phase by phase, from the same
// header as the kernel: stream (4-byte aligned) -> coef (coef_bytes of the
// parse, cap is checked; 16-byte aligned), *status = 0 or the kernel's reason
// code, *rounds = the sync rounds that decoded something.  Returns 0, or -1
// when out of memory.
int tcamd_host_jpeg_huffman_emulate(const uint8_t* stream, uint8_t* coef, uint64_t cap, uint32_t* status,
                                    uint32_t* rounds);

// The same for the K24 jpeg_huffman_wide kernels (csrc/kernels/jpeg_huff_wide.hip,
// layout and launch sequence: csrc/kernels/jpeg_huff_wide_core.h), which take a
// scan of up to 32 MiB of unstuffed data (262,144 subsequences) and write the
// compact coefficient buffer of any scale.  The pack is the one above with
// another magic word, so that neither kernel accepts the other's buffer, and
// the scale (1, 2, 4 or 8; anything else is the error of
// tcamd_host_jpeg_parse_scaled) in the header; info is the parse at that
// scale, *nsub the scan's subsequences, which size the device call's grid and
// workspace.  The rules of TCAMD_JPEG_NOT_PACKABLE are the same but for the ceiling.
uint64_t tcamd_host_jpeg_stream_bound_wide(uint64_t n);
int tcamd_host_jpeg_stream_pack_wide(const uint8_t* blob, uint64_t n, int scale, uint8_t* out, uint64_t cap,
                                     uint64_t* used, uint32_t* nsub, TcamdJpegInfo* info, char* msg, int msg_cap);
// The K24 launch sequence run on the host, launch by launch, workgroup by
// workgroup and thread by thread from the kernels' own header, with chunks of
// chunk_subs subsequences (a power of two up to 1024; 0 = 1024, the kernels'
// default; anything else is status 1).  *launches_that_changed = the
// inter-chunk launches in which a chunk took a new entry.  Returns 0, or -1
// when out of memory.
int tcamd_host_jpeg_huffman_wide_emulate(const uint8_t* stream, uint8_t* coef, uint64_t cap, uint32_t chunk_subs,
                                         uint32_t* status, uint32_t* launches_that_changed);
// The bytes of workspace a K24 call over that many subsequences and chunks
// needs: tcamd_jpeg_huffman_wide_workspace of the device library, for a
// staging plan made where that library is not loaded.
uint64_t tcamd_host_jpeg_huffman_wide_workspace(uint64_t total_subsequences, uint64_t total_chunks);

}  // extern "C"
