// PNG on the host: see png.h.  The parser reads untrusted bytes: every offset is
// checked against the blob before it is used (csrc/cpp/tests/png_test.cc runs it
// over corrupted and truncated files under sanitizers).
#include "png.h"

#include <zlib.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../kernels/png_math.h"

using namespace tcamd_png;

namespace {

struct Error {
  int code;
};

struct Ctx {
  char* msg;
  int cap;
  [[noreturn]] void fail(int code, const char* fmt, ...) const __attribute__((format(printf, 3, 4))) {
    if (msg && cap > 0) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(msg, (size_t)cap, fmt, ap);
      va_end(ap);
    }
    throw Error{code};
  }
};

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

struct Span {
  const uint8_t* p;
  uint32_t n;
  uint32_t crc;  // as stored
  const uint8_t* type;
};

struct Parsed {
  TcamdPngInfo info;
  Span plte{nullptr, 0, 0, nullptr};
  std::vector<Span> idat;
};

const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};

void check_crc(const Ctx& cx, const Span& s, const char* name) {
  uLong c = crc32(0L, s.type, 4);
  if (s.n) c = crc32(c, s.p, s.n);
  if ((uint32_t)c != s.crc) cx.fail(TCAMD_PNG_MALFORMED, "bad CRC in %s", name);
}

// the seven Adam7 sub-images: first column and row, column and row step
const int kAdam7[7][4] = {{0, 0, 8, 8}, {4, 0, 8, 8}, {0, 4, 4, 8}, {2, 0, 4, 4}, {0, 2, 2, 4}, {1, 0, 2, 2}, {0, 1, 1, 2}};

int pass_size(int full, int first, int step) { return full > first ? (full - first + step - 1) / step : 0; }

Parsed parse(const Ctx& cx, const uint8_t* blob, uint64_t n) {
  Parsed out;
  if (!blob || n < 8 || memcmp(blob, kSignature, 8) != 0) cx.fail(TCAMD_PNG_MALFORMED, "no PNG signature");
  uint64_t pos = 8;
  bool have_ihdr = false, end = false;
  TcamdPngInfo& info = out.info;
  memset(&info, 0, sizeof info);
  while (!end) {
    if (n - pos < 12) cx.fail(TCAMD_PNG_MALFORMED, have_ihdr ? "truncated chunk" : "missing IHDR");
    Span s;
    s.n = be32(blob + pos);
    s.type = blob + pos + 4;
    if ((uint64_t)s.n > n - pos - 12) cx.fail(TCAMD_PNG_MALFORMED, "truncated chunk");
    s.p = blob + pos + 8;
    s.crc = be32(s.p + s.n);
    pos += 12 + (uint64_t)s.n;
    const bool is_ihdr = memcmp(s.type, "IHDR", 4) == 0;
    if (!have_ihdr) {
      if (!is_ihdr) cx.fail(TCAMD_PNG_MALFORMED, "missing IHDR");
      if (s.n != 13) cx.fail(TCAMD_PNG_MALFORMED, "IHDR of %u bytes", s.n);
      check_crc(cx, s, "IHDR");
      have_ihdr = true;
      const uint32_t w = be32(s.p), h = be32(s.p + 4);
      const int depth = s.p[8], ctype = s.p[9];
      if (w == 0 || h == 0) cx.fail(TCAMD_PNG_MALFORMED, "a side of 0");
      if (w > (uint32_t)kMaxDim || h > (uint32_t)kMaxDim)
        cx.fail(TCAMD_PNG_UNSUPPORTED, "%u x %u, a side above %d", w, h, kMaxDim);
      if (!pair_ok(ctype, depth)) cx.fail(TCAMD_PNG_UNSUPPORTED, "colour type %d with bit depth %d", ctype, depth);
      if (s.p[10] != 0) cx.fail(TCAMD_PNG_UNSUPPORTED, "compression method %d", s.p[10]);
      if (s.p[11] != 0) cx.fail(TCAMD_PNG_UNSUPPORTED, "filter method %d", s.p[11]);
      if (s.p[12] > 1) cx.fail(TCAMD_PNG_UNSUPPORTED, "interlace method %d", s.p[12]);
      info.h = (int32_t)h, info.w = (int32_t)w, info.depth = depth, info.ctype = ctype, info.interlace = s.p[12];
      info.channels = out_channels(ctype);
      info.bpp = filter_bpp(ctype, depth);
      info.row_bytes = row_bytes(info.w, ctype, depth);
      info.pixel_bytes = (uint64_t)h * w * (uint64_t)info.channels;
      continue;
    }
    if (is_ihdr) cx.fail(TCAMD_PNG_MALFORMED, "a second IHDR");
    if (memcmp(s.type, "PLTE", 4) == 0) {
      if (out.plte.type || !out.idat.empty()) continue;  // only a PLTE before the image data counts
      check_crc(cx, s, "PLTE");
      if (s.n == 0 || s.n % 3 || s.n > (uint32_t)kPaletteBytes) cx.fail(TCAMD_PNG_MALFORMED, "PLTE of %u bytes", s.n);
      out.plte = s;
    } else if (memcmp(s.type, "IDAT", 4) == 0) {
      out.idat.push_back(s);
    } else if (memcmp(s.type, "IEND", 4) == 0) {
      end = true;
    }
  }
  if (info.ctype == kPalette && !out.plte.type) cx.fail(TCAMD_PNG_MALFORMED, "missing PLTE");
  if (out.idat.empty()) cx.fail(TCAMD_PNG_MALFORMED, "missing IDAT");
  if (info.interlace == 0) {
    const StageLayout s = stage_layout(info.h, info.w, info.ctype, info.depth);
    info.filtered_bytes = s.filtered_bytes, info.palette_off = s.palette_off, info.line_off = s.line_off;
    info.stage_bytes = s.stage_bytes;
  } else {
    for (const auto& a : kAdam7) {
      const int pw = pass_size(info.w, a[0], a[2]), ph = pass_size(info.h, a[1], a[3]);
      if (pw && ph) info.filtered_bytes += (uint64_t)ph * (1 + row_bytes(pw, info.ctype, info.depth));
    }
    info.stage_bytes = info.filtered_bytes;
  }
  return out;
}

// the IDAT chunks, as one zlib stream, -> exactly want bytes at out
void inflate_idat(const Ctx& cx, const Parsed& p, uint8_t* out, uint64_t want) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit(&zs) != Z_OK) cx.fail(TCAMD_PNG_MALFORMED, "zlib: cannot start");
  struct Guard {
    z_stream* z;
    ~Guard() { inflateEnd(z); }
  } guard{&zs};
  uint8_t spill[64];  // where output past want would go: any of it is an error
  uint64_t left = want;
  bool done = false;
  for (const Span& s : p.idat) {
    check_crc(cx, s, "IDAT");
    zs.next_in = const_cast<uint8_t*>(s.p);
    zs.avail_in = s.n;
    while (zs.avail_in && !done) {
      const bool over = left == 0;
      const uint32_t room = over ? (uint32_t)sizeof spill : (uint32_t)(left < (1u << 30) ? left : (1u << 30));
      zs.next_out = over ? spill : out + (want - left);
      zs.avail_out = room;
      const int rc = inflate(&zs, Z_NO_FLUSH);
      const uint32_t got = room - zs.avail_out;
      if (over && got) cx.fail(TCAMD_PNG_MALFORMED, "inflated length above the %llu of the header", (unsigned long long)want);
      if (!over) left -= got;
      if (rc == Z_STREAM_END) {
        done = true;
      } else if (rc != Z_OK && !(rc == Z_BUF_ERROR && got == 0 && zs.avail_in == 0)) {
        cx.fail(TCAMD_PNG_MALFORMED, "zlib: %s", zs.msg ? zs.msg : (rc == Z_BUF_ERROR ? "no progress" : "error"));
      }
    }
  }
  if (!done) cx.fail(TCAMD_PNG_MALFORMED, "zlib: the stream ends early");
  if (left)
    cx.fail(TCAMD_PNG_MALFORMED, "inflated length %llu, not the %llu of the header", (unsigned long long)(want - left),
            (unsigned long long)want);
}

void check_filter_bytes(const Ctx& cx, const uint8_t* filt, int h, uint32_t rb, int first_row) {
  for (int y = 0; y < h; ++y) {
    const int ft = filt[(uint64_t)y * (1 + rb)];
    if (ft > 4) cx.fail(TCAMD_PNG_MALFORMED, "filter type %d in row %d", ft, first_row + y);
  }
}

void write_palette(const Span& plte, uint8_t* pal) {
  memset(pal, 0, kPaletteBytes);
  memcpy(pal, plte.p, plte.n);
}

// h x w filtered scanlines -> the pixels (x0 + x * xs, y0 + y * ys) of the uint8 HWC image of width W at out
void unfilter(const uint8_t* filt, int h, int w, int ctype, int depth, const uint8_t* pal, uint8_t* out, int W, int x0,
              int xs, int y0, int ys) {
  const uint32_t rb = row_bytes(w, ctype, depth);
  const int bpp = filter_bpp(ctype, depth), nc = out_channels(ctype);
  std::vector<uint8_t> rows(2 * (size_t)rb, 0);
  uint8_t* cur = rows.data();
  uint8_t* up = rows.data() + rb;  // zero above the first row
  for (int y = 0; y < h; ++y) {
    const uint8_t* f = filt + (uint64_t)y * (1 + rb);
    const int ft = f[0];
    for (uint32_t i = 0; i < rb; ++i) {
      const int a = i >= (uint32_t)bpp ? cur[i - bpp] : 0, c = i >= (uint32_t)bpp ? up[i - bpp] : 0;
      cur[i] = (uint8_t)reconstruct(ft, f[1 + i], a, up[i], c);
    }
    uint8_t* o = out + ((uint64_t)(y0 + y * ys) * W + x0) * nc;
    const uint64_t step = (uint64_t)xs * nc;
    if (depth >= 8) {
      for (int x = 0; x < w; ++x) convert_pixel(ctype, depth, cur + (size_t)x * bpp, pal, o + x * step);
    } else {
      for (int x = 0; x < w; ++x) {
        const int per = 8 / depth;
        convert_low(ctype, depth, low_sample(cur[x / per], depth, x % per), pal, o + x * step);
      }
    }
    uint8_t* t = cur;
    cur = up;
    up = t;
  }
}

template <class F>
int guarded(char* msg, int msg_cap, F&& body) {
  if (msg && msg_cap > 0) msg[0] = 0;
  try {
    body(Ctx{msg, msg_cap});
  } catch (const Error& e) {
    return e.code;
  } catch (const std::bad_alloc&) {
    if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "out of memory");
    return TCAMD_PNG_MALFORMED;
  }
  return TCAMD_PNG_OK;
}

}  // namespace

extern "C" {

int tcamd_host_png_parse(const uint8_t* blob, uint64_t n, TcamdPngInfo* info, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&](const Ctx& cx) {
    const Parsed p = parse(cx, blob, n);
    if (info) *info = p.info;
  });
}

int tcamd_host_png_inflate(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&](const Ctx& cx) {
    const Parsed p = parse(cx, blob, n);
    const TcamdPngInfo& info = p.info;
    if (info.interlace) cx.fail(TCAMD_PNG_UNSUPPORTED, "an interlaced file has no staged form");
    if (!out || cap < info.stage_bytes) cx.fail(TCAMD_PNG_MALFORMED, "output buffer too small");
    inflate_idat(cx, p, out, info.filtered_bytes);
    check_filter_bytes(cx, out, info.h, info.row_bytes, 0);
    if (info.palette_off) {
      memset(out + info.filtered_bytes, 0, info.palette_off - info.filtered_bytes);
      write_palette(p.plte, out + info.palette_off);
    }
  });
}

int tcamd_host_png_unfilter(const uint8_t* staged, uint64_t staged_bytes, const TcamdPngInfo* info, uint8_t* out,
                            uint64_t cap) {
  if (!staged || !info || !out || info->interlace) return -1;
  if (info->h < 1 || info->w < 1 || info->h > kMaxDim || info->w > kMaxDim || !pair_ok(info->ctype, info->depth))
    return -1;
  const StageLayout s = stage_layout(info->h, info->w, info->ctype, info->depth);
  if (s.stage_bytes != info->stage_bytes || s.palette_off != info->palette_off || staged_bytes < s.stage_bytes) return -1;
  if (cap < (uint64_t)info->h * info->w * out_channels(info->ctype)) return -1;
  try {
    unfilter(staged, info->h, info->w, info->ctype, info->depth, staged + s.palette_off, out, info->w, 0, 1, 0, 1);
  } catch (const std::bad_alloc&) {
    return -1;
  }
  return 0;
}

int tcamd_host_png_decode(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&](const Ctx& cx) {
    const Parsed p = parse(cx, blob, n);
    const TcamdPngInfo& info = p.info;
    if (!out || cap < info.pixel_bytes) cx.fail(TCAMD_PNG_MALFORMED, "output buffer too small");
    std::vector<uint8_t> filt(info.filtered_bytes);
    inflate_idat(cx, p, filt.data(), info.filtered_bytes);
    uint8_t pal[kPaletteBytes] = {0};
    if (p.plte.type) write_palette(p.plte, pal);
    if (!info.interlace) {
      check_filter_bytes(cx, filt.data(), info.h, info.row_bytes, 0);
      unfilter(filt.data(), info.h, info.w, info.ctype, info.depth, pal, out, info.w, 0, 1, 0, 1);
      return;
    }
    uint64_t at = 0;
    for (const auto& a : kAdam7) {
      const int pw = pass_size(info.w, a[0], a[2]), ph = pass_size(info.h, a[1], a[3]);
      if (!pw || !ph) continue;
      const uint32_t rb = row_bytes(pw, info.ctype, info.depth);
      check_filter_bytes(cx, filt.data() + at, ph, rb, 0);
      unfilter(filt.data() + at, ph, pw, info.ctype, info.depth, pal, out, info.w, a[0], a[2], a[1], a[3]);
      at += (uint64_t)ph * (1 + rb);
    }
  });
}

}  // extern "C"
