// Baseline JPEG on the host: see jpeg.h.  The parser reads untrusted bytes:
// every read goes through a bounds check against the blob, every table index
// is checked before use, and the writers check the caller's capacity.
//
// Supported: SOF0 / SOF1, 8-bit, Huffman, one interleaved scan, 1 component or
// 3 (YCbCr, luma 1x1 / 2x1 / 2x2 over 1x1 chroma), DRI / RSTn, any number of
// DQT / DHT segments.  Everything else is "unsupported JPEG: <what>"; broken
// data is "malformed JPEG: <what>".

#include "jpeg.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../kernels/jpeg_huff_core.h"
#include "../kernels/jpeg_huff_wide_core.h"
#include "../kernels/jpeg_math.h"

namespace {

using namespace tcamd_jpeg;

constexpr int kMaxDim = 16384;  // RESIZE_MAX_DIM of the resize kernels that follow

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Error {
  int code;
  char what[64];
};

[[noreturn]] void bad(const char* what) {
  Error e{TCAMD_JPEG_MALFORMED, {0}};
  std::snprintf(e.what, sizeof(e.what), "%s", what);
  throw e;
}

[[noreturn]] void unsupported(const char* fmt, int v = 0) {
  Error e{TCAMD_JPEG_UNSUPPORTED, {0}};
  std::snprintf(e.what, sizeof(e.what), fmt, v);
  throw e;
}

struct Huff {
  bool defined = false;
  uint16_t look[512];  // 9 leading bits -> (length << 8) | symbol, 0 when the code is longer
  int32_t maxcode[17];  // last code of each length, -1 when the length has none
  int32_t valoff[17];   // index of the first symbol of a length minus its first code
  uint8_t vals[256];
};

struct Comp {
  int id, h, v, tq, td, ta;
};

struct Parsed {
  int h = 0, w = 0, ncomp = 0;
  Comp comp[3];
  bool have_q[4] = {false, false, false, false};
  uint16_t q[4][64];  // natural order
  Huff huff[2][4];    // [class][id]
  int dri = 0;
  size_t pos = 0;  // first entropy-coded byte
  int mcux = 0, mcuy = 0;
};

// scale 1 is the full-size layout: 8 x 8 everywhere, 128-byte blocks at multiples of 128
void fill_info(const Parsed& p, TcamdJpegInfo* info, int scale = 1) {
  std::memset(info, 0, sizeof(*info));
  info->h = (p.h + scale - 1) / scale;
  info->w = (p.w + scale - 1) / scale;
  info->ncomp = p.ncomp;
  info->hs = p.comp[0].h;
  info->vs = p.comp[0].v;
  info->scale = scale;
  uint64_t off = (uint64_t)p.ncomp * 128;
  for (int c = 0; c < p.ncomp; ++c) {
    info->bw[c] = p.mcux * p.comp[c].h;
    info->bh[c] = p.mcuy * p.comp[c].v;
    info->ny[c] = scaled_size(scale, p.comp[0].v, p.comp[c].v);
    info->nx[c] = scaled_size(scale, p.comp[0].h, p.comp[c].h);
    off = (off + 15) / 16 * 16;
    info->coef_off[c] = off;
    off += (uint64_t)info->bw[c] * info->bh[c] * info->ny[c] * info->nx[c] * 2;
  }
  info->coef_bytes = off;
}

void check_scale(int scale) {
  if (!scale_ok(scale)) unsupported("scale %d (1, 2, 4 or 8)", scale);
}

void build_huff(Huff& t, const uint8_t* counts, const uint8_t* vals, int nvals) {
  std::memset(t.look, 0, sizeof(t.look));
  std::memset(t.vals, 0, sizeof(t.vals));  // the stream pack copies the whole table
  std::memcpy(t.vals, vals, (size_t)nvals);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = counts[len - 1];
    if (code + cnt > (1 << len)) bad("DHT");
    t.valoff[len] = k - code;
    for (int i = 0; i < cnt; ++i, ++k, ++code) {
      if (len <= 9) {
        const int first = code << (9 - len);
        for (int j = 0; j < (1 << (9 - len)); ++j) t.look[first + j] = (uint16_t)((len << 8) | vals[k]);
      }
    }
    t.maxcode[len] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  t.defined = true;
}

// the markers up to the first SOS
void parse(const uint8_t* d, size_t n, Parsed& out) {
  if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) bad("no SOI");
  size_t p = 2;
  bool have_frame = false;
  int adobe = -1;
  for (;;) {
    if (p >= n) bad("truncated");
    if (d[p] != 0xFF) bad("marker expected");
    while (p < n && d[p] == 0xFF) ++p;
    if (p >= n) bad("truncated");
    const int m = d[p++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) bad("unexpected marker");
    if (m == 0xD9) bad("no scan");
    if (p + 2 > n) bad("truncated");
    const size_t len = ((size_t)d[p] << 8) | d[p + 1];
    if (len < 2 || p + len > n) bad("truncated");
    const uint8_t* seg = d + p + 2;
    const size_t sn = len - 2;
    p += len;
    if (m == 0xDB) {
      size_t s = 0;
      while (s < sn) {
        const int pq = seg[s] >> 4, tq = seg[s] & 15;
        if (pq > 1 || tq > 3 || s + 1 + 64 * (size_t)(pq + 1) > sn) bad("DQT");
        for (int k = 0; k < 64; ++k)
          out.q[tq][kZigzag[k]] = pq ? (uint16_t)((seg[s + 1 + 2 * k] << 8) | seg[s + 2 + 2 * k]) : seg[s + 1 + k];
        out.have_q[tq] = true;
        s += 1 + 64 * (size_t)(pq + 1);
      }
    } else if (m == 0xC4) {
      size_t s = 0;
      while (s < sn) {
        if (s + 17 > sn) bad("DHT");
        const int tc = seg[s] >> 4, th = seg[s] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[s + 1 + i];
        if (tc > 1 || th > 3 || total > 256 || s + 17 + (size_t)total > sn) bad("DHT");
        build_huff(out.huff[tc][th], seg + s + 1, seg + s + 17, total);
        s += 17 + (size_t)total;
      }
    } else if (m == 0xC0 || m == 0xC1) {
      if (have_frame) bad("second SOF");
      if (sn < 6) bad("SOF");
      if (seg[0] != 8) unsupported("%d-bit precision", seg[0]);
      out.h = (seg[1] << 8) | seg[2];
      out.w = (seg[3] << 8) | seg[4];
      out.ncomp = seg[5];
      if (out.h == 0) unsupported("DNL");
      if (out.w == 0) bad("zero width");
      if (out.ncomp != 1 && out.ncomp != 3) unsupported("%d components", out.ncomp);
      if (sn != 6 + 3 * (size_t)out.ncomp) bad("SOF");
      if (out.h > kMaxDim || out.w > kMaxDim) unsupported("dimension above %d", kMaxDim);
      for (int c = 0; c < out.ncomp; ++c) {
        Comp& k = out.comp[c];
        k.id = seg[6 + 3 * c];
        k.h = seg[7 + 3 * c] >> 4;
        k.v = seg[7 + 3 * c] & 15;
        k.tq = seg[8 + 3 * c];
        k.td = k.ta = 0;
      }
      if (out.ncomp == 1) {
        out.comp[0].h = out.comp[0].v = 1;  // a one-component scan is not interleaved: the factors do not matter
      } else {
        const Comp* k = out.comp;
        const bool luma = (k[0].h == 1 || k[0].h == 2) && (k[0].v == 1 || k[0].v == 2) && !(k[0].h == 1 && k[0].v == 2);
        if (!luma || k[1].h != 1 || k[1].v != 1 || k[2].h != 1 || k[2].v != 1) unsupported("sampling factors");
      }
      for (int c = 0; c < out.ncomp; ++c)
        if (out.comp[c].tq > 3) bad("SOF");
      have_frame = true;
    } else if (m >= 0xC2 && m <= 0xCF && m != 0xC8) {
      if (m == 0xC2) unsupported("progressive");
      unsupported("SOF%d", m - 0xC0);
    } else if (m == 0xDC) {
      unsupported("DNL");
    } else if (m == 0xDD) {
      if (sn != 2) bad("DRI");
      out.dri = (seg[0] << 8) | seg[1];
    } else if (m == 0xEE) {
      if (sn >= 12 && std::memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
    } else if (m == 0xDA) {
      if (!have_frame) bad("SOS before SOF");
      if (out.ncomp == 3 && adobe != -1 && adobe != 1) unsupported("Adobe colour transform %d", adobe);
      if (sn < 1 || sn != 4 + 2 * (size_t)seg[0]) bad("SOS");
      if (seg[0] != out.ncomp) unsupported("multi-scan");
      for (int c = 0; c < out.ncomp; ++c) {
        Comp& k = out.comp[c];
        if (seg[1 + 2 * c] != k.id) unsupported("scan component order");
        k.td = seg[2 + 2 * c] >> 4;
        k.ta = seg[2 + 2 * c] & 15;
        if (k.td > 3 || k.ta > 3 || !out.huff[0][k.td].defined || !out.huff[1][k.ta].defined || !out.have_q[k.tq])
          bad("undefined table");
      }
      if (seg[sn - 3] != 0 || seg[sn - 2] != 63 || seg[sn - 1] != 0) bad("SOS");
      out.pos = p;
      out.mcux = (out.w + 8 * out.comp[0].h - 1) / (8 * out.comp[0].h);
      out.mcuy = (out.h + 8 * out.comp[0].v - 1) / (8 * out.comp[0].v);
      return;
    }
    // APPn, COM and the rest carry nothing the decode needs
  }
}

// Entropy-coded bytes with the stuffing removed, MSB first.  It never reads
// past a marker or the end of the blob: asking for bits that are not there is
// an error, not zeros.
struct Bits {
  const uint8_t* d;
  size_t n, p;
  uint64_t acc = 0;
  int cnt = 0;
  bool end = false;

  Bits(const uint8_t* d_, size_t n_, size_t p_) : d(d_), n(n_), p(p_) {}

  void fill() {
    while (cnt <= 56 && !end) {
      if (p >= n) {
        end = true;
        break;
      }
      const uint8_t b = d[p];
      if (b == 0xFF) {
        if (p + 1 < n && d[p + 1] == 0) {
          p += 2;
        } else {
          end = true;
          break;
        }
      } else {
        ++p;
      }
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }

  int symbol(const Huff& t) {
    if (cnt < 16) fill();
    // the next 16 bits, zero-padded past the end
    const uint32_t v = cnt >= 16 ? (uint32_t)(acc >> (cnt - 16)) & 0xffffu : (uint32_t)(acc << (16 - cnt)) & 0xffffu;
    const uint16_t e = t.look[v >> 7];
    int len, sym;
    if (e) {
      len = e >> 8;
      sym = e & 255;
    } else {
      len = 10;
      while (len <= 16 && (int32_t)(v >> (16 - len)) > t.maxcode[len]) ++len;
      if (len > 16) bad("bad Huffman code");
      const int idx = (int)(v >> (16 - len)) + t.valoff[len];
      if (idx < 0 || idx > 255) bad("bad Huffman code");
      sym = t.vals[idx];
    }
    if (len > cnt) bad("entropy-coded data ends early");
    cnt -= len;
    return sym;
  }

  // s bits as the signed value of size category s
  int value(int s) {
    if (s == 0) return 0;
    if (cnt < s) fill();
    if (cnt < s) bad("entropy-coded data ends early");
    const int v = (int)((acc >> (cnt - s)) & ((1u << s) - 1));
    cnt -= s;
    return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
  }

  void restart(int k) {
    // what is buffered ends at the marker: in a valid stream only padding is left
    if (!end) fill();
    if (!end || cnt >= 8) bad("missing or wrong RSTn");
    cnt = 0;
    acc = 0;
    if (p >= n || d[p] != 0xFF) bad("missing or wrong RSTn");
    while (p < n && d[p] == 0xFF) ++p;
    if (p >= n || d[p] != 0xD0 + (k & 7)) bad("missing or wrong RSTn");
    ++p;
    end = false;
  }
};

void entropy_decode(const uint8_t* d, size_t n, const Parsed& P, const TcamdJpegInfo& info, uint8_t* buf) {
  uint16_t* qout = reinterpret_cast<uint16_t*>(buf);
  for (int c = 0; c < P.ncomp; ++c) std::memcpy(qout + 64 * c, P.q[P.comp[c].tq], 128);
  std::memset(buf + info.coef_off[0], 0, info.coef_bytes - info.coef_off[0]);
  // zigzag index -> where the coefficient goes in its component's ny x nx block, -1 when dropped
  int8_t slot[3][64];
  uint64_t blk_bytes[3] = {0, 0, 0};
  for (int c = 0; c < P.ncomp; ++c) {
    for (int k = 0; k < 64; ++k) {
      const int v = kZigzag[k] >> 3, u = kZigzag[k] & 7;
      slot[c][k] = v < info.ny[c] && u < info.nx[c] ? (int8_t)(v * info.nx[c] + u) : (int8_t)-1;
    }
    blk_bytes[c] = (uint64_t)info.ny[c] * info.nx[c] * 2;
  }
  Bits bits(d, n, P.pos);
  int pred[3] = {0, 0, 0};
  int rst = 0;
  const int64_t mcus = (int64_t)P.mcux * P.mcuy;
  int mx = 0, my = 0;
  for (int64_t mcu = 0; mcu < mcus; ++mcu) {
    if (P.dri && mcu && mcu % P.dri == 0) {
      bits.restart(rst++);
      pred[0] = pred[1] = pred[2] = 0;
    }
    for (int c = 0; c < P.ncomp; ++c) {
      const Comp& k = P.comp[c];
      const Huff& dc = P.huff[0][k.td];
      const Huff& ac = P.huff[1][k.ta];
      for (int by = 0; by < k.v; ++by) {
        for (int bx = 0; bx < k.h; ++bx) {
          const uint64_t blk = (uint64_t)(my * k.v + by) * info.bw[c] + (uint64_t)(mx * k.h + bx);
          int16_t* out = reinterpret_cast<int16_t*>(buf + info.coef_off[c] + blk * blk_bytes[c]);
          const int8_t* to = slot[c];
          int s = bits.symbol(dc);
          if (s > 11) bad("DC size category");
          pred[c] += bits.value(s);
          if (pred[c] < -32768 || pred[c] > 32767) bad("DC out of range");
          out[0] = (int16_t)pred[c];
          int i = 1;
          while (i < 64) {
            const int rs = bits.symbol(ac);
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;
              i += 16;
              if (i > 64) bad("run passes coefficient 63");
              continue;
            }
            if (s > 10) bad("AC size category");
            i += r;
            if (i > 63) bad("run passes coefficient 63");
            // a dropped coefficient goes to a sink: which ones are kept is not predictable at 1/2
            int16_t sink;
            int16_t* dst = to[i] >= 0 ? out + to[i] : &sink;
            *dst = (int16_t)bits.value(s);
            ++i;
          }
        }
      }
    }
    if (++mx == P.mcux) {
      mx = 0;
      ++my;
    }
  }
  // what follows the scan: another scan or DNL is refused
  for (size_t p = bits.p; p + 1 < n; ++p) {
    if (d[p] == 0xFF && d[p + 1] != 0x00 && d[p + 1] != 0xFF) {
      if (d[p + 1] == 0xDA) unsupported("multi-scan");
      if (d[p + 1] == 0xDC) unsupported("DNL");
      break;
    }
  }
}

// ---- the stream buffer of K23 jpeg_huffman (kernels/jpeg_huff_core.h) and of the K24 ----
// ---- jpeg_huffman_wide kernels (kernels/jpeg_huff_wide_core.h) ---------------------------
namespace jh = tcamd_jhuff;

struct NotPackable {};

// what the kernel that reads the buffer takes
struct PackFor {
  uint32_t magic, max_sub, max_data, scale;  // scale: the header word K23 leaves 0
};
constexpr PackFor kPackK23{jh::kMagic, (uint32_t)jh::kMaxSub, jh::kMaxDataBytes, 0};

// One linear pass over the scan: the bytes between markers are copied (memchr /
// memcpy runs), FF 00 becomes FF, every expected RSTn closes a segment.
// Anything but the plain structure throws NotPackable: the host decoder then
// gives the answer or the error.
uint64_t stream_pack(const uint8_t* d, size_t n, const Parsed& P, uint8_t* out, uint64_t cap,
                     const PackFor& lim = kPackK23) {
  // the distinct tables in order of first use
  int ids[jh::kMaxTabs];
  uint32_t ntab = 0, tabmap = 0;
  for (int c = 0; c < P.ncomp; ++c) {
    for (int cls = 0; cls < 2; ++cls) {
      const int id = cls * 4 + (cls ? P.comp[c].ta : P.comp[c].td);
      uint32_t k = 0;
      while (k < ntab && ids[k] != id) ++k;
      if (k == ntab) ids[ntab++] = id;  // at most 2 * ncomp <= kMaxTabs
      tabmap |= k << (8 * c + 4 * cls);
    }
  }
  const uint64_t mcus = (uint64_t)P.mcux * P.mcuy;
  const uint64_t interval = P.dri && (uint64_t)P.dri < mcus ? (uint64_t)P.dri : mcus;
  const uint64_t nseg = (mcus + interval - 1) / interval;
  if (nseg > (uint64_t)lim.max_sub) throw NotPackable{};
  const uint32_t data_off = jh::data_offset(ntab, (uint32_t)nseg);
  if (cap < (uint64_t)data_off + jh::kTailPad) throw NotPackable{};

  std::memset(out, 0, data_off);
  uint16_t* q = reinterpret_cast<uint16_t*>(out + jh::kQOff);
  for (int c = 0; c < P.ncomp; ++c) std::memcpy(q + 64 * c, P.q[P.comp[c].tq], 128);
  for (uint32_t k = 0; k < ntab; ++k) {
    const Huff& t = P.huff[ids[k] >> 2][ids[k] & 3];
    jh::HuffTab* o = reinterpret_cast<jh::HuffTab*>(out + jh::kTabOff) + k;
    std::memcpy(o->look, t.look, sizeof(o->look));
    std::memcpy(o->maxcode, t.maxcode, sizeof(o->maxcode));
    std::memcpy(o->valoff, t.valoff, sizeof(o->valoff));
    std::memcpy(o->vals, t.vals, sizeof(o->vals));
    o->maxcode[0] = o->valoff[0] = 0;  // never read; defined bytes all the same
  }
  jh::Segment* segs = reinterpret_cast<jh::Segment*>(out + jh::kTabOff + ntab * sizeof(jh::HuffTab));
  uint8_t* data = out + data_off;
  const uint64_t room = cap - data_off;  // every write below keeps kTailPad + 3 bytes of it free

  size_t p = P.pos;
  uint64_t o = 0, seg_start = 0;
  uint32_t k = 0, nsub = 0;
  for (;;) {
    const uint8_t* ff = p < n ? static_cast<const uint8_t*>(std::memchr(d + p, 0xFF, n - p)) : nullptr;
    const size_t run = ff ? (size_t)(ff - (d + p)) : n - p;
    if (o + run + 1 + 3 + 2 * jh::kTailPad > room) throw NotPackable{};  // does not fit
    std::memcpy(data + o, d + p, run);
    o += run;
    p += run;
    if (p + 1 < n && d[p + 1] == 0x00) {  // d[p] == 0xFF: a stuffed byte
      data[o++] = 0xFF;
      p += 2;
      continue;
    }
    // a marker, or the end of the blob: the segment is complete
    const uint64_t bytes = o - seg_start;
    if (bytes > lim.max_data) throw NotPackable{};
    segs[k].byte_off = (uint32_t)seg_start;
    segs[k].bits = (uint32_t)bytes * 8;
    segs[k].first_mcu = (uint32_t)(k * interval);
    segs[k].first_sub = nsub;
    nsub += jh::subs_of((uint32_t)bytes * 8);
    if (nsub > lim.max_sub) throw NotPackable{};  // above what the kernel's workspace holds
    while (o % 4) data[o++] = 0;
    size_t m = p;
    while (m < n && d[m] == 0xFF) ++m;
    const int marker = m < n ? d[m] : -1;
    if (k + 1 < nseg) {
      if (marker != 0xD0 + (int)(k & 7)) throw NotPackable{};  // missing or misnumbered
      p = m + 1;
      seg_start = o;
      ++k;
      continue;
    }
    // The scan is over: a surplus RSTn, another scan and DNL are the host decoder's business.  So
    // is FF fill followed by 00: the host decoder ends the data at the fill, but its look for a
    // later scan or DNL reads on past FF FF and FF 00 alike.
    if ((marker >= 0xD0 && marker <= 0xD7) || marker == 0xDA || marker == 0xDC || marker == 0x00)
      throw NotPackable{};
    break;
  }
  while (o % 16) data[o++] = 0;
  std::memset(data + o, 0, jh::kTailPad);
  o += jh::kTailPad;

  jh::StreamHeader* h = reinterpret_cast<jh::StreamHeader*>(out);
  h->magic = lim.magic;
  h->reserved = lim.scale;
  h->total_bytes = data_off + (uint32_t)o;
  h->h = P.h;
  h->w = P.w;
  h->ncomp = P.ncomp;
  h->hs = P.comp[0].h;
  h->vs = P.comp[0].v;
  h->mcux = P.mcux;
  h->mcuy = P.mcuy;
  h->interval = (uint32_t)interval;
  h->nseg = (uint32_t)nseg;
  h->nsub = nsub;
  h->ntab = ntab;
  h->tabmap = tabmap;
  h->data_bytes = (uint32_t)o;
  return h->total_bytes;
}

// K23 on the host: the phases of jpeg_huff_core.h, each run for every thread in
// turn where the kernel has a barrier.
uint32_t emulate(const uint8_t* stream, uint8_t* coef, uint64_t cap, uint32_t* rounds) {
  jh::Geo g;
  if (rounds) *rounds = 0;
  if (!jh::read_header(stream, g) || cap < g.coef_bytes) return jh::kBadHeader;
  std::vector<jh::Work> store(1);
  jh::Work& w = store[0];
  w.status = jh::kOk;
  for (uint32_t t = 0; t < (uint32_t)jh::kThreads; ++t) jh::phase_init(t, g, w, coef);
  if (w.status != jh::kOk) return w.status;
  for (uint32_t round = 0; round <= g.nsub; ++round) {
    if (round)
      for (uint32_t t = 0; t < (uint32_t)jh::kThreads; ++t) jh::phase_sync_read(t, g, w);
    bool any = false;
    for (uint32_t t = 0; t < (uint32_t)jh::kThreads; ++t) any |= jh::phase_sync_decode(t, g, w);
    if (!any) break;
    if (rounds) *rounds = round + 1;
  }
  for (uint32_t t = 0; t < (uint32_t)jh::kThreads; ++t) jh::phase_count(t, g, w);
  for (uint32_t t = 0; t < (uint32_t)jh::kThreads; ++t) jh::phase_write(t, g, w, coef);
  return w.status;
}

// The K24 launch sequence on the host (kernels/jpeg_huff_wide_core.h): launch by launch, workgroup
// by workgroup, each phase for every thread in turn where the kernels have a barrier.  A
// workgroup that a kernel leaves by a uniform early return is left the same way.  The workspace
// is a heap block of exactly the size the device call asks for.  *changed counts the inter-chunk
// launches (r >= 1) in which a chunk took a new entry.
uint32_t emulate_wide(const uint8_t* stream, uint8_t* coef, uint64_t cap, uint32_t cs, uint32_t* changed) {
  if (changed) *changed = 0;
  if (cs == 0) cs = jh::kThreads;
  jh::WideGeo wg;
  if (!jh::chunk_subs_ok(cs) || !jh::read_header_wide(stream, wg) || cap < wg.g.coef_bytes) return jh::kBadHeader;
  const jh::Geo& g = wg.g;
  const uint32_t T = jh::kThreads, nchunk = (g.nsub + cs - 1) / cs;
  std::unique_ptr<uint8_t[]> store(new uint8_t[jh::wide_ws_bytes(g.nsub, nchunk)]);
  const jh::WideWs w = jh::wide_ws_carve(store.get(), g.nsub, nchunk);
  std::vector<jh::HuffTab> tabs(jh::kMaxTabs);  // every workgroup's copy holds the same
  std::vector<jh::Acc> lds(T), next(T);
  uint32_t status = jh::kOk;
  for (uint32_t k = 0; k < nchunk; ++k) {
    const jh::Chunk c = jh::chunk_of(g, cs, k);
    for (uint32_t t = 0; t < T; ++t) jh::wide_init(t, wg, w, c, coef, &status);
  }
  if (status != jh::kOk) return status;  // the later launches return at once
  for (uint32_t t = 0; t < T; ++t) jh::wide_load_tables(t, g, tabs.data());
  for (uint32_t r = 0; r < nchunk; ++r) {
    bool took = false;
    for (uint32_t k = 0; k < nchunk; ++k) {
      const jh::Chunk c = jh::chunk_of(g, cs, k);
      if (r == 0 || jh::wide_take(w, c, r)) {
        took = true;
        for (uint32_t round = 0; round <= c.n; ++round) {
          if (round)
            for (uint32_t t = 0; t < T; ++t) jh::wide_sync_read(t, w, c);
          bool any = false;
          for (uint32_t t = 0; t < T; ++t) any |= jh::wide_sync_decode(t, g, tabs.data(), w, c);
          if (!any) break;
        }
      }
      jh::wide_publish(w, c, r);
    }
    if (r && took && changed) ++*changed;
  }
  auto scan = [&](uint32_t n) {
    for (uint32_t d = 1; d < n; d <<= 1) {
      for (uint32_t t = 0; t < T; ++t) next[t] = jh::scan_step(t, d, lds.data());
      lds.swap(next);
    }
  };
  for (uint32_t k = 0; k < nchunk; ++k) {
    const jh::Chunk c = jh::chunk_of(g, cs, k);
    for (uint32_t t = 0; t < T; ++t) lds[t] = jh::wide_count_load(t, w, c);
    scan(c.n);
    for (uint32_t t = 0; t < T; ++t) jh::wide_count_store(t, w, c, lds.data());
  }
  jh::Acc carry{0, 0, 0, 0, 0};
  for (uint32_t base = 0; base < nchunk; base += T) {
    for (uint32_t t = 0; t < T; ++t) lds[t] = jh::wide_tile_load(t, w, base, nchunk);
    scan(T);
    for (uint32_t t = 0; t < T; ++t) jh::wide_tile_store(t, w, base, nchunk, carry, lds.data());
    carry = jh::combine(carry, lds[T - 1]);
  }
  for (uint32_t k = 0; k < nchunk; ++k) {
    const jh::Chunk c = jh::chunk_of(g, cs, k);
    for (uint32_t t = 0; t < T; ++t) jh::wide_write(t, wg, tabs.data(), w, c, coef, &status);
  }
  return status;
}

// one component's blocks -> its sample plane, (bh*8) x (bw*8)
void idct_plane(const uint16_t* q, const int16_t* coef, int bw, int bh, uint8_t* plane) {
  const size_t stride = (size_t)bw * 8;
  for (int by = 0; by < bh; ++by) {
    for (int bx = 0; bx < bw; ++bx) {
      const int16_t* blk = coef + ((size_t)by * bw + bx) * 64;
      int ws[8][8];
      for (int y = 0; y < 8; ++y) {
        int v[8];
        for (int u = 0; u < 8; ++u) v[u] = dequantise(blk[y * 8 + u], q[y * 8 + u]);
        idct_row(v, ws[y]);
      }
      for (int x = 0; x < 8; ++x) {
        int col[8], s[8];
        for (int y = 0; y < 8; ++y) col[y] = ws[y][x];
        idct_col(col, s);
        for (int y = 0; y < 8; ++y) plane[((size_t)by * 8 + y) * stride + (size_t)bx * 8 + x] = (uint8_t)s[y];
      }
    }
  }
}

template <int HS, int VS>
void colour(const TcamdJpegInfo& info, const uint8_t* const* planes, uint8_t* out) {
  const int H = info.h, W = info.w;
  const int cw = (W + HS - 1) / HS, ch = (H + VS - 1) / VS;
  const size_t ys = (size_t)info.bw[0] * 8, cs = (size_t)info.bw[1] * 8;
  for (int Y = 0; Y < H; ++Y) {
    for (int X = 0; X < W; ++X) {
      const int cb = chroma_up<HS, VS>([&](int x, int y) { return (int)planes[1][(size_t)y * cs + x]; }, X, Y, cw, ch);
      const int cr = chroma_up<HS, VS>([&](int x, int y) { return (int)planes[2][(size_t)y * cs + x]; }, X, Y, cw, ch);
      int rgb[3];
      ycc_to_rgb(planes[0][(size_t)Y * ys + X], cb, cr, rgb);
      uint8_t* px = out + ((size_t)Y * W + X) * 3;
      px[0] = (uint8_t)rgb[0];
      px[1] = (uint8_t)rgb[1];
      px[2] = (uint8_t)rgb[2];
    }
  }
}

void reconstruct(const TcamdJpegInfo& info, const uint8_t* buf, uint8_t* out) {
  std::vector<uint8_t> store[3];
  const uint8_t* planes[3] = {nullptr, nullptr, nullptr};
  const uint16_t* q = reinterpret_cast<const uint16_t*>(buf);
  for (int c = 0; c < info.ncomp; ++c) {
    store[c].resize((size_t)info.bw[c] * info.bh[c] * 64);
    idct_plane(q + 64 * c, reinterpret_cast<const int16_t*>(buf + info.coef_off[c]), info.bw[c], info.bh[c],
               store[c].data());
    planes[c] = store[c].data();
  }
  if (info.ncomp == 1) {
    for (int y = 0; y < info.h; ++y)
      std::memcpy(out + (size_t)y * info.w, planes[0] + (size_t)y * info.bw[0] * 8, (size_t)info.w);
  } else if (info.hs == 1) {
    colour<1, 1>(info, planes, out);
  } else if (info.vs == 1) {
    colour<2, 1>(info, planes, out);
  } else {
    colour<2, 2>(info, planes, out);
  }
}

// one component's ny x nx blocks -> its sample plane, (bh*NY) x (bw*NX)
template <int NY, int NX>
void idct_plane_n(const uint16_t* q, const int16_t* coef, int bw, int bh, uint8_t* plane) {
  const size_t stride = (size_t)bw * NX;
  for (int by = 0; by < bh; ++by) {
    for (int bx = 0; bx < bw; ++bx) {
      const int16_t* blk = coef + ((size_t)by * bw + bx) * (NY * NX);
      int ws[NY][NX];
      for (int y = 0; y < NY; ++y) {
        int v[NX];
        for (int u = 0; u < NX; ++u) v[u] = dequantise(blk[y * NX + u], q[y * 8 + u]);
        idct_row_n<NX>(v, ws[y]);
      }
      for (int x = 0; x < NX; ++x) {
        int col[NY], s[NY];
        for (int y = 0; y < NY; ++y) col[y] = ws[y][x];
        idct_col_n<NY>(col, s);
        for (int y = 0; y < NY; ++y) plane[((size_t)by * NY + y) * stride + (size_t)bx * NX + x] = (uint8_t)s[y];
      }
    }
  }
}

// scale >= 2: every plane is at the output resolution; crop, and convert three of them
void reconstruct_scaled(const TcamdJpegInfo& info, const uint8_t* buf, uint8_t* out) {
  std::vector<uint8_t> store[3];
  size_t stride[3] = {0, 0, 0};
  const uint16_t* q = reinterpret_cast<const uint16_t*>(buf);
  for (int c = 0; c < info.ncomp; ++c) {
    const int ny = info.ny[c], nx = info.nx[c], bw = info.bw[c], bh = info.bh[c];
    store[c].resize((size_t)bw * bh * ny * nx);
    stride[c] = (size_t)bw * nx;
    const int16_t* coef = reinterpret_cast<const int16_t*>(buf + info.coef_off[c]);
    uint8_t* pl = store[c].data();
    const uint16_t* qc = q + 64 * c;
    switch (ny * 16 + nx) {
      case 0x88: idct_plane_n<8, 8>(qc, coef, bw, bh, pl); break;
      case 0x48: idct_plane_n<4, 8>(qc, coef, bw, bh, pl); break;
      case 0x44: idct_plane_n<4, 4>(qc, coef, bw, bh, pl); break;
      case 0x24: idct_plane_n<2, 4>(qc, coef, bw, bh, pl); break;
      case 0x22: idct_plane_n<2, 2>(qc, coef, bw, bh, pl); break;
      case 0x12: idct_plane_n<1, 2>(qc, coef, bw, bh, pl); break;
      default: idct_plane_n<1, 1>(qc, coef, bw, bh, pl); break;
    }
  }
  for (int y = 0; y < info.h; ++y) {
    if (info.ncomp == 1) {
      std::memcpy(out + (size_t)y * info.w, store[0].data() + (size_t)y * stride[0], (size_t)info.w);
      continue;
    }
    for (int x = 0; x < info.w; ++x) {
      int rgb[3];
      ycc_to_rgb(store[0][(size_t)y * stride[0] + x], store[1][(size_t)y * stride[1] + x],
                 store[2][(size_t)y * stride[2] + x], rgb);
      uint8_t* px = out + ((size_t)y * info.w + x) * 3;
      px[0] = (uint8_t)rgb[0];
      px[1] = (uint8_t)rgb[1];
      px[2] = (uint8_t)rgb[2];
    }
  }
}

int report(const Error& e, char* msg, int cap) {
  if (msg && cap > 0) std::snprintf(msg, (size_t)cap, "%s", e.what);
  return e.code;
}

template <class F>
int guarded(char* msg, int cap, F&& f) {
  try {
    if (msg && cap > 0) msg[0] = 0;
    f();
    return TCAMD_JPEG_OK;
  } catch (const Error& e) {
    return report(e, msg, cap);
  } catch (const std::bad_alloc&) {
    return report(Error{TCAMD_JPEG_UNSUPPORTED, "out of memory"}, msg, cap);
  }
}

}  // namespace

extern "C" {

int tcamd_host_jpeg_parse(const uint8_t* blob, uint64_t n, TcamdJpegInfo* info, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&] {
    Parsed P;
    parse(blob, (size_t)n, P);
    fill_info(P, info);
  });
}

int tcamd_host_jpeg_entropy_decode(const uint8_t* blob, uint64_t n, uint8_t* buf, uint64_t cap, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&] {
    Parsed P;
    parse(blob, (size_t)n, P);
    TcamdJpegInfo info;
    fill_info(P, &info);
    if (cap < info.coef_bytes) bad("coefficient buffer too small");
    entropy_decode(blob, (size_t)n, P, info, buf);
  });
}

int tcamd_host_jpeg_parse_scaled(const uint8_t* blob, uint64_t n, int scale, TcamdJpegInfo* info, char* msg,
                                 int msg_cap) {
  return guarded(msg, msg_cap, [&] {
    check_scale(scale);
    Parsed P;
    parse(blob, (size_t)n, P);
    fill_info(P, info, scale);
  });
}

int tcamd_host_jpeg_entropy_decode_scaled(const uint8_t* blob, uint64_t n, int scale, uint8_t* buf, uint64_t cap,
                                          char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&] {
    check_scale(scale);
    Parsed P;
    parse(blob, (size_t)n, P);
    TcamdJpegInfo info;
    fill_info(P, &info, scale);
    if (cap < info.coef_bytes) bad("coefficient buffer too small");
    entropy_decode(blob, (size_t)n, P, info, buf);
  });
}

int tcamd_host_jpeg_decode_scaled(const uint8_t* blob, uint64_t n, int scale, uint8_t* out, uint64_t cap, char* msg,
                                  int msg_cap) {
  if (scale == 1) return tcamd_host_jpeg_decode(blob, n, out, cap, msg, msg_cap);
  return guarded(msg, msg_cap, [&] {
    check_scale(scale);
    Parsed P;
    parse(blob, (size_t)n, P);
    TcamdJpegInfo info;
    fill_info(P, &info, scale);
    if (cap < (uint64_t)info.h * info.w * info.ncomp) bad("pixel buffer too small");
    std::vector<uint8_t> coef((size_t)info.coef_bytes);
    entropy_decode(blob, (size_t)n, P, info, coef.data());
    reconstruct_scaled(info, coef.data(), out);
  });
}

uint64_t tcamd_host_jpeg_stream_bound(uint64_t n) {
  // every table and segment slot, the blob itself, the padding of every segment and of the whole
  return (uint64_t)jh::data_offset(jh::kMaxTabs, jh::kMaxSub) + n + 4ull * jh::kMaxSub + 4 * jh::kTailPad;
}

int tcamd_host_jpeg_stream_pack(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* used,
                                TcamdJpegInfo* info, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&] {
    Parsed P;
    parse(blob, (size_t)n, P);
    if (info) fill_info(P, info);
    try {
      if (reinterpret_cast<uintptr_t>(out) % 16) throw NotPackable{};  // the buffer is read as words on the device
      const uint64_t bytes = stream_pack(blob, (size_t)n, P, out, cap);
      if (used) *used = bytes;
    } catch (const NotPackable&) {
      throw Error{TCAMD_JPEG_NOT_PACKABLE, "not packable"};
    }
  });
}

int tcamd_host_jpeg_huffman_emulate(const uint8_t* stream, uint8_t* coef, uint64_t cap, uint32_t* status,
                                    uint32_t* rounds) {
  uint32_t st = jh::kBadHeader;
  try {
    st = emulate(stream, coef, cap, rounds);
  } catch (const std::bad_alloc&) {
    return -1;
  }
  if (status) *status = st;
  return 0;
}

uint64_t tcamd_host_jpeg_stream_bound_wide(uint64_t n) {
  // as above; a restart interval ends in a marker of two bytes, so n bytes hold n / 2 + 1 at most
  const uint64_t nseg = n / 2 + 1 < jh::kWideMaxSub ? n / 2 + 1 : jh::kWideMaxSub;
  return (uint64_t)jh::data_offset(jh::kMaxTabs, (uint32_t)nseg) + n + 4 * nseg + 4 * jh::kTailPad;
}

int tcamd_host_jpeg_stream_pack_wide(const uint8_t* blob, uint64_t n, int scale, uint8_t* out, uint64_t cap,
                                     uint64_t* used, uint32_t* nsub, TcamdJpegInfo* info, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&] {
    check_scale(scale);
    Parsed P;
    parse(blob, (size_t)n, P);
    if (info) fill_info(P, info, scale);
    try {
      if (reinterpret_cast<uintptr_t>(out) % 16) throw NotPackable{};  // the buffer is read as words on the device
      const uint64_t bytes = stream_pack(blob, (size_t)n, P, out, cap,
                                         PackFor{jh::kWideMagic, jh::kWideMaxSub, jh::kWideMaxDataBytes, (uint32_t)scale});
      if (used) *used = bytes;
      if (nsub) *nsub = reinterpret_cast<const jh::StreamHeader*>(out)->nsub;
    } catch (const NotPackable&) {
      throw Error{TCAMD_JPEG_NOT_PACKABLE, "not packable"};
    }
  });
}

int tcamd_host_jpeg_huffman_wide_emulate(const uint8_t* stream, uint8_t* coef, uint64_t cap, uint32_t chunk_subs,
                                         uint32_t* status, uint32_t* launches_that_changed) {
  uint32_t st = jh::kBadHeader;
  try {
    st = emulate_wide(stream, coef, cap, chunk_subs, launches_that_changed);
  } catch (const std::bad_alloc&) {
    return -1;
  }
  if (status) *status = st;
  return 0;
}

uint64_t tcamd_host_jpeg_huffman_wide_workspace(uint64_t total_subsequences, uint64_t total_chunks) {
  return jh::wide_ws_bytes(total_subsequences, total_chunks);
}

int tcamd_host_jpeg_decode(const uint8_t* blob, uint64_t n, uint8_t* out, uint64_t cap, char* msg, int msg_cap) {
  return guarded(msg, msg_cap, [&] {
    Parsed P;
    parse(blob, (size_t)n, P);
    TcamdJpegInfo info;
    fill_info(P, &info);
    if (cap < (uint64_t)info.h * info.w * info.ncomp) bad("pixel buffer too small");
    std::vector<uint8_t> coef((size_t)info.coef_bytes);
    entropy_decode(blob, (size_t)n, P, info, coef.data());
    reconstruct(info, coef.data(), out);
  });
}

}  // extern "C"
