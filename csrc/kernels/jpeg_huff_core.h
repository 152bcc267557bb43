// The Huffman stage of the baseline JPEG decode as K23 jpeg_huffman runs it
// (csrc/kernels/jpeg_huff.hip), in plain C++ that the kernel and the host
// library (csrc/host/jpeg.cc: the stream pack and the emulation of the kernel)
// both compile, as they do jpeg_math.h.  Nothing here trusts the stream buffer:
// every table index, word index and write index is checked, every loop is
// bounded by a bit count or a validated element count.
//
// Stream buffer (what tcamd_host_jpeg_stream_pack writes, little endian, 16-byte
// aligned):
//   StreamHeader                      64 bytes
//   uint16 q[3][64]                   quantisation tables per component, natural order (K22's form)
//   HuffTab tab[ntab]                 the distinct Huffman tables the scan names, in order of first use
//   Segment seg[nseg]                 one per restart interval (one when there is no DRI)
//   data, from a 16-byte boundary     the entropy-coded bytes without FF 00 stuffing and RSTn markers,
//                                     each segment from a 4-byte boundary, zero bytes between them and
//                                     16 zero bytes after the last
// A segment is cut into subsequences of kSubBits bits (the last one shorter, an
// empty segment has one empty subsequence); Segment::first_sub numbers them
// through the image.  A bit position is counted from the first data byte, MSB
// first.
//
// The algorithm, one workgroup (kThreads threads) per image, the phases
// separated by workgroup barriers (the emulation runs each phase for every
// thread in turn):
//   init    tables -> workspace, coefficient area zeroed, quantisation tables written, the segment
//           table checked, every subsequence given the entry (its first bit, block 0, DC next)
//   sync    rounds of read (take the predecessor's exit as the entry if it is valid and differs
//           from the entry last decoded from) and decode (from the entry to the first symbol
//           boundary at or past the subsequence's end).  The first subsequence of a segment is
//           right from the start, so after round k the first k + 1 are; a round without a decode
//           is the fixed point.  An invalid exit is never taken as an entry.
//   count   per segment, serially: the exclusive sums of completed blocks and of the DC
//           differences per component give every subsequence its first block and predictors
//   write   every subsequence decodes once more from its true entry and stores values at
//           natural-order positions of K22's layout, the DC as the running predictor; it stops at
//           the segment's block budget
// Errors end in one status word per image.
#pragma once

#include <stdint.h>

#include "jpeg_math.h"

namespace tcamd_jhuff {

constexpr int kThreads = 1024;  // one subsequence per thread up to 1024 of them
constexpr uint32_t kSubBits = 1024;  // S: bits per subsequence (128 bytes)
constexpr int kMaxSub = 2048;        // subsequences per image: what the workspace holds
constexpr int kMaxTabs = 6;
constexpr uint32_t kMaxDataBytes = kMaxSub * (kSubBits / 8);  // 256 KiB of unstuffed scan data
constexpr uint32_t kMagic = 0x3153544au;                      // "JTS1"
constexpr int kMaxDim = 16384;
constexpr uint32_t kTailPad = 16;  // zero bytes after the last segment

enum Status : uint32_t {
  kOk = 0,
  kBadHeader = 1,
  kBadCode = 2,
  kDcCategory = 3,
  kAcCategory = 4,
  kRunPast63 = 5,
  kEndsEarly = 6,
  kRestartRule = 7,
  kDcRange = 8,
  kBadState = 9,
  kWriteBounds = 10,
};

struct HuffTab {
  uint16_t look[512];   // 9 leading bits -> (length << 8) | symbol, 0 when the code is longer
  int32_t maxcode[17];  // last code of each length, -1 when the length has none
  int32_t valoff[17];   // index of the first symbol of a length minus its first code
  uint8_t vals[256];
};
static_assert(sizeof(HuffTab) == 1416, "HuffTab is part of the stream buffer");

struct StreamHeader {
  uint32_t magic, total_bytes;
  int32_t h, w, ncomp, hs, vs, mcux, mcuy;
  uint32_t interval;  // MCUs per segment: DRI, or all of them
  uint32_t nseg, nsub, ntab;
  uint32_t tabmap;  // component c: DC table in bits [8c, 8c+4), AC table in bits [8c+4, 8c+8)
  uint32_t data_bytes;
  uint32_t reserved;
};
static_assert(sizeof(StreamHeader) == 64, "StreamHeader is part of the stream buffer");

struct Segment {
  uint32_t byte_off;  // from the first data byte, a multiple of 4
  uint32_t bits;
  uint32_t first_mcu;
  uint32_t first_sub;
};

constexpr uint32_t kQOff = sizeof(StreamHeader);
constexpr uint32_t kTabOff = kQOff + 3 * 128;

TCAMD_HD uint32_t data_offset(uint32_t ntab, uint32_t nseg) {
  return (kTabOff + ntab * (uint32_t)sizeof(HuffTab) + nseg * (uint32_t)sizeof(Segment) + 15u) & ~15u;
}

TCAMD_HD uint32_t subs_of(uint32_t bits) { return bits == 0 ? 1u : (bits + kSubBits - 1) / kSubBits; }

// what a thread needs of the header, checked
// (no array a thread indexes with a run-time value: it would live in scratch memory)
struct Geo {
  int32_t ncomp, hs, vs, mcux, bpm;
  int32_t bw0, bw1;                      // blocks per row of the luma / of a chroma component
  uint32_t off0, off1, off2, coef_bytes;  // coef_off[c]
  uint32_t mcus, interval, nseg, nsub, ntab, nwords;
  uint32_t dc_pack, ac_pack, comp_pack;  // 4 bits per block of the MCU: its DC table, AC table, component
  const uint8_t* q;
  const uint32_t* tabs;
  const Segment* segs;
  const uint32_t* words;
};

// magic, max_sub, max_data: what the reading kernel takes (K23: kMagic, kMaxSub, kMaxDataBytes; the
// wide kernels of jpeg_huff_wide_core.h have their own)
TCAMD_HD bool read_header_as(const uint8_t* buf, Geo& g, uint32_t magic, uint32_t max_sub, uint32_t max_data) {
  const StreamHeader& h = *reinterpret_cast<const StreamHeader*>(buf);
  if (h.magic != magic) return false;
  if (h.h < 1 || h.w < 1 || h.h > kMaxDim || h.w > kMaxDim) return false;
  const bool grey = h.ncomp == 1 && h.hs == 1 && h.vs == 1;
  const bool colour = h.ncomp == 3 && (h.hs == 1 || h.hs == 2) && (h.vs == 1 || h.vs == 2) && !(h.hs == 1 && h.vs == 2);
  if (!grey && !colour) return false;
  if (h.mcux != (h.w + 8 * h.hs - 1) / (8 * h.hs) || h.mcuy != (h.h + 8 * h.vs - 1) / (8 * h.vs)) return false;
  g.ncomp = h.ncomp;
  g.hs = h.hs;
  g.vs = h.vs;
  g.mcux = h.mcux;
  g.bpm = h.ncomp == 1 ? 1 : h.hs * h.vs + 2;
  g.mcus = (uint32_t)h.mcux * (uint32_t)h.mcuy;  // at most 2048 * 2048
  uint64_t off = (uint64_t)h.ncomp * 128;
  g.bw0 = h.mcux * h.hs;
  g.bw1 = h.mcux;
  g.off0 = (uint32_t)off;
  off += (uint64_t)g.bw0 * (uint64_t)(h.mcuy * h.vs) * 128;
  g.off1 = (uint32_t)off;
  if (h.ncomp == 3) off += (uint64_t)g.bw1 * (uint64_t)h.mcuy * 128;
  g.off2 = (uint32_t)off;
  if (h.ncomp == 3) off += (uint64_t)g.bw1 * (uint64_t)h.mcuy * 128;
  if (off > 0xffffffffull) return false;  // 16384 x 16384 x 3 samples x 2 bytes fits
  g.coef_bytes = (uint32_t)off;
  if (h.interval < 1 || h.interval > g.mcus) return false;
  if (h.nseg != (g.mcus + h.interval - 1) / h.interval) return false;
  if (h.nsub < h.nseg || h.nsub > max_sub) return false;
  if (h.ntab < 1 || h.ntab > (uint32_t)kMaxTabs) return false;
  if (h.data_bytes < kTailPad || h.data_bytes > max_data + 4 * h.nseg + 2 * kTailPad) return false;
  if (h.data_bytes % 4) return false;
  if (h.total_bytes != data_offset(h.ntab, h.nseg) + h.data_bytes) return false;
  g.interval = h.interval;
  g.nseg = h.nseg;
  g.nsub = h.nsub;
  g.ntab = h.ntab;
  g.nwords = h.data_bytes / 4;
  g.dc_pack = g.ac_pack = g.comp_pack = 0;
  for (int b = 0; b < 6; ++b) {
    const uint32_t c = h.ncomp == 1 ? 0 : (b < h.hs * h.vs ? 0 : (b - h.hs * h.vs + 1 < 3 ? b - h.hs * h.vs + 1 : 2));
    const uint32_t dc = (h.tabmap >> (8 * c)) & 15, ac = (h.tabmap >> (8 * c + 4)) & 15;
    if (dc >= h.ntab || ac >= h.ntab) return false;
    g.comp_pack |= c << (4 * b);
    g.dc_pack |= dc << (4 * b);
    g.ac_pack |= ac << (4 * b);
  }
  g.q = buf + kQOff;
  g.tabs = reinterpret_cast<const uint32_t*>(buf + kTabOff);
  g.segs = reinterpret_cast<const Segment*>(buf + kTabOff + h.ntab * sizeof(HuffTab));
  g.words = reinterpret_cast<const uint32_t*>(buf + data_offset(h.ntab, h.nseg));
  return true;
}

TCAMD_HD bool read_header(const uint8_t* buf, Geo& g) {
  return read_header_as(buf, g, kMagic, (uint32_t)kMaxSub, kMaxDataBytes);
}

// the workspace of one image: LDS on the device
struct Work {
  HuffTab tab[kMaxTabs];
  uint32_t exit0[kMaxSub];  // bit position | state << 22 | invalid << 31
  uint32_t aux[kMaxSub];    // sync: the entry last decoded from; from count on: the first block, or kSkip
  int32_t dc[kMaxSub][3];   // DC difference sums of the last decode; from count on: the predictors at entry
  uint16_t cnt[kMaxSub];    // blocks completed by the last decode | kTodo
  uint16_t seg[kMaxSub];
  uint32_t status;
};

constexpr uint32_t kInvalid = 1u << 31;
constexpr uint32_t kPosMask = (1u << 22) - 1;
constexpr uint16_t kTodo = 1u << 15;
constexpr uint32_t kSkip = 0xffffffffu;
static_assert(kMaxDataBytes * 8 + 64 * (uint32_t)kMaxSub <= kPosMask, "a bit position fits its field");

TCAMD_HD void set_status(Work& w, uint32_t code) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(&w.status, code);
#else
  if (w.status < code) w.status = code;
#endif
}

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

TCAMD_HD uint32_t nibble(uint32_t pack, uint32_t blk) { return (pack >> (4 * blk)) & 15; }  // blk < 6

TCAMD_HD uint32_t be_word(const Geo& g, uint32_t i) {
  if (i >= g.nwords) return 0;
  const uint32_t v = g.words[i];
  return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
}

// The data words around a bit position, kept in registers: w0 holds bit `32 * i`, w1 the word
// after it; w2 and w3 follow and are loaded two words ahead of their use, so that the wait for a
// load falls a word (several symbols) after its issue and a symbol does not wait for memory.  A
// symbol has at most 27 bits, so a position moves on by at most one word.
struct Window {
  uint32_t i, w0, w1, w2, w3;
  TCAMD_HD void open(const Geo& g, uint32_t pos) {
    i = pos >> 5;
    w0 = be_word(g, i);
    w1 = be_word(g, i + 1);
    w2 = be_word(g, i + 2);
    w3 = be_word(g, i + 3);
  }
  TCAMD_HD void move_to(const Geo& g, uint32_t pos) {
    if ((pos >> 5) != i) {
      ++i;
      w0 = w1;
      w1 = w2;
      w2 = w3;
      w3 = be_word(g, i + 3);
    }
  }
  // the 32 bits from bit `pos` (in word i), those at or past `limit` read as zero
  TCAMD_HD uint32_t peek32(uint32_t pos, uint32_t limit) const {
    const uint32_t sh = pos & 31;
    uint32_t v = sh ? (w0 << sh) | (w1 >> (32 - sh)) : w0;
    const uint32_t avail = limit - pos;
    if (avail < 32) v = avail ? v & (0xffffffffu << (32 - avail)) : 0;
    return v;
  }
};

// The per-thread routine.  From bit `pos` in state `state` (block within the
// MCU * 64 + zigzag index, 0 = a DC symbol is next) it decodes whole symbols
// (a Huffman code and its value bits) until the position is at or past `stop`
// or `budget` blocks are complete; `limit` (>= stop) is the end of the
// segment: bits past it read as zero and consuming one is kEndsEarly.  Returns
// kOk with pos / state / done at the exit, or the reason the data is invalid.
// emit(blocks done, block within the MCU, natural index, value) gets every
// coefficient, the DC (natural index 0 of a fresh block) as its difference.
// Each pass consumes at least one bit, so the loop ends within limit - pos passes.
template <class Emit>
TCAMD_HD uint32_t decode(const Geo& g, const HuffTab* tabs, uint32_t& pos, uint32_t& state, uint32_t stop,
                         uint32_t limit, uint32_t budget, uint32_t& done, Emit&& emit) {
  uint32_t blk = state >> 6, zz = state & 63;
  done = 0;
  if (blk >= (uint32_t)g.bpm || stop > limit) return kBadState;
  Window win;
  win.open(g, pos);
  while (pos < stop && done < budget) {
    const uint32_t avail = limit - pos;
    const uint32_t v32 = win.peek32(pos, limit);
    const uint32_t v = v32 >> 16;
    const HuffTab& t = tabs[nibble(zz == 0 ? g.dc_pack : g.ac_pack, blk)];  // < ntab <= kMaxTabs: read_header
    const uint32_t e = t.look[v >> 7];
    uint32_t len, sym;
    if (e) {
      len = e >> 8;
      sym = e & 255;
      if (len == 0 || len > 16) return kBadCode;  // the pack writes neither; a pass consumes a bit
    } else {
      len = 10;
      while (len <= 16 && (int32_t)(v >> (16 - len)) > t.maxcode[len]) ++len;
      if (len > 16) return kBadCode;
      const int32_t idx = (int32_t)(v >> (16 - len)) + t.valoff[len];
      if (idx < 0 || idx > 255) return kBadCode;
      sym = t.vals[idx];
    }
    if (len > avail) return kEndsEarly;
    const uint32_t s = zz == 0 ? sym : (sym & 15), r = zz == 0 ? 0 : (sym >> 4);
    if (zz == 0 && s > 11) return kDcCategory;
    if (zz != 0 && s > 10) return kAcCategory;
    if (len + s > avail) return kEndsEarly;
    int val = 0;
    if (s) {
      const int u = (int)((v32 << len) >> (32 - s));
      val = u >= (1 << (s - 1)) ? u : u - (1 << s) + 1;
    }
    bool complete = false;
    if (zz == 0) {
      emit(done, blk, 0u, val);
      zz = 1;
    } else if (s == 0) {
      if (r != 15) {
        complete = true;  // EOB
      } else {
        zz += 16;
        if (zz > 64) return kRunPast63;
        complete = zz == 64;
      }
    } else {
      zz += r;
      if (zz > 63) return kRunPast63;
      emit(done, blk, (uint32_t)kZigzag[zz], val);
      complete = ++zz == 64;
    }
    pos += len + s;
    win.move_to(g, pos);
    if (complete) {
      ++done;
      zz = 0;
      blk = blk + 1 == (uint32_t)g.bpm ? 0 : blk + 1;
    }
    state = blk * 64 + zz;
  }
  return kOk;
}

struct U4 {
  uint32_t x, y, z, w;
} __attribute__((aligned(16)));

// the bounds of subsequence i: its segment's first bit and limit, its own first bit and stop
struct Span {
  uint32_t seg, start, stop, limit, first_sub, last_sub;
};

TCAMD_HD Span span_of(const Geo& g, const Work& w, uint32_t i) {
  Span sp;
  sp.seg = w.seg[i];  // < nseg: phase_init
  const Segment sg = g.segs[sp.seg];
  const uint32_t b0 = sg.byte_off * 8;
  sp.limit = b0 + sg.bits;
  sp.first_sub = sg.first_sub;
  sp.last_sub = sg.first_sub + subs_of(sg.bits) - 1;
  sp.start = b0 + (i - sg.first_sub) * kSubBits;
  sp.stop = sp.start + kSubBits < sp.limit ? sp.start + kSubBits : sp.limit;
  if (sp.start > sp.limit) sp.start = sp.limit;
  return sp;
}

// ---- the phases: thread `tid` of kThreads --------------------------------------------------
// coef: the image's coefficient buffer, coef_bytes of its parse, 16-byte aligned
TCAMD_HD void phase_init(uint32_t tid, const Geo& g, Work& w, uint8_t* coef) {
  uint32_t* tw = reinterpret_cast<uint32_t*>(w.tab);
  for (uint32_t k = tid; k < g.ntab * (uint32_t)(sizeof(HuffTab) / 4); k += kThreads) tw[k] = g.tabs[k];
  U4* out = reinterpret_cast<U4*>(coef);
  const U4* q = reinterpret_cast<const U4*>(g.q);
  const uint32_t nq = (uint32_t)g.ncomp * 8, nall = g.coef_bytes / 16;
  for (uint32_t k = tid; k < nall; k += kThreads) out[k] = k < nq ? q[k] : U4{0, 0, 0, 0};
  for (uint32_t s = tid; s < g.nseg; s += kThreads) {
    const Segment sg = g.segs[s];
    const uint32_t n = subs_of(sg.bits);
    const uint32_t next = s + 1 < g.nseg ? g.segs[s + 1].first_sub : g.nsub;
    const bool ok = sg.byte_off % 4 == 0 && sg.byte_off <= g.nwords * 4 - kTailPad &&
                    sg.bits <= (g.nwords * 4 - kTailPad - sg.byte_off) * 8 && sg.first_mcu == s * g.interval &&
                    (s != 0 || sg.first_sub == 0) && sg.first_sub < g.nsub && n <= g.nsub - sg.first_sub &&
                    sg.first_sub + n == next;
    if (!ok) {
      set_status(w, kBadHeader);
      continue;
    }
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t i = sg.first_sub + j;  // < nsub <= kMaxSub
      w.seg[i] = (uint16_t)s;
      w.aux[i] = sg.byte_off * 8 + j * kSubBits;  // state 0
      w.exit0[i] = kInvalid;
      w.cnt[i] = kTodo;
    }
  }
}

TCAMD_HD void phase_sync_read(uint32_t tid, const Geo& g, Work& w) {
  for (uint32_t i = tid; i < g.nsub; i += kThreads) {
    if (i == 0 || w.seg[i - 1] != w.seg[i]) continue;  // the first of a segment keeps its entry
    const uint32_t e = w.exit0[i - 1];
    if (!(e & kInvalid) && e != w.aux[i]) {
      w.aux[i] = e;
      w.cnt[i] |= kTodo;
    }
  }
}

// (the functors copy what they need of the Geo: a reference kept in a struct would keep the
// whole Geo in scratch memory)
struct SumDc {
  uint32_t comp_pack;
  int32_t s0, s1, s2;
  TCAMD_HD void operator()(uint32_t, uint32_t blk, uint32_t nat, int val) {
    if (nat != 0) return;  // an AC value never has natural index 0
    const uint32_t c = nibble(comp_pack, blk);
    s0 += c == 0 ? val : 0;
    s1 += c == 1 ? val : 0;
    s2 += c == 2 ? val : 0;
  }
};

// returns whether this thread decoded anything
TCAMD_HD bool phase_sync_decode(uint32_t tid, const Geo& g, Work& w) {
  bool any = false;
  for (uint32_t i = tid; i < g.nsub; i += kThreads) {
    if (!(w.cnt[i] & kTodo)) continue;
    any = true;
    const Span sp = span_of(g, w, i);
    uint32_t pos = w.aux[i] & kPosMask, state = (w.aux[i] >> 22) & 511, done = 0;
    SumDc sum{g.comp_pack, 0, 0, 0};
    uint32_t rc = kBadState;
    if (pos <= sp.limit) rc = decode(g, w.tab, pos, state, sp.stop, sp.limit, 0x7fffu, done, sum);
    w.exit0[i] = rc == kOk ? (pos | (state << 22)) : kInvalid;
    w.cnt[i] = (uint16_t)done;  // at most kSubBits / 2 + 1
    w.dc[i][0] = sum.s0;
    w.dc[i][1] = sum.s1;
    w.dc[i][2] = sum.s2;
  }
  return any;
}

TCAMD_HD int32_t saturate30(int64_t v) {
  const int64_t lim = 1 << 30;
  return (int32_t)(v < -lim ? -lim : (v > lim ? lim : v));
}

TCAMD_HD void phase_count(uint32_t tid, const Geo& g, Work& w) {
  for (uint32_t s = tid; s < g.nseg; s += kThreads) {
    const Segment sg = g.segs[s];
    const uint32_t n = subs_of(sg.bits);  // checked against nsub in phase_init
    uint32_t first = 0;
    int64_t pred[3] = {0, 0, 0};
    bool right = true;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t i = sg.first_sub + j;
      w.aux[i] = right ? first : kSkip;
      for (int c = 0; c < 3; ++c) {
        const int32_t d = w.dc[i][c];
        w.dc[i][c] = saturate30(pred[c]);  // a predictor this far out fails the range check for sure
        pred[c] += d;
      }
      first += w.cnt[i] & 0x7fffu;
      if (w.exit0[i] & kInvalid) right = false;
    }
  }
}

struct Store {
  uint32_t bpm, mcux, hs, vs, comp_pack, off0, off1, off2, bw0, bw1, coef_bytes, mcus;
  uint8_t* coef;
  uint32_t mcu0, first;  // the segment's first MCU, the subsequence's first block in the segment
  int32_t p0, p1, p2;
  uint32_t err;
  TCAMD_HD void operator()(uint32_t done, uint32_t blk, uint32_t nat, int val) {
    const uint32_t b = first + done;  // the block in the segment
    const uint32_t mcu = mcu0 + b / (uint32_t)bpm;
    const uint32_t c = nibble(comp_pack, blk);
    // masks, not selects between neighbouring members: the compiler turns those into an indexed
    // load, and the struct then lives in scratch memory
    const uint32_t m0 = 0u - (uint32_t)(c == 0), m1 = 0u - (uint32_t)(c == 1), m2 = 0u - (uint32_t)(c == 2);
    if (nat == 0) {
      // |predictor| <= 2^30 and a subsequence adds less than 2^21: no overflow
      const int32_t p = (int32_t)(((uint32_t)p0 & m0) | ((uint32_t)p1 & m1) | ((uint32_t)p2 & m2)) + val;
      p0 = (int32_t)(((uint32_t)p & m0) | ((uint32_t)p0 & ~m0));
      p1 = (int32_t)(((uint32_t)p & m1) | ((uint32_t)p1 & ~m1));
      p2 = (int32_t)(((uint32_t)p & m2) | ((uint32_t)p2 & ~m2));
      if (p < -32768 || p > 32767) {
        err = kDcRange;
        return;
      }
      val = p;
    }
    const uint32_t mx = mcu % (uint32_t)mcux, my = mcu / (uint32_t)mcux;
    const uint32_t bx = c == 0 ? mx * hs + blk % hs : mx, by = c == 0 ? my * vs + blk / hs : my;
    const uint32_t first_off = (off0 & m0) | (off1 & m1) | (off2 & m2);
    const uint64_t off = first_off + ((uint64_t)by * ((bw0 & m0) | (bw1 & ~m0)) + bx) * 128 + nat * 2;
    if (mcu >= mcus || off + 2 > coef_bytes) {
      err = kWriteBounds;
      return;
    }
    *reinterpret_cast<int16_t*>(coef + off) = (int16_t)val;
  }
};

TCAMD_HD void phase_write(uint32_t tid, const Geo& g, Work& w, uint8_t* coef) {
  for (uint32_t i = tid; i < g.nsub; i += kThreads) {
    const uint32_t first = w.aux[i];
    if (first == kSkip) continue;
    const Span sp = span_of(g, w, i);
    const uint32_t mcu0 = sp.seg * g.interval;
    const uint32_t left = g.mcus - mcu0;  // interval >= 1 and seg < nseg: mcu0 < mcus
    const uint32_t blocks = (left < g.interval ? left : g.interval) * (uint32_t)g.bpm;
    if (first >= blocks) continue;  // the budget was met before this subsequence
    uint32_t pos = sp.start, state = 0, done = 0;
    if (i != sp.first_sub) {
      const uint32_t e = w.exit0[i - 1];  // valid: phase_count
      pos = e & kPosMask;
      state = (e >> 22) & 511;
    }
    if (pos > sp.limit) {
      set_status(w, kBadState);
      continue;
    }
    Store st{(uint32_t)g.bpm, (uint32_t)g.mcux, (uint32_t)g.hs, (uint32_t)g.vs, g.comp_pack, g.off0, g.off1, g.off2,
             (uint32_t)g.bw0, (uint32_t)g.bw1, g.coef_bytes, g.mcus, coef, mcu0, first,
             w.dc[i][0], w.dc[i][1], w.dc[i][2], kOk};
    const uint32_t rc = decode(g, w.tab, pos, state, sp.stop, sp.limit, blocks - first, done, st);
    if (rc != kOk) {
      set_status(w, rc);
    } else if (st.err != kOk) {
      set_status(w, st.err);
    } else if (first + done == blocks) {
      // the RSTn rule of the host decoder: only padding, fewer than 8 bits, before the marker
      if (sp.seg + 1 < g.nseg && sp.limit - pos >= 8) set_status(w, kRestartRule);
    } else if (i == sp.last_sub) {
      set_status(w, kEndsEarly);
    }
  }
}

}  // namespace tcamd_jhuff
