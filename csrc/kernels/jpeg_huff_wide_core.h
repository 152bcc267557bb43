// The Huffman stage of the baseline JPEG decode as the K24 jpeg_huffman_wide
// kernels run it (csrc/kernels/jpeg_huff_wide.hip), in plain C++ that the
// kernels and the host library (csrc/host/jpeg.cc: the wide stream pack and the
// emulation of the launch sequence) both compile.  It is K23's algorithm
// (jpeg_huff_core.h: decode(), Window, HuffTab, Segment and the status codes
// are used as they are) without K23's two limits: the scan may be as long as
// the staging area (kWideMaxDataBytes), and the coefficients are stored in the
// compact layout of any jpeg_scale.
//
// Stream buffer: K23's, with kWideMagic and the scale (1, 2, 4 or 8) in the
// header word K23 leaves reserved.  Neither kernel accepts the other's buffer.
//
// An image's subsequences (kSubBits bits, numbered through the image) are dealt
// in order into chunks of `cs` subsequences (a power of two up to kThreads, the
// default); one workgroup handles one chunk, one subsequence per thread.  The
// per-subsequence state lives in a device workspace the caller provides
// (WideWs).  Workgroups never wait for each other inside a launch: what one
// chunk hands to the next crosses a kernel boundary.  The launches of a call:
//   init      every workgroup validates the header again; the coefficient area is zeroed and the
//             quantisation tables written, strided over all workgroups of the image; the segment
//             table is checked; every subsequence finds its segment by binary search of
//             Segment::first_sub and gets its own first bit as its entry
//   sync 0    every chunk runs K23's read / decode rounds among its own subsequences until a
//             round decodes nothing, and publishes the exit of its last subsequence
//   sync r    r = 1 .. R, R = the largest chunk count of an image - 1: chunk k takes the exit chunk
//             k - 1 published in launch r - 1 (two slots per chunk, by launch parity) as the entry
//             of its first subsequence if that is in the same segment, valid, and not the entry
//             last decoded from, and runs its rounds again; they end as soon as exits stop
//             changing.  A chunk whose entry did not change returns at once.  As in K23, the
//             first chunk of a segment's run is right after launch 0, so after launch r the
//             first r + 1 are: R launches reach the fixed point with nothing read back.
//   count     a segmented exclusive scan of completed blocks, DC sums (64-bit) and the "an exit
//             before me in my segment is invalid" flag: inside every chunk, then over the chunk
//             totals by one workgroup per image
//   write     every subsequence adds its chunk's carry-in to its own prefix, decodes once more
//             from its true entry and stores what the scale keeps; the restart rule, the block
//             budget and kEndsEarly on a segment's last subsequence as in K23's phase_write
// Errors end in one status word per image, by atomicMax; the kernels never trap and write only
// inside [coef, coef + coef_bytes), the status words and the workspace.
#pragma once

#include "jpeg_huff_core.h"

namespace tcamd_jhuff {

constexpr uint32_t kWideMagic = 0x3157544au;  // "JTW1"
constexpr uint32_t kWideMaxSub = 1u << 18;    // subsequences per image
constexpr uint32_t kWideMaxDataBytes = kWideMaxSub * (kSubBits / 8);  // 32 MiB of unstuffed scan data
constexpr int kWideMaxImgs = 64;                                      // images per launch sequence
// a bit position (data, the padding of every segment, the tail) stays a 32-bit count
static_assert(((uint64_t)kWideMaxDataBytes + 4ull * kWideMaxSub + 2 * kTailPad) * 8 < (1ull << 32),
              "a bit position fits 32 bits");

// An exit, and the entry made of it: the bits past the subsequence's nominal end (an exit lies
// within one symbol of it) | state << kRelBits | kInvalid.  The nominal end of a subsequence is
// the first bit of the next one of its segment, so the word is the successor's entry as it is.
constexpr uint32_t kRelBits = 6;
constexpr uint32_t kRelMask = (1u << kRelBits) - 1;
constexpr uint32_t kMaxSymbolBits = 16 + 11;
static_assert(kMaxSymbolBits - 1 <= kRelMask, "the field holds an exit of the largest scan: it is relative");
constexpr uint32_t kTodoW = 1u << 31;
// blocks a subsequence can complete (two bits each at least), and the largest DC difference
constexpr int64_t kMaxSubDc = (int64_t)(kSubBits / 2 + 1) * 2047;
static_assert(kMaxSubDc * kThreads < (1ll << 31), "the DC sums inside a chunk fit 32 bits");

struct WideGeo {
  Geo g;  // off0 .. off2, coef_bytes: the compact layout of the scale
  uint32_t ny0, nx0, ny1, nx1;  // the coefficients kept of a luma / a chroma block
};

// the layout is fill_info's (csrc/host/jpeg.cc): 16-byte aligned offsets, ny * nx int16 per block
TCAMD_HD bool read_header_wide(const uint8_t* buf, WideGeo& wg) {
  Geo& g = wg.g;
  if (!read_header_as(buf, g, kWideMagic, kWideMaxSub, kWideMaxDataBytes)) return false;
  const StreamHeader& h = *reinterpret_cast<const StreamHeader*>(buf);
  if (h.reserved > 8 || !tcamd_jpeg::scale_ok((int)h.reserved)) return false;
  const int scale = (int)h.reserved;
  wg.ny0 = (uint32_t)tcamd_jpeg::scaled_size(scale, h.vs, h.vs);
  wg.nx0 = (uint32_t)tcamd_jpeg::scaled_size(scale, h.hs, h.hs);
  wg.ny1 = (uint32_t)tcamd_jpeg::scaled_size(scale, h.vs, 1);
  wg.nx1 = (uint32_t)tcamd_jpeg::scaled_size(scale, h.hs, 1);
  const uint64_t luma = (uint64_t)g.bw0 * (uint64_t)(h.mcuy * h.vs) * (wg.ny0 * wg.nx0 * 2);
  const uint64_t chroma = (uint64_t)g.bw1 * (uint64_t)h.mcuy * (wg.ny1 * wg.nx1 * 2);
  uint64_t off = (uint64_t)h.ncomp * 128;  // a multiple of 16
  g.off0 = (uint32_t)off;
  off += luma;
  if (h.ncomp == 3) off = (off + 15) / 16 * 16;
  g.off1 = (uint32_t)off;
  if (h.ncomp == 3) off = (off + chroma + 15) / 16 * 16;
  g.off2 = (uint32_t)off;
  if (h.ncomp == 3) off += chroma;
  g.coef_bytes = (uint32_t)off;  // at most the full-size buffer, which read_header_as checked
  return true;
}

// what a range of subsequences (or of chunks) adds up to, for the segmented scan
struct Acc {
  uint32_t blocks;
  uint32_t flags;  // kHead: a segment starts inside the range; kBad: an invalid exit since that start
  int64_t dc0, dc1, dc2;
};
static_assert(sizeof(Acc) == 32, "Acc is part of the workspace");
constexpr uint32_t kHead = 1, kBad = 2;

// a then b; associative, Acc{} is its identity
TCAMD_HD Acc combine(const Acc& a, const Acc& b) {
  if (b.flags & kHead) return b;
  return Acc{a.blocks + b.blocks, a.flags | b.flags, a.dc0 + b.dc0, a.dc1 + b.dc1, a.dc2 + b.dc2};
}

// The workspace of a call: `subs` subsequences and `chunks` chunks over all its images; an
// image's part starts at its first subsequence and its first chunk.
struct WideWs {
  Acc* ctot;        // per chunk: its total
  Acc* cin;         // per chunk: what the chunks before it carry in
  uint32_t* bexit0;  // per chunk: the exit of its last subsequence, as published by an even launch
  uint32_t* bexit1;  //            ... by an odd launch
  uint32_t* exit0;   // per subsequence: the exit of the last decode
  uint32_t* aux;     // sync: the entry last decoded from; from count on: the first block within the chunk's run
  uint32_t* cnt;     // sync: blocks completed by the last decode | kTodoW; from count on: kHead | kBad of the prefix
  uint32_t* seg;
  int32_t* dc;  // [3] per subsequence: DC sums of the last decode; from count on: their prefix within the chunk
};

TCAMD_HD uint64_t wide_ws_bytes(uint64_t subs, uint64_t chunks) {
  return (chunks * (2 * sizeof(Acc) + 8) + subs * 28 + 15) / 16 * 16;
}

// base: 16-byte aligned
TCAMD_HD WideWs wide_ws_carve(uint8_t* base, uint64_t subs, uint64_t chunks) {
  WideWs w;
  w.ctot = reinterpret_cast<Acc*>(base);
  w.cin = w.ctot + chunks;
  w.bexit0 = reinterpret_cast<uint32_t*>(w.cin + chunks);
  w.bexit1 = w.bexit0 + chunks;
  w.exit0 = w.bexit1 + chunks;
  w.aux = w.exit0 + subs;
  w.cnt = w.aux + subs;
  w.seg = w.cnt + subs;
  w.dc = reinterpret_cast<int32_t*>(w.seg + subs);
  return w;
}

TCAMD_HD WideWs wide_ws_of_image(const WideWs& a, uint64_t first_sub, uint64_t first_chunk) {
  WideWs w;
  w.ctot = a.ctot + first_chunk;
  w.cin = a.cin + first_chunk;
  w.bexit0 = a.bexit0 + first_chunk;
  w.bexit1 = a.bexit1 + first_chunk;
  w.exit0 = a.exit0 + first_sub;
  w.aux = a.aux + first_sub;
  w.cnt = a.cnt + first_sub;
  w.seg = a.seg + first_sub;
  w.dc = a.dc + 3 * first_sub;
  return w;
}

TCAMD_HD bool chunk_subs_ok(uint32_t cs) { return cs >= 1 && cs <= (uint32_t)kThreads && (cs & (cs - 1)) == 0; }

// chunk k of an image's chunks of cs subsequences: its first subsequence and how many it has
struct Chunk {
  uint32_t k, nchunk, first, n;
};

TCAMD_HD Chunk chunk_of(const Geo& g, uint32_t cs, uint32_t k) {
  Chunk c;
  c.k = k;
  c.nchunk = (g.nsub + cs - 1) / cs;
  c.first = k * cs;  // k < nchunk: below nsub
  c.n = g.nsub - c.first < cs ? g.nsub - c.first : cs;
  return c;
}

TCAMD_HD void status_max(uint32_t* status, uint32_t code) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(status, code);
#else
  if (*status < code) *status = code;
#endif
}

TCAMD_HD Span wide_span_of(const Geo& g, uint32_t seg, uint32_t i) {
  Span sp;
  sp.seg = seg;  // < nseg: wide_init
  const Segment sg = g.segs[seg];
  const uint32_t b0 = sg.byte_off * 8;
  sp.limit = b0 + sg.bits;
  sp.first_sub = sg.first_sub;
  sp.last_sub = sg.first_sub + subs_of(sg.bits) - 1;
  sp.start = b0 + (i - sg.first_sub) * kSubBits;
  sp.stop = sp.start + kSubBits < sp.limit ? sp.start + kSubBits : sp.limit;
  if (sp.start > sp.limit) sp.start = sp.limit;
  return sp;
}

// ---- the phases: thread `tid` of the kThreads of chunk c's workgroup ------------------------
TCAMD_HD void wide_load_tables(uint32_t tid, const Geo& g, HuffTab* tabs) {
  uint32_t* tw = reinterpret_cast<uint32_t*>(tabs);
  for (uint32_t j = tid; j < g.ntab * (uint32_t)(sizeof(HuffTab) / 4); j += kThreads) tw[j] = g.tabs[j];
}

// coef: the image's coefficient buffer, coef_bytes of its parse at the scale, 16-byte aligned
TCAMD_HD void wide_init(uint32_t tid, const WideGeo& wg, const WideWs& w, const Chunk& c, uint8_t* coef,
                        uint32_t* status) {
  const Geo& g = wg.g;
  const uint32_t gt = c.k * kThreads + tid, stride = c.nchunk * kThreads;  // at most 2^28
  U4* out = reinterpret_cast<U4*>(coef);
  const U4* q = reinterpret_cast<const U4*>(g.q);
  const uint32_t nq = (uint32_t)g.ncomp * 8, nall = g.coef_bytes / 16;
  for (uint32_t j = gt; j < nall; j += stride) out[j] = j < nq ? q[j] : U4{0, 0, 0, 0};
  uint16_t* tail = reinterpret_cast<uint16_t*>(coef);  // the compact buffer is a whole number of int16
  for (uint32_t j = nall * 8 + gt; j < g.coef_bytes / 2; j += stride) tail[j] = 0;
  for (uint32_t s = gt; s < g.nseg; s += stride) {
    const Segment sg = g.segs[s];
    const uint32_t n = subs_of(sg.bits);
    const uint32_t next = s + 1 < g.nseg ? g.segs[s + 1].first_sub : g.nsub;
    const bool ok = sg.byte_off % 4 == 0 && sg.byte_off <= g.nwords * 4 - kTailPad &&
                    sg.bits <= (g.nwords * 4 - kTailPad - sg.byte_off) * 8 && sg.first_mcu == s * g.interval &&
                    (s != 0 || sg.first_sub == 0) && sg.first_sub < g.nsub && n <= g.nsub - sg.first_sub &&
                    sg.first_sub + n == next;
    if (!ok) status_max(status, kBadHeader);
  }
  if (tid == 0) w.bexit0[c.k] = w.bexit1[c.k] = kInvalid;
  if (tid >= c.n) return;
  const uint32_t i = c.first + tid;
  // the last segment that starts at or before i: right when the table holds, in [0, nseg) anyway
  uint32_t lo = 0, hi = g.nseg;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.segs[mid].first_sub <= i) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  const uint32_t next = lo + 1 < g.nseg ? g.segs[lo + 1].first_sub : g.nsub;
  if (g.segs[lo].first_sub > i || i >= next) status_max(status, kBadHeader);
  w.seg[i] = lo;
  w.aux[i] = 0;  // its own first bit, state 0
  w.exit0[i] = kInvalid;
  w.cnt[i] = kTodoW;
}

// Launch r >= 1, one thread of the chunk: take what the chunk before published in launch r - 1.
// Returns whether the entry of the chunk's first subsequence changed.
TCAMD_HD bool wide_take(const WideWs& w, const Chunk& c, uint32_t r) {
  if (c.k == 0) return false;
  const uint32_t i = c.first;
  if (w.seg[i - 1] != w.seg[i]) return false;  // the first of a segment keeps its entry
  const uint32_t e = (r & 1 ? w.bexit0 : w.bexit1)[c.k - 1];
  if ((e & kInvalid) || e == w.aux[i]) return false;
  w.aux[i] = e;
  w.cnt[i] |= kTodoW;
  return true;
}

// every launch, one thread of the chunk, after the rounds (or instead of them)
TCAMD_HD void wide_publish(const WideWs& w, const Chunk& c, uint32_t r) {
  (r & 1 ? w.bexit1 : w.bexit0)[c.k] = w.exit0[c.first + c.n - 1];
}

TCAMD_HD void wide_sync_read(uint32_t tid, const WideWs& w, const Chunk& c) {
  if (tid == 0 || tid >= c.n) return;  // the chunk's first takes its entry between launches
  const uint32_t i = c.first + tid;
  if (w.seg[i - 1] != w.seg[i]) return;
  const uint32_t e = w.exit0[i - 1];
  if (!(e & kInvalid) && e != w.aux[i]) {
    w.aux[i] = e;
    w.cnt[i] |= kTodoW;
  }
}

// returns whether this thread decoded anything
TCAMD_HD bool wide_sync_decode(uint32_t tid, const Geo& g, const HuffTab* tabs, const WideWs& w, const Chunk& c) {
  if (tid >= c.n) return false;
  const uint32_t i = c.first + tid;
  if (!(w.cnt[i] & kTodoW)) return false;
  const Span sp = wide_span_of(g, w.seg[i], i);
  const uint32_t entry = w.aux[i];
  uint32_t pos = sp.start + (entry & kRelMask), state = (entry >> kRelBits) & 511, done = 0;
  SumDc sum{g.comp_pack, 0, 0, 0};
  uint32_t rc = kBadState;
  if (pos <= sp.limit) rc = decode(g, tabs, pos, state, sp.stop, sp.limit, 0x7fffu, done, sum);
  // pos - stop < kMaxSymbolBits: the loop of decode() goes on while pos < stop
  w.exit0[i] = rc == kOk ? ((pos - sp.stop) | (state << kRelBits)) : kInvalid;
  w.cnt[i] = done;  // at most kSubBits / 2 + 1
  w.dc[3 * i + 0] = sum.s0;
  w.dc[3 * i + 1] = sum.s1;
  w.dc[3 * i + 2] = sum.s2;
  return true;
}

// ---- count: an inclusive segmented scan of kThreads Acc in `lds`, by doubling steps.  A step is
// scan_step() by every thread, a barrier, the thread's store of what it returned, a barrier.
TCAMD_HD Acc scan_step(uint32_t tid, uint32_t d, const Acc* lds) {
  return tid >= d ? combine(lds[tid - d], lds[tid]) : lds[tid];
}

TCAMD_HD Acc wide_count_load(uint32_t tid, const WideWs& w, const Chunk& c) {
  if (tid >= c.n) return Acc{0, 0, 0, 0, 0};
  const uint32_t i = c.first + tid;
  const uint32_t head = i == 0 || w.seg[i - 1] != w.seg[i] ? kHead : 0u;
  const uint32_t bad = w.exit0[i] & kInvalid ? kBad : 0u;
  return Acc{w.cnt[i] & ~kTodoW, head | bad, w.dc[3 * i + 0], w.dc[3 * i + 1], w.dc[3 * i + 2]};
}

// after the scan: the subsequence's exclusive prefix inside its chunk, and the chunk's total
TCAMD_HD void wide_count_store(uint32_t tid, const WideWs& w, const Chunk& c, const Acc* lds) {
  if (tid >= c.n) return;
  const uint32_t i = c.first + tid;
  Acc ex{0, 0, 0, 0, 0};
  if (i == 0 || w.seg[i - 1] != w.seg[i]) {
    ex.flags = kHead;  // its segment starts here: nothing before counts
  } else if (tid > 0) {
    ex = lds[tid - 1];
  }
  w.aux[i] = ex.blocks;
  w.cnt[i] = ex.flags;
  w.dc[3 * i + 0] = (int32_t)ex.dc0;  // kMaxSubDc
  w.dc[3 * i + 1] = (int32_t)ex.dc1;
  w.dc[3 * i + 2] = (int32_t)ex.dc2;
  if (tid == c.n - 1) w.ctot[c.k] = lds[tid];
}

// one workgroup per image, its chunks in tiles of kThreads: load a tile, scan it, store
TCAMD_HD Acc wide_tile_load(uint32_t tid, const WideWs& w, uint32_t base, uint32_t nchunk) {
  return base + tid < nchunk ? w.ctot[base + tid] : Acc{0, 0, 0, 0, 0};
}

// carry: the chunks before the tile
TCAMD_HD void wide_tile_store(uint32_t tid, const WideWs& w, uint32_t base, uint32_t nchunk, const Acc& carry,
                              const Acc* lds) {
  if (base + tid >= nchunk) return;
  w.cin[base + tid] = tid ? combine(carry, lds[tid - 1]) : carry;
}

struct WideStore {
  uint32_t bpm, mcux, hs, vs, comp_pack, off0, off1, off2, bw0, bw1, coef_bytes, mcus;
  uint32_t ny0, nx0, ny1, nx1;
  uint8_t* coef;
  uint32_t mcu0, first;  // the segment's first MCU, the subsequence's first block in the segment
  int32_t p0, p1, p2;
  uint32_t err;
  TCAMD_HD void operator()(uint32_t done, uint32_t blk, uint32_t nat, int val) {
    const uint32_t b = first + done;  // the block in the segment
    const uint32_t mcu = mcu0 + b / bpm;
    const uint32_t c = nibble(comp_pack, blk);
    // masks, not selects between neighbouring members (see Store)
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
    if (mcu >= mcus) {
      err = kWriteBounds;
      return;
    }
    // a coefficient the scale drops is decoded all the same: the stream fails where it fails at full size
    const uint32_t v = nat >> 3, u = nat & 7;
    const uint32_t ny = (ny0 & m0) | (ny1 & ~m0), nx = (nx0 & m0) | (nx1 & ~m0);
    if (v >= ny || u >= nx) return;
    const uint32_t mx = mcu % mcux, my = mcu / mcux;
    const uint32_t bx = c == 0 ? mx * hs + blk % hs : mx, by = c == 0 ? my * vs + blk / hs : my;
    const uint32_t first_off = (off0 & m0) | (off1 & m1) | (off2 & m2);
    const uint64_t off =
        first_off + ((uint64_t)by * ((bw0 & m0) | (bw1 & ~m0)) + bx) * (ny * nx * 2) + (v * nx + u) * 2;
    if (off + 2 > coef_bytes) {
      err = kWriteBounds;
      return;
    }
    *reinterpret_cast<int16_t*>(coef + off) = (int16_t)val;
  }
};

TCAMD_HD void wide_write(uint32_t tid, const WideGeo& wg, const HuffTab* tabs, const WideWs& w, const Chunk& c,
                         uint8_t* coef, uint32_t* status) {
  if (tid >= c.n) return;
  const Geo& g = wg.g;
  const uint32_t i = c.first + tid;
  // the prefix inside the chunk, and what the chunks before carry in when the segment began there
  Acc pre{w.aux[i], w.cnt[i], w.dc[3 * i + 0], w.dc[3 * i + 1], w.dc[3 * i + 2]};
  if (!(pre.flags & kHead)) pre = combine(w.cin[c.k], pre);
  if (pre.flags & kBad) return;  // an invalid exit earlier in the segment: nothing later is written
  const uint32_t first = pre.blocks;
  const Span sp = wide_span_of(g, w.seg[i], i);
  const uint32_t mcu0 = sp.seg * g.interval;
  const uint32_t left = g.mcus - mcu0;  // interval >= 1 and seg < nseg: mcu0 < mcus
  const uint32_t blocks = (left < g.interval ? left : g.interval) * (uint32_t)g.bpm;
  if (first >= blocks) return;  // the budget was met before this subsequence
  uint32_t pos = sp.start, state = 0, done = 0;
  if (i != sp.first_sub) {
    const uint32_t e = w.exit0[i - 1];  // valid: the prefix has no kBad
    pos = sp.start + (e & kRelMask);
    state = (e >> kRelBits) & 511;
  }
  if (pos > sp.limit) {
    status_max(status, kBadState);
    return;
  }
  // a predictor this far out fails the range check for sure
  WideStore st{(uint32_t)g.bpm, (uint32_t)g.mcux, (uint32_t)g.hs, (uint32_t)g.vs, g.comp_pack, g.off0, g.off1, g.off2,
               (uint32_t)g.bw0, (uint32_t)g.bw1, g.coef_bytes, g.mcus, wg.ny0, wg.nx0, wg.ny1, wg.nx1, coef, mcu0,
               first, saturate30(pre.dc0), saturate30(pre.dc1), saturate30(pre.dc2), kOk};
  const uint32_t rc = decode(g, tabs, pos, state, sp.stop, sp.limit, blocks - first, done, st);
  if (rc != kOk) {
    status_max(status, rc);
  } else if (st.err != kOk) {
    status_max(status, st.err);
  } else if (first + done == blocks) {
    // the RSTn rule of the host decoder: only padding, fewer than 8 bits, before the marker
    if (sp.seg + 1 < g.nseg && sp.limit - pos >= 8) status_max(status, kRestartRule);
  } else if (i == sp.last_sub) {
    status_max(status, kEndsEarly);
  }
}

}  // namespace tcamd_jhuff
