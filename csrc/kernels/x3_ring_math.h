// The index rule of K11x's 3x3 phase (csrc/kernels/densenet_x3.hip,
// x3_dense_fused_kernel and x3_dense_fused3_kernel), compiled for the host and
// the device so that csrc/cpp/tests/x3_ring_test.cc can check it exhaustively.
//
// A block walks contiguous 64-pixel tiles of the [imgs][H][W] pixel list; tile
// m0's 3x3 reads the band [m0 - W - 1, m0 + 64 + W + 1) from a ring of kRing
// logical rows, pixel m in logical row (m + W + 1) % kRing.  A ring row is
// kRowBytes bytes (hi plane | lo plane at +kLoPlane | padding); physical row =
// logical + 1, the two guard rows mirror logical kRing - 1 and 0, and the
// physical rows kZeroRow .. kZeroRow + 2 hold zeros.
//
// What a tile needs is known from its first pixel alone, which is the same for
// every lane of the block: X3Tile = (x, y) of pixel m0 in its image and its
// ring position.  x3r_advance carries that 64 pixels on with additions and
// compares only (the steps 64 % W and (64 / W) % H are per-block constants),
// so only a block's first tile divides.  Being uniform, the carried state
// lives in scalar registers and costs the vector pipe nothing.
//
// x3r_rows turns the state into what a lane reads: for each of its 4 pixel
// groups (pixels m0 + 16 pg + l15) and each tap row dy, the LDS byte address
// of the dx = -1 operand, with the ring stride, the lane's 16-B chunk and the
// ring's LDS base folded in (`cbase`).  dx is then an immediate: the operands
// of tap (dy, dx) are at
//     off[pg][dy] + (dx + 1) * kRowBytes        (hi plane)
//     off[pg][dy] + (dx + 1) * kRowBytes + kLoPlane
// A tap row outside the image, or a pixel past M, has the address of the first
// zero row instead, whose three rows absorb dx.  At the image's left / right
// edge (lf / rt false) the dx = -1 / +1 tap reads zeros: one select between
// off[pg][dy] and `zero` (x3r_tap).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define X3R_HD __host__ __device__ __forceinline__
#else
#define X3R_HD inline
#endif

namespace x3r {

constexpr int kRing = 192;      // logical ring rows
constexpr int kZeroRow = 194;   // first of the three zero rows (physical)
constexpr int kRowBytes = 544;  // ring row stride
constexpr int kLoPlane = 256;   // the lo plane within a row
constexpr int kTile = 64;       // pixels per tile
constexpr int kRingBytes = kRing * kRowBytes;

// pixel m0 (the tile's first): x = m0 % W, y = (m0 / W) % H, pos = (m0 + W + 1) % kRing
struct X3Tile {
  int x, y, pos;
};

// what one tile step adds, per block
struct X3Step {
  int dx, dy;  // 64 % W, (64 / W) % H
};

X3R_HD X3Step x3r_step(int H, int W) { return X3Step{kTile % W, (kTile / W) % H}; }

// the state of tile m0 by division (a block's first tile; the test's reference)
X3R_HD X3Tile x3r_first(int m0, int H, int W) {
  return X3Tile{m0 % W, (m0 / W) % H, (m0 + W + 1) % kRing};
}

// tile m0 -> tile m0 + 64
X3R_HD void x3r_advance(X3Tile& t, const X3Step& s, int H, int W) {
  t.x += s.dx;
  int c = 0;
  if (t.x >= W) {
    t.x -= W;
    c = 1;
  }
  t.y += s.dy + c;  // < 2H: one wrap
  if (t.y >= H) t.y -= H;
  t.pos += kTile;
  if (t.pos >= kRing) t.pos -= kRing;
}

struct X3Rows {
  int x[4], y[4], pos[4];  // of pixel m0 + 16 pg + l15 (pos: its logical ring row)
  bool in[4];              // pixel < M
  bool lf[4], rt[4];       // x > 0, x < W - 1
  uint32_t off[4][3];      // see above
};

// Lane l15 (0..15) of a tile.  cbase = the ring's LDS address + the lane's
// 16-B chunk offset; zero = the ring's LDS address + kZeroRow * kRowBytes.
// W >= 16, so 16 pixels on wrap an image row at most once.  KEEP = false
// leaves x / y / pos / in unwritten (the kernel reads only off, lf and rt).
template <bool KEEP = true>
X3R_HD void x3r_rows(const X3Tile& t, int m0, int l15, int M, int H, int W, uint32_t cbase, uint32_t zero, X3Rows& r) {
  int x = t.x + l15, y = t.y, pos = t.pos + l15;
  if (x >= W) {
    x -= W;
    if (++y == H) y = 0;
  }
  if (pos >= kRing) pos -= kRing;
#if defined(__HIP_DEVICE_COMPILE__)
  int pb = __mul24(pos, kRowBytes);  // the only multiply of a tile, full rate
#else
  int pb = pos * kRowBytes;
#endif
  const int wb = W * kRowBytes;
  const int m = m0 + l15;
#if defined(__clang__)
#pragma unroll
#endif
  for (int pg = 0; pg < 4; ++pg) {
    if (pg) {
      x += 16;
      if (x >= W) {
        x -= W;
        if (++y == H) y = 0;
      }
      pb += 16 * kRowBytes;
      if (pb >= kRingBytes) pb -= kRingBytes;
    }
    const bool in = m + 16 * pg < M;
    int up = pb - wb, dn = pb + wb;
    if (up < 0) up += kRingBytes;
    if (dn >= kRingBytes) dn -= kRingBytes;
    r.off[pg][0] = (in && y > 0) ? cbase + (uint32_t)up : zero;
    r.off[pg][1] = in ? cbase + (uint32_t)pb : zero;
    r.off[pg][2] = (in && y < H - 1) ? cbase + (uint32_t)dn : zero;
    r.lf[pg] = x > 0;
    r.rt[pg] = x < W - 1;
    if (KEEP) {
      r.x[pg] = x;
      r.y[pg] = y;
      r.pos[pg] = pb / kRowBytes;
      r.in[pg] = in;
    }
  }
}

// the address tap (dy, dxi = dx + 1) of pixel group pg reads at, before the
// immediate (dxi * kRowBytes, + kLoPlane for the lo plane)
X3R_HD uint32_t x3r_tap(const X3Rows& r, int pg, int dy, int dxi, uint32_t zero) {
  uint32_t a = r.off[pg][dy];
  if (dxi == 0 && !r.lf[pg]) a = zero;
  if (dxi == 2 && !r.rt[pg]) a = zero;
  return a;
}

}  // namespace x3r
