// The index rule of K11x's 3x3 phase (kernels/x3_ring_math.h) as a stand-alone
// program, meant for a sanitizer build too (`make asan` builds it as
// build-asan/bin/x3_ring_test):
//
//   x3_ring_test
//
// Host code only; nothing of it runs on a GPU.  For every W in 16..56 and H in
// 1..57, with M = three images plus a ragged end (M % 64 != 0):
//   * from every tile of the pixel list as a block's first tile, the state
//     carried tile by tile (x3r_advance) equals the state division gives for
//     that tile (x3r_first), up to the last tile;
//   * for every tile, from the carried state, every lane's 4 pixel groups: x,
//     y, ring position, the in-image and edge flags and the 12 row addresses
//     equal what division gives for that pixel, written out here the way the
//     kernels computed it before they carried anything (per-pixel division,
//     logical ring rows, the zero row for a tap row outside the image);
//   * every tap address (row address + the dx immediate) equals the address
//     the earlier per-step arithmetic formed, or both lie in the zero rows
//     with the whole 16-B read of both planes inside them.
// The row functions depend on the tile state and the lane alone, so they are
// run for the walk from tile 0 and at every walk's first tile, not for every
// (first tile, tile) pair.  Exits 0 when all held; the last line of the output
// ends " 0 failures".

#include <cstdint>
#include <cstdio>

#include "../../kernels/x3_ring_math.h"

namespace {

long g_checks = 0;
long g_failures = 0;

#define CHECK(cond, ...)                \
  do {                                  \
    ++g_checks;                         \
    if (!(cond)) {                      \
      if (++g_failures <= 20) {         \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);       \
        std::printf("\n");              \
      }                                 \
    }                                   \
  } while (0)

using namespace x3r;

constexpr uint32_t kZeroLo = kZeroRow * kRowBytes, kZeroHi = (kZeroRow + 3) * kRowBytes;

// a 16-B read of both planes at `a` (relative to the ring) stays in the zero rows
bool in_zero_rows(uint32_t a) { return a >= kZeroLo && a + kLoPlane + 16 <= kZeroHi; }

void check_rows(const X3Tile& t, int m0, int M, int H, int W, uint32_t ring, uint32_t chunk16) {
  const uint32_t cbase = ring + chunk16, zero = ring + kZeroLo;
  const int HW = H * W;
  for (int l15 = 0; l15 < 16; ++l15) {
    X3Rows r;
    x3r_rows<true>(t, m0, l15, M, H, W, cbase, zero, r);
    for (int pg = 0; pg < 4; ++pg) {
      // the pixel by division
      const int m = m0 + 16 * pg + l15;
      const int x = (m % HW) % W, y = (m % HW) / W, pos = (m + W + 1) % kRing;
      const bool in = m < M;
      CHECK(r.x[pg] == x && r.y[pg] == y && r.pos[pg] == pos, "W %d H %d m %d: x %d/%d y %d/%d pos %d/%d", W, H, m,
            r.x[pg], x, r.y[pg], y, r.pos[pg], pos);
      CHECK(r.in[pg] == in && r.lf[pg] == (x > 0) && r.rt[pg] == (x < W - 1), "W %d H %d m %d: flags", W, H, m);
      // logical rows as the kernels formed them: kZeroRow stands for "zeros"
      const int rm = pos - W, rp = pos + W;
      const int R[3] = {(in && y > 0) ? (rm < 0 ? rm + kRing : rm) : kZeroRow, in ? pos : kZeroRow,
                        (in && y < H - 1) ? (rp >= kRing ? rp - kRing : rp) : kZeroRow};
      for (int dy = 0; dy < 3; ++dy) {
        const uint32_t want = R[dy] == kZeroRow ? zero : cbase + (uint32_t)R[dy] * kRowBytes;
        CHECK(r.off[pg][dy] == want, "W %d H %d m %d dy %d: off %u want %u", W, H, m, dy, r.off[pg][dy], want);
        for (int dxi = 0; dxi < 3; ++dxi) {
          const int dx = dxi - 1;
          // the earlier per-step form: physical row = logical + 1
          int off = (R[dy] + dx) * kRowBytes + (int)chunk16;
          if (dx < 0 && !(x > 0)) off = kZeroRow * kRowBytes;
          if (dx > 0 && !(x < W - 1)) off = kZeroRow * kRowBytes;
          const uint32_t old_a = (uint32_t)(kRowBytes + off);
          const uint32_t new_a = x3r_tap(r, pg, dy, dxi, zero) + (uint32_t)dxi * kRowBytes - ring;
          CHECK(new_a == old_a || (in_zero_rows(new_a) && in_zero_rows(old_a)),
                "W %d H %d m %d tap (%d, %d): address %u, was %u", W, H, m, dy, dx, new_a, old_a);
          CHECK(new_a + kLoPlane + 16 <= (uint32_t)(kZeroRow + 3) * kRowBytes, "W %d H %d m %d: past the ring", W, H, m);
        }
      }
    }
  }
}

}  // namespace

int main() {
  for (int W = 16; W <= 56; ++W) {
    for (int H = 1; H <= 57; ++H) {
      int M = 3 * H * W + 37;
      if (M % kTile == 0) ++M;
      const int tiles = (M + kTile - 1) / kTile;
      const X3Step step = x3r_step(H, W);
      CHECK(step.dx == kTile % W && step.dy == (kTile / W) % H, "W %d H %d: step", W, H);
      for (int first = 0; first < tiles; ++first) {
        X3Tile t = x3r_first(first * kTile, H, W);
        for (int tile = first; tile < tiles; ++tile) {
          const int m0 = tile * kTile;
          const X3Tile d = x3r_first(m0, H, W);
          CHECK(t.x == d.x && t.y == d.y && t.pos == d.pos, "W %d H %d first %d tile %d: carried (%d, %d, %d), (%d, %d, %d)",
                W, H, first, tile, t.x, t.y, t.pos, d.x, d.y, d.pos);
          CHECK(d.x == (m0 % (H * W)) % W && d.y == (m0 % (H * W)) / W, "W %d H %d tile %d: first", W, H, tile);
          if (first == 0 || tile == first)
            check_rows(t, m0, M, H, W, (tile & 1) ? 1024u : 0u, (uint32_t)((tile * 7 + first) & 15) << 4);
          x3r_advance(t, step, H, W);
        }
      }
    }
  }
  std::printf("x3_ring_test: %ld checks, %ld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
