// K22 jpeg_decode — the device half of a baseline JPEG decode: dequantise, 8x8
// inverse DCT, chroma upsampling and YCbCr -> RGB of entropy-decoded
// coefficients, to uint8 HWC pixels in device memory.  The host
// (csrc/host/jpeg.cc) does the serial half, the Huffman decode, and writes per
// image the buffer this kernel reads: uint16 q[ncomp][64] in natural order,
// then each component's blocks in raster order over the MCU-padded block grid,
// 64 int16 each (csrc/host/jpeg.h).  The arithmetic is integer fixed point and
// lives in kernels/jpeg_math.h, which the host decoder compiles too, so device
// and host pixels are equal bit for bit (contract: tests/jpeg_cases.py).
//
// A workgroup owns a kTileW x kTileH tile of luma pixels of one image (grid y).
// It transforms the tile's luma blocks and the chroma blocks under the tile
// plus the one-sample halo the triangle filter reads; neighbouring workgroups
// recompute the shared chroma blocks instead of exchanging them, so the planes
// only ever exist in LDS.  Eight lanes share a block: lane r loads row r of
// the coefficients and of the quantisation table (one 16-byte load each), runs
// the 8-point row pass and writes its row of the workspace; after a barrier
// lane c reads column c and runs the column pass.  A block's workspace is 72
// dwords apart from the next, so the column reads of the four blocks in a
// 32-lane half fall on banks 8b + c + 8k: no conflicts.  kBlock / 8 = 32 blocks
// are in flight per pass; a 4:2:0 tile has 32 luma + 2 x 24 chroma blocks.
//
// Then each thread converts pixels of the tile into an LDS row buffer laid out
// like the destination: row y starts at the byte offset (address of its first
// output byte) % 4, so every aligned dword of the output row is an aligned
// dword in LDS.  Rows of 3*W bytes start anywhere; the workgroup stores the
// aligned dwords inside a row segment as dwords and the at most 3 + 3 ragged
// bytes at its ends as bytes.  Nothing outside [dst, dst + H*W*c) is written.
// LDS (about 21 KB) and registers do not depend on the image.
//
// The reduced-size decode (scale 1/2, 1/4, 1/8; contract: tests/jpeg_scaled_cases.py) is a second
// kernel, jpeg_decode_scaled, with the same tile of kTileW x kTileH output pixels, the same row
// buffer and the same stores.  Component c is transformed with an NY x NX inverse DCT of its
// lowest frequencies (jpeg_math.h: scaled_size), so every component comes out at the output
// resolution: there is no halo and no upsampling, and a tile holds (kTileW / NX) x (kTileH / NY)
// blocks of it, each NY * NX int16 in the compact buffer.  max(NY, NX) lanes share a block: lane
// r < NY loads row r (2 * NX bytes) and the first NX entries of row r of the quantisation table,
// runs the NX-point row pass and writes its row of the workspace; lane c < NX runs the NY-point
// column pass; at 1 x 1 a thread has a sample to itself.  kBlock / max(NY, NX) blocks are in
// flight per pass.  A block's workspace is NY * NX + NX dwords apart from the next (NX = 8: 72 or
// 40, 4 x 4: 20, 2 x 4: 12, 2 x 2: 6), so the ds_read_b32 column reads of a 32-lane half fall on
// 32 different banks; the two workspaces alternate between passes, which leaves one barrier per
// pass.  A call of tcamd_jpeg_decode_scaled takes images of mixed sizes, samplings and scales: the
// full-size images go to jpeg_decode as before, in launches of their own, and the images of
// scales 2, 4 and 8 share launches of jpeg_decode_scaled, which dispatches per image (grid y).
// Its LDS (about 30 KB, the second workspace) and registers do not depend on the image either.

#include <vector>

#include "kernels/common.h"
#include "kernels/jpeg_math.h"

using namespace tcamd;
using namespace tcamd_jpeg;

namespace {

constexpr int kMaxImgs = 64;
constexpr int kMaxDim = 16384;
constexpr int kTileW = 64, kTileH = 32;   // luma pixels per workgroup
constexpr int kSlots = kBlock / 8;        // blocks transformed per pass
constexpr int kWsStride = 72;             // dwords between two blocks' workspaces
constexpr int kPlaneStride = 64;          // bytes per row of a sample plane in LDS
constexpr int kRowDwords = kTileW * 3 / 4 + 1;  // an output row segment plus its start offset

enum Mode : int { kGrey = 0, k444 = 1, k422 = 2, k420 = 3 };

struct JpegParams {
  const uint8_t* src[kMaxImgs];  // quantisation tables, then coefficients
  uint8_t* dst[kMaxImgs];
  int32_t h[kMaxImgs], w[kMaxImgs];
  uint8_t mode[kMaxImgs];
};

struct Lds {
  int ws[kSlots * kWsStride];
  uint8_t plane[3][kTileH * kPlaneStride];
  uint32_t rows[kTileH * kRowDwords];
};

// The row buffer (row y of the tile at rows[y * kRowDwords], shifted by its destination's byte
// offset in a dword) -> dst.  Row segment y: n bytes from byte address a; head bytes up to the
// first aligned dword, then whole dwords, then the tail bytes.
template <int NC>
__device__ __forceinline__ void store_rows(const uint32_t* rows, uint8_t* __restrict__ dst, int W, int tx0, int ty0,
                                           int tw, int th) {
  const uint8_t* rowbuf = reinterpret_cast<const uint8_t*>(rows);
  const int n = tw * NC;
  constexpr int kBody = kTileW * 3 / 4;
  for (int q = threadIdx.x; q < th * kBody; q += kBlock) {
    const int y = q / kBody, d = q - y * kBody;
    uint8_t* a = dst + ((size_t)(ty0 + y) * W + tx0) * NC;
    const int skew = (int)(reinterpret_cast<uintptr_t>(a) & 3);
    int head = (4 - skew) & 3;
    head = head < n ? head : n;
    if (d < (n - head) / 4)
      *reinterpret_cast<uint32_t*>(a + head + 4 * d) = rows[y * kRowDwords + (skew + head) / 4 + d];
  }
  for (int q = threadIdx.x; q < th * 8; q += kBlock) {
    const int y = q >> 3, e = q & 7;
    uint8_t* a = dst + ((size_t)(ty0 + y) * W + tx0) * NC;
    const int skew = (int)(reinterpret_cast<uintptr_t>(a) & 3);
    int head = (4 - skew) & 3;
    head = head < n ? head : n;
    const int body = (n - head) / 4, tail = n - head - 4 * body;
    int k = -1;  // byte of the segment this thread stores
    if (e < 4) {
      if (e < head) k = e;
    } else if (e - 4 < tail) {
      k = head + 4 * body + e - 4;
    }
    if (k >= 0) a[k] = rowbuf[y * (kRowDwords * 4) + skew + k];
  }
}

template <int HS, int VS, int NC>
__device__ __forceinline__ void decode_tile(Lds& s, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                            int H, int W, int tile) {
  const int tiles_x = (W + kTileW - 1) / kTileW;
  const int tx0 = (tile % tiles_x) * kTileW, ty0 = (tile / tiles_x) * kTileH;
  const int mcux = (W + 8 * HS - 1) / (8 * HS), mcuy = (H + 8 * VS - 1) / (8 * VS);
  const int bw_y = mcux * HS, bh_y = mcuy * VS;

  // chroma blocks in LDS: kCbw x 4 from block (cbx0, cby0), which is one block before the tile's
  // first on a subsampled axis (the halo); blocks outside the grid are never read and are skipped
  constexpr int kCbw = HS == 2 ? 6 : 8;
  constexpr int kChroma = NC == 3 ? kCbw * 4 : 0;
  constexpr int kTotal = 32 + 2 * kChroma;
  constexpr int kPer = kChroma ? kChroma : 1;
  const int cbx0 = tx0 / HS / 8 - (HS == 2 ? 1 : 0), cby0 = ty0 / VS / 8 - (VS == 2 ? 1 : 0);

  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  for (int base = 0; base < kTotal; base += kSlots) {
    const int t = base + g;
    int c = 0, i = 0, j = 0, bx = -1, by = -1, bw = bw_y, bh = bh_y;
    size_t first = (size_t)NC * 128;  // the component's first block
    if (t < 32) {
      i = t & 7;
      j = t >> 3;
      bx = tx0 / 8 + i;
      by = ty0 / 8 + j;
    } else if (t < kTotal) {
      int u = t - 32;
      c = 1 + u / kPer;
      u -= (c - 1) * kChroma;
      i = u % kCbw;
      j = u / kCbw;
      bx = cbx0 + i;
      by = cby0 + j;
      bw = mcux;
      bh = mcuy;
      first += ((size_t)bw_y * bh_y + (size_t)(c - 1) * mcux * mcuy) * 128;
    }
    const bool valid = bx >= 0 && bx < bw && by >= 0 && by < bh;
    if (valid) {
      const uint8_t* blk = src + first + ((size_t)by * bw + bx) * 128;
      const uint4 cv = *reinterpret_cast<const uint4*>(blk + l * 16);
      const uint4 qv = *reinterpret_cast<const uint4*>(src + c * 128 + l * 16);
      const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
      int v[8], r[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = dequantise((int)(int16_t)(cw[k] & 0xffffu), (int)(qw[k] & 0xffffu));
        v[2 * k + 1] = dequantise((int)(int16_t)(cw[k] >> 16), (int)(qw[k] >> 16));
      }
      idct_row(v, r);
      int4* out = reinterpret_cast<int4*>(&s.ws[g * kWsStride + l * 8]);
      out[0] = make_int4(r[0], r[1], r[2], r[3]);
      out[1] = make_int4(r[4], r[5], r[6], r[7]);
    }
    __syncthreads();
    if (valid) {
      int col[8], smp[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) col[k] = s.ws[g * kWsStride + k * 8 + l];
      idct_col(col, smp);
      uint8_t* pl = &s.plane[c][(j * 8) * kPlaneStride + i * 8 + l];
#pragma unroll
      for (int k = 0; k < 8; ++k) pl[k * kPlaneStride] = (uint8_t)smp[k];
    }
    __syncthreads();
  }

  // pixels -> the row buffer, each row shifted by its destination's byte offset in a dword
  const int tw = W - tx0 < kTileW ? W - tx0 : kTileW, th = H - ty0 < kTileH ? H - ty0 : kTileH;
  const int cw = (W + HS - 1) / HS, ch = (H + VS - 1) / VS;
  uint8_t* rowbuf = reinterpret_cast<uint8_t*>(s.rows);
  const int x = threadIdx.x & (kTileW - 1);
  for (int y = threadIdx.x / kTileW; y < th; y += kBlock / kTileW) {
    if (x >= tw) continue;
    const size_t a = ((size_t)(ty0 + y) * W + tx0) * NC;
    uint8_t* o = rowbuf + y * (kRowDwords * 4) + (int)((reinterpret_cast<uintptr_t>(dst) + a) & 3) + x * NC;
    const int Y = s.plane[0][y * kPlaneStride + x];
    if constexpr (NC == 1) {
      o[0] = (uint8_t)Y;
    } else {
      const int ox = cbx0 * 8, oy = cby0 * 8;
      const uint8_t* pb = s.plane[1];
      const uint8_t* pr = s.plane[2];
      const int cb = chroma_up<HS, VS>(
          [&](int px, int py) { return (int)pb[(py - oy) * kPlaneStride + px - ox]; }, tx0 + x, ty0 + y, cw, ch);
      const int cr = chroma_up<HS, VS>(
          [&](int px, int py) { return (int)pr[(py - oy) * kPlaneStride + px - ox]; }, tx0 + x, ty0 + y, cw, ch);
      int rgb[3];
      ycc_to_rgb(Y, cb, cr, rgb);
      o[0] = (uint8_t)rgb[0];
      o[1] = (uint8_t)rgb[1];
      o[2] = (uint8_t)rgb[2];
    }
  }
  __syncthreads();

  store_rows<NC>(s.rows, dst, W, tx0, ty0, tw, th);
}

// grid: x = tile of the largest image's tile count, y = image
__global__ void __launch_bounds__(kBlock) jpeg_decode(JpegParams p) {
  __shared__ __attribute__((aligned(16))) Lds s;
  const int n = blockIdx.y;
  const int H = p.h[n], W = p.w[n];
  const int tiles = ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH);
  const int tile = blockIdx.x;
  if (tile >= tiles) return;  // the whole workgroup: a smaller image in a mixed launch
  switch (p.mode[n]) {
    case kGrey: decode_tile<1, 1, 1>(s, p.src[n], p.dst[n], H, W, tile); break;
    case k444: decode_tile<1, 1, 3>(s, p.src[n], p.dst[n], H, W, tile); break;
    case k422: decode_tile<2, 1, 3>(s, p.src[n], p.dst[n], H, W, tile); break;
    default: decode_tile<2, 2, 3>(s, p.src[n], p.dst[n], H, W, tile); break;
  }
}

// ---- the reduced-size decode ----------------------------------------------------------------
struct ScaledParams {
  const uint8_t* src[kMaxImgs];  // quantisation tables, then the compact coefficients
  uint8_t* dst[kMaxImgs];
  int32_t h[kMaxImgs], w[kMaxImgs];  // the output
  uint8_t mode[kMaxImgs], scale[kMaxImgs];
};

struct LdsScaled {
  int ws[2][kSlots * kWsStride];
  uint8_t plane[3][kTileH * kPlaneStride];
  uint32_t rows[kTileH * kRowDwords];
};

// N uint16 from p (2 * N-byte aligned), two to a word
template <int N>
__device__ __forceinline__ void load_u16s(const uint8_t* __restrict__ p, uint32_t* w) {
  if constexpr (N == 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else if constexpr (N == 4) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    w[0] = v.x, w[1] = v.y;
  } else if constexpr (N == 2) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  } else {
    w[0] = *reinterpret_cast<const uint16_t*>(p);
  }
}

// The tile's blocks of one component, block (bx0, by0) of its bw x bh grid first, -> its plane.
// pass counts the passes of the workgroup so far and picks the workspace.
template <int NY, int NX>
__device__ __forceinline__ void transform_blocks(LdsScaled& s, int& pass, const uint8_t* __restrict__ q,
                                                 const uint8_t* __restrict__ coef, int bw, int bh, int bx0, int by0,
                                                 uint8_t* plane) {
  constexpr int kLanes = NY > NX ? NY : NX;
  constexpr int kInFlight = kBlock / kLanes;
  constexpr int kStride = NY * NX + (NY > 1 ? NX : 0);
  constexpr int kBx = kTileW / NX, kBy = kTileH / NY;
  static_assert((kBx * kBy) % kInFlight == 0 && kInFlight * kStride <= kSlots * kWsStride, "tile and workspace");
  const int g = threadIdx.x / kLanes, l = threadIdx.x % kLanes;
  for (int base = 0; base < kBx * kBy; base += kInFlight) {
    const int t = base + g, i = t % kBx, j = t / kBx;
    const int bx = bx0 + i, by = by0 + j;
    const bool valid = bx < bw && by < bh;
    int* ws = &s.ws[pass & 1][g * kStride];
    if (valid && l < NY) {
      uint32_t cw[(NX + 1) / 2], qw[(NX + 1) / 2];
      load_u16s<NX>(coef + ((size_t)by * bw + bx) * (NY * NX * 2) + l * (NX * 2), cw);
      load_u16s<NX>(q + l * 16, qw);
      int v[NX], r[NX];
#pragma unroll
      for (int k = 0; k < NX; ++k)
        v[k] = dequantise((int)(int16_t)(cw[k / 2] >> (16 * (k & 1))), (int)((qw[k / 2] >> (16 * (k & 1))) & 0xffffu));
      idct_row_n<NX>(v, r);
#pragma unroll
      for (int k = 0; k < NX; ++k) ws[l * NX + k] = r[k];
    }
    __syncthreads();
    if (valid && l < NX) {
      int col[NY], smp[NY];
#pragma unroll
      for (int k = 0; k < NY; ++k) col[k] = ws[k * NX + l];
      idct_col_n<NY>(col, smp);
      uint8_t* pl = plane + (j * NY) * kPlaneStride + i * NX + l;
#pragma unroll
      for (int k = 0; k < NY; ++k) pl[k * kPlaneStride] = (uint8_t)smp[k];
    }
    ++pass;  // the next pass writes the other workspace: no barrier before it
  }
}

// H x W is the output; SC the scale, 2, 4 or 8
template <int HS, int VS, int NC, int SC>
__device__ __forceinline__ void decode_tile_scaled(LdsScaled& s, const uint8_t* __restrict__ src,
                                                   uint8_t* __restrict__ dst, int H, int W, int tile) {
  constexpr int N = 8 / SC;
  constexpr int NXC = N * HS < 8 ? N * HS : 8, NYC = N * VS < 8 ? N * VS : 8;  // scaled_size of chroma
  const int tiles_x = (W + kTileW - 1) / kTileW;
  const int tx0 = (tile % tiles_x) * kTileW, ty0 = (tile / tiles_x) * kTileH;
  // ceil(ceil(w / s) / (N * hs)) = ceil(w / (8 * hs)): the MCU grid of the source
  const int mcux = (W + N * HS - 1) / (N * HS), mcuy = (H + N * VS - 1) / (N * VS);
  const int bw_y = mcux * HS, bh_y = mcuy * VS;

  int pass = 0;
  size_t off = (size_t)NC * 128;
  transform_blocks<N, N>(s, pass, src, src + off, bw_y, bh_y, tx0 / N, ty0 / N, s.plane[0]);
  if constexpr (NC == 3) {
    off = (off + (size_t)bw_y * bh_y * (N * N * 2) + 15) / 16 * 16;
    transform_blocks<NYC, NXC>(s, pass, src + 128, src + off, mcux, mcuy, tx0 / NXC, ty0 / NYC, s.plane[1]);
    off = (off + (size_t)mcux * mcuy * (NYC * NXC * 2) + 15) / 16 * 16;
    transform_blocks<NYC, NXC>(s, pass, src + 256, src + off, mcux, mcuy, tx0 / NXC, ty0 / NYC, s.plane[2]);
  }
  __syncthreads();

  // pixels -> the row buffer, each row shifted by its destination's byte offset in a dword
  const int tw = W - tx0 < kTileW ? W - tx0 : kTileW, th = H - ty0 < kTileH ? H - ty0 : kTileH;
  uint8_t* rowbuf = reinterpret_cast<uint8_t*>(s.rows);
  const int x = threadIdx.x & (kTileW - 1);
  for (int y = threadIdx.x / kTileW; y < th; y += kBlock / kTileW) {
    if (x >= tw) continue;
    const size_t a = ((size_t)(ty0 + y) * W + tx0) * NC;
    uint8_t* o = rowbuf + y * (kRowDwords * 4) + (int)((reinterpret_cast<uintptr_t>(dst) + a) & 3) + x * NC;
    const int at = y * kPlaneStride + x;
    if constexpr (NC == 1) {
      o[0] = s.plane[0][at];
    } else {
      int rgb[3];
      ycc_to_rgb(s.plane[0][at], s.plane[1][at], s.plane[2][at], rgb);
      o[0] = (uint8_t)rgb[0];
      o[1] = (uint8_t)rgb[1];
      o[2] = (uint8_t)rgb[2];
    }
  }
  __syncthreads();

  store_rows<NC>(s.rows, dst, W, tx0, ty0, tw, th);
}

template <int SC>
__device__ __forceinline__ void decode_tile_mode(LdsScaled& s, int mode, const uint8_t* src, uint8_t* dst, int H,
                                                 int W, int tile) {
  switch (mode) {
    case kGrey: decode_tile_scaled<1, 1, 1, SC>(s, src, dst, H, W, tile); break;
    case k444: decode_tile_scaled<1, 1, 3, SC>(s, src, dst, H, W, tile); break;
    case k422: decode_tile_scaled<2, 1, 3, SC>(s, src, dst, H, W, tile); break;
    default: decode_tile_scaled<2, 2, 3, SC>(s, src, dst, H, W, tile); break;
  }
}

// grid: x = tile of the largest image's tile count, y = image; the scale and the sampling are
// the same for a whole workgroup
__global__ void __launch_bounds__(kBlock) jpeg_decode_scaled(ScaledParams p) {
  __shared__ __attribute__((aligned(16))) LdsScaled s;
  const int n = blockIdx.y;
  const int H = p.h[n], W = p.w[n];
  const int tiles = ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH);
  const int tile = blockIdx.x;
  if (tile >= tiles) return;
  switch (p.scale[n]) {
    case 2: decode_tile_mode<2>(s, p.mode[n], p.src[n], p.dst[n], H, W, tile); break;
    case 4: decode_tile_mode<4>(s, p.mode[n], p.src[n], p.dst[n], H, W, tile); break;
    default: decode_tile_mode<8>(s, p.mode[n], p.src[n], p.dst[n], H, W, tile); break;
  }
}

}  // namespace

// srcs / h / w / ncomp / hs / vs / dsts: host arrays of n_imgs entries.  srcs[i]
// is a device pointer, 16-byte aligned, to image i's quantisation tables and
// coefficients in the layout of csrc/host/jpeg.h; h x w is the image, ncomp 1
// or 3, hs x vs the luma sampling (1x1, 2x1 or 2x2; 1x1 for one component);
// dsts[i] is a device pointer (any alignment) to its h*w*ncomp uint8 HWC
// output.  Images past 64 take further launches.  A dimension outside
// [1, 16384], another component count or sampling, a null table or entry, or a
// misaligned srcs[i] is hipErrorInvalidValue before any launch.
extern "C" int tcamd_jpeg_decode(const void* const* srcs, const int32_t* h, const int32_t* w, const int32_t* ncomp,
                                 const int32_t* hs, const int32_t* vs, int n_imgs, void* const* dsts, void* stream) {
  if (n_imgs < 0) return hipErrorInvalidValue;
  if (n_imgs == 0) return hipSuccess;
  if (!srcs || !h || !w || !ncomp || !hs || !vs || !dsts) return hipErrorInvalidValue;
  for (int i = 0; i < n_imgs; ++i) {
    if (!srcs[i] || !dsts[i] || ((uintptr_t)srcs[i]) % 16) return hipErrorInvalidValue;
    if (h[i] < 1 || w[i] < 1 || h[i] > kMaxDim || w[i] > kMaxDim) return hipErrorInvalidValue;
    const bool grey = ncomp[i] == 1 && hs[i] == 1 && vs[i] == 1;
    const bool colour = ncomp[i] == 3 && (hs[i] == 1 || hs[i] == 2) && (vs[i] == 1 || vs[i] == 2) &&
                        !(hs[i] == 1 && vs[i] == 2);
    if (!grey && !colour) return hipErrorInvalidValue;
  }
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n_imgs; base += kMaxImgs) {
    JpegParams p;
    const int cnt = n_imgs - base < kMaxImgs ? n_imgs - base : kMaxImgs;
    int tiles = 0;
    for (int i = 0; i < kMaxImgs; ++i) {
      const int j = base + (i < cnt ? i : 0);
      p.src[i] = static_cast<const uint8_t*>(srcs[j]);
      p.dst[i] = static_cast<uint8_t*>(dsts[j]);
      p.h[i] = h[j];
      p.w[i] = w[j];
      p.mode[i] = (uint8_t)(ncomp[j] == 1 ? kGrey : (hs[j] == 1 ? k444 : (vs[j] == 1 ? k422 : k420)));
      const int t = ((w[j] + kTileW - 1) / kTileW) * ((h[j] + kTileH - 1) / kTileH);
      if (i < cnt && t > tiles) tiles = t;
    }
    hipLaunchKernelGGL(jpeg_decode, dim3((unsigned)tiles, (unsigned)cnt), dim3(kBlock), 0, s, p);
    const int rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

// The reduced-size decode: as tcamd_jpeg_decode, and scale[i] is 1, 2, 4 or 8,
// h[i] x w[i] the output (ceil(H / scale) x ceil(W / scale)), srcs[i] the
// compact coefficient buffer of that scale (csrc/host/jpeg.h), ny / nx host
// arrays of 3 * n_imgs entries, component c of image i at [3 * i + c], which
// must be what the scale and the sampling give (jpeg_math.h: scaled_size).
// Images of mixed sizes, samplings and scales share a call: those of scale 1
// go through tcamd_jpeg_decode, unchanged, in launches of their own; the others
// share launches of jpeg_decode_scaled, 64 images each, which dispatches per
// image.  Another scale or transform size, or anything tcamd_jpeg_decode
// refuses, is hipErrorInvalidValue before any launch.
extern "C" int tcamd_jpeg_decode_scaled(const void* const* srcs, const int32_t* h, const int32_t* w,
                                        const int32_t* ncomp, const int32_t* hs, const int32_t* vs,
                                        const int32_t* scale, const int32_t* ny, const int32_t* nx, int n_imgs,
                                        void* const* dsts, void* stream) {
  if (n_imgs < 0) return hipErrorInvalidValue;
  if (n_imgs == 0) return hipSuccess;
  if (!srcs || !h || !w || !ncomp || !hs || !vs || !scale || !ny || !nx || !dsts) return hipErrorInvalidValue;
  std::vector<int> full, reduced;
  for (int i = 0; i < n_imgs; ++i) {
    if (!srcs[i] || !dsts[i] || ((uintptr_t)srcs[i]) % 16) return hipErrorInvalidValue;
    if (h[i] < 1 || w[i] < 1 || h[i] > kMaxDim || w[i] > kMaxDim) return hipErrorInvalidValue;
    const bool grey = ncomp[i] == 1 && hs[i] == 1 && vs[i] == 1;
    const bool colour = ncomp[i] == 3 && (hs[i] == 1 || hs[i] == 2) && (vs[i] == 1 || vs[i] == 2) &&
                        !(hs[i] == 1 && vs[i] == 2);
    if ((!grey && !colour) || !scale_ok(scale[i])) return hipErrorInvalidValue;
    for (int c = 0; c < ncomp[i]; ++c) {
      if (ny[3 * i + c] != scaled_size(scale[i], vs[i], c ? 1 : vs[i]) ||
          nx[3 * i + c] != scaled_size(scale[i], hs[i], c ? 1 : hs[i]))
        return hipErrorInvalidValue;
    }
    (scale[i] == 1 ? full : reduced).push_back(i);
  }
  if (!full.empty()) {
    std::vector<const void*> fs;
    std::vector<void*> fd;
    std::vector<int32_t> fh, fw, fn, fhs, fvs;
    for (int i : full) {
      fs.push_back(srcs[i]);
      fd.push_back(dsts[i]);
      fh.push_back(h[i]);
      fw.push_back(w[i]);
      fn.push_back(ncomp[i]);
      fhs.push_back(hs[i]);
      fvs.push_back(vs[i]);
    }
    const int rc = tcamd_jpeg_decode(fs.data(), fh.data(), fw.data(), fn.data(), fhs.data(), fvs.data(),
                                     (int)full.size(), fd.data(), stream);
    if (rc != hipSuccess) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  const int n_red = (int)reduced.size();
  for (int base = 0; base < n_red; base += kMaxImgs) {
    ScaledParams p;
    const int cnt = n_red - base < kMaxImgs ? n_red - base : kMaxImgs;
    int tiles = 0;
    for (int i = 0; i < kMaxImgs; ++i) {
      const int j = reduced[base + (i < cnt ? i : 0)];
      p.src[i] = static_cast<const uint8_t*>(srcs[j]);
      p.dst[i] = static_cast<uint8_t*>(dsts[j]);
      p.h[i] = h[j];
      p.w[i] = w[j];
      p.mode[i] = (uint8_t)(ncomp[j] == 1 ? kGrey : (hs[j] == 1 ? k444 : (vs[j] == 1 ? k422 : k420)));
      p.scale[i] = (uint8_t)scale[j];
      const int t = ((w[j] + kTileW - 1) / kTileW) * ((h[j] + kTileH - 1) / kTileH);
      if (i < cnt && t > tiles) tiles = t;
    }
    hipLaunchKernelGGL(jpeg_decode_scaled, dim3((unsigned)tiles, (unsigned)cnt), dim3(kBlock), 0, s, p);
    const int rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}
