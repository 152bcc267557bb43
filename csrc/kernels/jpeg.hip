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

  // row segment y: n bytes from byte address a; head bytes up to the first aligned dword, then
  // whole dwords, then the tail bytes
  const int n = tw * NC;
  constexpr int kBody = kTileW * 3 / 4;
  for (int q = threadIdx.x; q < th * kBody; q += kBlock) {
    const int y = q / kBody, d = q - y * kBody;
    uint8_t* a = dst + ((size_t)(ty0 + y) * W + tx0) * NC;
    const int skew = (int)(reinterpret_cast<uintptr_t>(a) & 3);
    int head = (4 - skew) & 3;
    head = head < n ? head : n;
    if (d < (n - head) / 4)
      *reinterpret_cast<uint32_t*>(a + head + 4 * d) = s.rows[y * kRowDwords + (skew + head) / 4 + d];
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
