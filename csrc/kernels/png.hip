// K25 png_unfilter — the device half of a PNG decode: the filtered scanlines the
// host inflated (csrc/host/png.cc, tcamd_host_png_inflate) -> uint8 HWC pixels in
// device memory.  Reverses the None / Sub / Up / Average / Paeth prediction and
// converts the samples (palette lookup, depth 1 / 2 / 4 / 16, alpha drop) in one
// go; the arithmetic and the layout of an image's staged bytes are
// kernels/png_math.h, which the host decoder compiles too, so device and host
// pixels are equal bit for bit (contract: tests/png_cases.py).
//
// The dependency is a 2-D wavefront: a byte needs the bytes bpp to its left,
// above it and above-left.  The unit of work is bpp bytes of a row (a pixel from
// depth 8 up, a byte of 8 / depth pixels below).  One workgroup owns one image.
// Its kRowsPerPass threads take one row each, and a wave runs its 64 rows one
// unit behind each other: at step s lane l reconstructs unit s - l, with the unit
// above it coming from lane l - 1 by __shfl_up (what that lane reconstructed in
// the step before) and the unit above-left being what the lane received the step
// before.  A lane therefore holds two units of state, whatever the image.
//
// A wave sweeps kColChunk units of its rows (kColChunk + 63 steps) per phase, and
// every phase ends at a workgroup barrier.  Lane 63 leaves its units of the chunk
// in LDS, where lane 0 of the next wave reads them one phase later: wave v of a
// pass sweeps chunk q in phase v + q of that pass, and two buffers per wave,
// picked by the phase's parity, keep a chunk being written apart from the one
// being read.  The passes are pipelined the same way, T = max(chunks, waves)
// phases apart, so a wave starts the next pass's rows as soon as it is through
// with this one's.  The last row of a pass is needed up to T - 3 phases after it
// was made, which is a whole scanline and has no fixed size; it goes through one
// scanline of scratch in device memory that the staged bytes of an image of more
// than kRowsPerPass rows carry behind them (png_math.h: stage_layout), written by
// lane 63 of the last wave and read by lane 0 of the first, phases apart.  No
// wave ever waits for another by polling: every hand-over is separated by a
// barrier, and the number of barriers, passes * T + waves - 1, follows from the
// image's dimensions and is the same for every wave.  Workgroups share nothing.
// LDS (about 7 KB) and registers do not depend on the image.
//
// The reconstructed bytes are never stored at source depth, but for that one
// scanline per pass: a lane converts each unit as it completes it and stores the
// uint8 pixels to dst, byte by byte, at any alignment.  Nothing outside
// [dst, dst + h * w * channels) is written, and of src only the scratch scanline.
// A step is bound by its instructions (one wave per SIMD; loading the filtered
// bytes four steps ahead instead of one changed nothing: profiles/r15_png.md).

#include <type_traits>

#include "kernels/common.h"
#include "kernels/png_math.h"

using namespace tcamd;
using namespace tcamd_png;

namespace {

constexpr int kMaxImgs = 64;
constexpr int kWave = 64;
constexpr int kWaves = kRowsPerPass / kRowsPerWave;
static_assert(kRowsPerPass == kBlock && kRowsPerWave == kWave && kWaves >= 2, "a lane per row");

struct PngParams {
  uint8_t* src[kMaxImgs];  // the staged bytes; only the scratch scanline is written
  uint8_t* dst[kMaxImgs];
  int32_t h[kMaxImgs], w[kMaxImgs];
  uint8_t ctype[kMaxImgs], depth[kMaxImgs];
};

struct Lds {
  uint64_t hand[kWaves - 1][2][kColChunk];  // [wave][phase parity]: lane 63's units of a chunk
  uint8_t pal[kPaletteBytes];
};

template <int BPP>
using Unit = typename std::conditional<(BPP <= 4), uint32_t, uint64_t>::type;

template <int BPP>
__device__ __forceinline__ Unit<BPP> load_unit(const uint8_t* p) {
  Unit<BPP> v = 0;
#pragma unroll
  for (int k = 0; k < BPP; ++k) v |= (Unit<BPP>)p[k] << (8 * k);
  return v;
}

template <int BPP>
__device__ __forceinline__ void store_unit(uint8_t* p, Unit<BPP> v) {
#pragma unroll
  for (int k = 0; k < BPP; ++k) p[k] = (uint8_t)(v >> (8 * k));
}

template <int BPP>
__device__ __forceinline__ void unfilter_image(Lds& s, uint8_t* src, uint8_t* __restrict__ dst, int H, int W,
                                               int ctype, int depth) {
  using U = Unit<BPP>;
  const StageLayout lay = stage_layout(H, W, ctype, depth);
  const uint32_t rb = row_bytes(W, ctype, depth);
  const int nunits = (int)(rb / BPP);
  const int nchunks = (nunits + kColChunk - 1) / kColChunk;
  const int npasses = (H + kRowsPerPass - 1) / kRowsPerPass;
  const int T = nchunks > kWaves ? nchunks : kWaves;
  const int nphases = npasses * T + kWaves - 1;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int nc = out_channels(ctype);
  const int per = depth < 8 ? 8 / depth : 1;  // pixels in a unit
  uint8_t* line = src + lay.line_off;

  if (ctype == kPalette) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + lay.palette_off);
    for (int i = threadIdx.x; i < kPaletteBytes / 4; i += kBlock) reinterpret_cast<uint32_t*>(s.pal)[i] = p[i];
  }
  __syncthreads();

  U a = 0, c = 0;  // this row's last unit, and the last unit received from the row above
  int row = 0, ft = 0;
  bool live = false;
  const uint8_t* rowp = src;
  for (int P = 0; P < nphases; ++P) {
    const int pw = P - wave;
    const int pass = pw >= 0 ? pw / T : npasses, q = pw >= 0 ? pw % T : 0;
    if (pass < npasses && q < nchunks) {  // the same for the whole wave
      if (q == 0) {
        row = pass * kRowsPerPass + wave * kRowsPerWave + lane;
        live = row < H;
        a = c = 0;
        rowp = src + (size_t)(live ? row : 0) * (rb + 1);
        ft = live ? rowp[0] : 0;
      }
      const int x0 = q * kColChunk;
      const int cw = nunits - x0 < kColChunk ? nunits - x0 : kColChunk;
      const uint64_t* hand_in = wave ? s.hand[wave - 1][(P + 1) & 1] : nullptr;
      uint64_t* hand_out = wave < kWaves - 1 ? s.hand[wave][P & 1] : nullptr;
      U f_next = live && lane == 0 ? load_unit<BPP>(rowp + 1 + (size_t)x0 * BPP) : 0;
      for (int st = 0; st < cw + kWave - 1; ++st) {
        const int u = st - lane;
        const bool act = live && u >= 0 && u < cw;
        const U f = f_next;  // loaded one step ahead
        if (live && u + 1 >= 0 && u + 1 < cw) f_next = load_unit<BPP>(rowp + 1 + (size_t)(x0 + u + 1) * BPP);
        U b = __shfl_up(a, 1);  // lane - 1 reconstructed unit u of its row in the step before
        if (lane == 0) {
          b = 0;
          if (act) {
            if (wave) b = (U)hand_in[u];
            else if (pass > 0) b = load_unit<BPP>(line + (size_t)(x0 + u) * BPP);
          }
        }
        if (act) {
          const int x = x0 + u;
          U r = 0;
          uint8_t px[BPP];
#pragma unroll
          for (int k = 0; k < BPP; ++k) {
            px[k] = (uint8_t)reconstruct(ft, (int)((f >> (8 * k)) & 0xff), (int)((a >> (8 * k)) & 0xff),
                                         (int)((b >> (8 * k)) & 0xff), (int)((c >> (8 * k)) & 0xff));
            r |= (U)px[k] << (8 * k);
          }
          a = r;
          c = b;
          if (depth >= 8) {
            convert_pixel(ctype, depth, px, s.pal, dst + ((size_t)row * W + x) * nc);
          } else {
            for (int k = 0; k < per && x * per + k < W; ++k)
              convert_low(ctype, depth, low_sample(px[0], depth, k), s.pal, dst + ((size_t)row * W + x * per + k) * nc);
          }
          if (lane == kWave - 1) {
            if (hand_out) hand_out[u] = r;
            else if (row + 1 < H) store_unit<BPP>(line + (size_t)x * BPP, r);
          }
        }
      }
    }
    __syncthreads();
  }
}

// grid: x = image
__global__ void __launch_bounds__(kBlock) png_unfilter(PngParams p) {
  __shared__ __attribute__((aligned(16))) Lds s;
  const int n = blockIdx.x;
  const int H = p.h[n], W = p.w[n], ctype = p.ctype[n], depth = p.depth[n];
  switch (filter_bpp(ctype, depth)) {
    case 1: unfilter_image<1>(s, p.src[n], p.dst[n], H, W, ctype, depth); break;
    case 2: unfilter_image<2>(s, p.src[n], p.dst[n], H, W, ctype, depth); break;
    case 3: unfilter_image<3>(s, p.src[n], p.dst[n], H, W, ctype, depth); break;
    case 4: unfilter_image<4>(s, p.src[n], p.dst[n], H, W, ctype, depth); break;
    case 6: unfilter_image<6>(s, p.src[n], p.dst[n], H, W, ctype, depth); break;
    default: unfilter_image<8>(s, p.src[n], p.dst[n], H, W, ctype, depth); break;
  }
}

}  // namespace

// The kernel's decomposition, for the tests that sit on its edges: rows per
// wave, rows per pass, units (of bpp bytes) per column chunk.
extern "C" void tcamd_png_unfilter_geometry(int32_t* out3) {
  out3[0] = kRowsPerWave;
  out3[1] = kRowsPerPass;
  out3[2] = kColChunk;
}

// srcs / h / w / ctype / depth / interlace / dsts: host arrays of n_imgs entries.
// srcs[i] is a device pointer, 16-byte aligned, to image i's staged bytes in the
// layout of png_math.h (stage_layout; what tcamd_host_png_inflate writes, plus
// the scratch scanline of an image of more than kRowsPerPass rows, which the
// kernel writes); h x w is the image, ctype / depth its colour type and bit
// depth; dsts[i] is a device pointer (any alignment) to its h * w * channels
// uint8 HWC output.  One workgroup per image; images past 64 take further
// launches.  An interlaced image, a dimension outside [1, 16384], a colour
// type / depth pair the standard does not have, a null table or entry, or a
// misaligned srcs[i] is hipErrorInvalidValue before any launch.
extern "C" int tcamd_png_unfilter(void* const* srcs, const int32_t* h, const int32_t* w, const int32_t* ctype,
                                  const int32_t* depth, const int32_t* interlace, int n_imgs, void* const* dsts,
                                  void* stream) {
  if (n_imgs < 0) return hipErrorInvalidValue;
  if (n_imgs == 0) return hipSuccess;
  if (!srcs || !h || !w || !ctype || !depth || !interlace || !dsts) return hipErrorInvalidValue;
  for (int i = 0; i < n_imgs; ++i) {
    if (!srcs[i] || !dsts[i] || ((uintptr_t)srcs[i]) % 16) return hipErrorInvalidValue;
    if (h[i] < 1 || w[i] < 1 || h[i] > kMaxDim || w[i] > kMaxDim) return hipErrorInvalidValue;
    if (interlace[i] != 0 || !pair_ok(ctype[i], depth[i])) return hipErrorInvalidValue;
  }
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n_imgs; base += kMaxImgs) {
    PngParams p;
    const int cnt = n_imgs - base < kMaxImgs ? n_imgs - base : kMaxImgs;
    for (int i = 0; i < kMaxImgs; ++i) {
      const int j = base + (i < cnt ? i : 0);
      p.src[i] = static_cast<uint8_t*>(srcs[j]);
      p.dst[i] = static_cast<uint8_t*>(dsts[j]);
      p.h[i] = h[j];
      p.w[i] = w[j];
      p.ctype[i] = (uint8_t)ctype[j];
      p.depth[i] = (uint8_t)depth[j];
    }
    hipLaunchKernelGGL(png_unfilter, dim3((unsigned)cnt), dim3(kBlock), 0, s, p);
    const int rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}
