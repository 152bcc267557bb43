// K20 resize_pack — bilinear resize + channel adapt + per-channel affine +
// dtype convert + layout pack of raw uint8 HWC images, each of its own size,
// into model input tensors.  The device form of
// triton_client_amd/utils/image.py::preprocess (reference
// src/python/examples/image_client.py:154-194), so a raw image can go to the
// GPU at one byte per element and never be resampled on the host.
//
//   y_n[c, i, j] = bilinear(x_n)[i, j, c] * scale[c] + bias[c]
//
// Sampling uses half-pixel centres, no antialiasing, clamped indices.  The
// source coordinate of output index i on an axis n_in -> n_out is computed in
// integers (resize_axis_table in utils/image.py is the same rule in numpy):
//   num = (2i+1)*n_in - n_out, den = 2*n_out, i0 = floor(num/den),
//   frac = (num - i0*den) / den
// and after the clamp i0 < 0 gives weight 0, i0 > n_in-1 weight 1.  Every
// dimension is at most 16384, so num fits 32 bits; an fp32 coordinate would
// lose 5e-4 near 4096, which is 0.1 on a 255 step between neighbours.
//
// One thread produces 4 consecutive output pixels of one row for every
// channel: the row terms are computed once, the taps are byte loads (source
// pointers may have any alignment: a blob's pixels start 10 or ~15 bytes in),
// and the 4 outputs per channel plane (NCHW) or the 4*C interleaved outputs
// (NHWC) leave as 16-byte (fp32) / 8-byte (16-bit) stores when W % 4 == 0 and
// every destination is 16-byte aligned.  Anything else takes the same kernel
// with guarded scalar stores.  Up to 64 images per launch, described by a
// table passed by value as K6 does.
//
// K20 does not antialias: at a downscale ratio r it still reads 2x2 source
// pixels per output and skips the rest.  K21 resize_pack_aa below is the
// antialiased form, with the same arguments, adapt, affine, dtypes and layouts.
//
// K21 resize_pack_aa — the triangle filter widened by the downscale ratio
// (support max(1, n_in/n_out) per axis, renormalised at the borders), the
// device form of utils/image.py::resize_area.  Per axis n_in -> n_out, in
// integers (area_axis_table in utils/image.py is the same rule in numpy):
//   D = 2*max(n_in, n_out),  t(i, j) = D - |(2j+1)*n_out - (2i+1)*n_in|,
//   out[i] = sum_j t(i, j) * src[j] / sum_j t(i, j)   over the j with t > 0
// so an upscaled axis has K20's two taps and weights.  The integer taps are
// accumulated with fma and the sum is divided by the integer total once, so a
// pass rounds once per tap and twice at the end; up to 16384 every term fits
// 32 bits (the largest total is 402,653,184 at 16384 -> 1).
//
// Separable, staged through LDS.  A workgroup owns kAaBand output rows x
// kAaTile output columns of one image, lane = column, wave = row lane.  The
// source rows under the band's vertical footprint pass through a slab of
// kAaChunk rows: each wave filters whole source rows horizontally (byte loads,
// lanes along x) into slab[row][channel][column], then every thread walks the
// slab rows under its own output rows and accumulates them in registers.
// Neighbouring output rows share most of their source rows, which the slab
// filters once.  The tap loops are run-time loops and the footprint streams
// through the slab chunk by chunk, so 2 taps and 16384 taps use the same
// registers and LDS.  Slab writes and reads are 64 consecutive dwords per
// wave: no bank conflicts.  The finished tile goes through a second LDS
// array laid out in destination order (NHWC writes it at a stride of 3
// dwords, conflict-free) so that the stores are K20's: 16-byte (fp32) /
// 8-byte (16-bit) vectors when W % 4 == 0 and every destination is 16-byte
// aligned, guarded scalar stores otherwise.

#include "kernels/common.h"

using namespace tcamd;

namespace {

constexpr int kMaxImgs = 64;
constexpr int kMaxDim = 16384;
constexpr int kPix = 4;  // output pixels per thread

struct ResizeParams {
  const uint8_t* src[kMaxImgs];
  void* dst[kMaxImgs];
  int32_t h[kMaxImgs], w[kMaxImgs];
  uint8_t c[kMaxImgs];
  float scale[3], bias[3];
  int H, W;
  int rne;  // bf16 rounding
};

struct Axis {
  int i0, i1;
  float w;
};

__device__ __forceinline__ Axis axis_term(int i, int n_in, int n_out) {
  const int num = (2 * i + 1) * n_in - n_out, den = 2 * n_out;
  int i0 = num >= 0 ? num / den : -1;  // num > -n_out, so floor(num/den) is -1 below zero
  Axis a;
  a.w = (float)(num - i0 * den) / (float)den;
  if (i0 < 0) {
    i0 = 0;
    a.w = 0.f;
  } else if (i0 > n_in - 1) {
    i0 = n_in - 1;
    a.w = 1.f;
  }
  a.i0 = i0;
  a.i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
  return a;
}

template <int DT>
__device__ __forceinline__ uint32_t bits16(float f, int rne) {
  if constexpr (DT == kBF16) return rne ? f32_to_bf16_rne(f) : f32_to_bf16_trunc(f);
  else {
    _Float16 h = (_Float16)f;
    return *reinterpret_cast<uint16_t*>(&h);
  }
}

// 4 consecutive outputs at element e of dst (vector form: e % 4 == 0, dst 16-byte aligned)
template <int DT>
__device__ __forceinline__ void st4(void* dst, size_t e, const float* f, int rne) {
  if constexpr (DT == kFP32) {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(dst) + e) = make_float4(f[0], f[1], f[2], f[3]);
  } else {
    const uint32_t a = bits16<DT>(f[0], rne) | (bits16<DT>(f[1], rne) << 16);
    const uint32_t b = bits16<DT>(f[2], rne) | (bits16<DT>(f[3], rne) << 16);
    *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(dst) + e) = make_uint2(a, b);
  }
}

template <int DT>
__device__ __forceinline__ void st1(void* dst, size_t e, float f, int rne) {
  if constexpr (DT == kFP32) reinterpret_cast<float*>(dst)[e] = f;
  else reinterpret_cast<uint16_t*>(dst)[e] = (uint16_t)bits16<DT>(f, rne);
}

// grid: x = groups of kBlock threads over (row, 4-pixel group), y = image
template <int DT, int C, bool NHWC, bool VEC>
__global__ void __launch_bounds__(kBlock) resize_pack(ResizeParams p) {
  const int n = blockIdx.y;
  const int H = p.H, W = p.W;
  const int xq = (W + kPix - 1) / kPix;
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= (int64_t)H * xq) return;
  const int y = (int)(q / xq);
  const int x_first = (int)(q - (int64_t)y * xq) * kPix;
  const int ih = p.h[n], iw = p.w[n], sc = p.c[n];
  const uint8_t* src = p.src[n];
  void* dst = p.dst[n];

  const Axis ay = axis_term(y, ih, H);
  const uint8_t* row0 = src + (size_t)ay.i0 * iw * sc;
  const uint8_t* row1 = src + (size_t)ay.i1 * iw * sc;

  float o[C][kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const int x = x_first + k < W ? x_first + k : W - 1;  // a tail lane resamples the last pixel and stores nothing
    const Axis ax = axis_term(x, iw, W);
    const size_t o0 = (size_t)ax.i0 * sc, o1 = (size_t)ax.i1 * sc;
    // source channels after the adapt: 3 -> 1 is (r+g+b)/3 per tap, 1 -> 3 repeats
    float v[C];
    if (sc == C) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float a = (float)row0[o0 + c], b = (float)row0[o1 + c];
        const float d = (float)row1[o0 + c], e = (float)row1[o1 + c];
        const float top = a * (1.f - ax.w) + b * ax.w;
        const float bot = d * (1.f - ax.w) + e * ax.w;
        v[c] = top * (1.f - ay.w) + bot * ay.w;
      }
    } else {
      float a, b, d, e;
      if (sc == 3) {
        a = ((float)row0[o0] + (float)row0[o0 + 1] + (float)row0[o0 + 2]) / 3.f;
        b = ((float)row0[o1] + (float)row0[o1 + 1] + (float)row0[o1 + 2]) / 3.f;
        d = ((float)row1[o0] + (float)row1[o0 + 1] + (float)row1[o0 + 2]) / 3.f;
        e = ((float)row1[o1] + (float)row1[o1 + 1] + (float)row1[o1 + 2]) / 3.f;
      } else {
        a = (float)row0[o0];
        b = (float)row0[o1];
        d = (float)row1[o0];
        e = (float)row1[o1];
      }
      const float top = a * (1.f - ax.w) + b * ax.w;
      const float bot = d * (1.f - ax.w) + e * ax.w;
      const float r = top * (1.f - ay.w) + bot * ay.w;
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = r;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) o[c][k] = v[c] * p.scale[c] + p.bias[c];
  }

  const size_t pix = (size_t)y * W + x_first;
  if constexpr (VEC) {
    if constexpr (NHWC) {
      float f[C * kPix];
#pragma unroll
      for (int k = 0; k < kPix; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) f[k * C + c] = o[c][k];
#pragma unroll
      for (int j = 0; j < C; ++j) st4<DT>(dst, pix * C + 4 * j, f + 4 * j, p.rne);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) st4<DT>(dst, (size_t)c * H * W + pix, o[c], p.rne);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      if (x_first + k < W) {
#pragma unroll
        for (int c = 0; c < C; ++c)
          st1<DT>(dst, NHWC ? (pix + k) * C + c : (size_t)c * H * W + pix + k, o[c][k], p.rne);
      }
    }
  }
}

// ---- K21 resize_pack_aa ---------------------------------------------------------
constexpr int kAaTile = 64;                  // output columns per workgroup: the lanes of a wave
constexpr int kAaBand = 8;                   // output rows per workgroup
constexpr int kAaChunk = 16;                 // source rows in the LDS slab
constexpr int kAaWaves = kBlock / kAaTile;   // row lanes
constexpr int kAaRows = kAaBand / kAaWaves;  // output rows per thread

// the source indices [lo, hi] with t > 0 for one output index, and what t needs
struct Taps {
  int lo, hi;
  int c, D;  // (2i+1)*n_in, 2*max(n_in, n_out)
};

__device__ __forceinline__ Taps aa_taps(int i, int n_in, int n_out) {
  Taps a;
  a.D = 2 * (n_in > n_out ? n_in : n_out);
  a.c = (2 * i + 1) * n_in;
  const int den = 2 * n_out;
  const int below = a.c - a.D - n_out;  // t(j) > 0  <=>  below < j*den < c + D - n_out
  a.lo = below >= 0 ? below / den + 1 : 0;
  const int hi = (a.c + a.D - n_out - 1) / den;
  a.hi = hi < n_in - 1 ? hi : n_in - 1;
  return a;
}

__device__ __forceinline__ int aa_t(const Taps& a, int j, int n_out) {
  const int v = (2 * j + 1) * n_out - a.c;
  return a.D - (v < 0 ? -v : v);
}

// grid: x = (band of kAaBand output rows, tile of kAaTile output columns), y = image
template <int DT, int C, bool NHWC, bool VEC>
__global__ void __launch_bounds__(kBlock) resize_pack_aa(ResizeParams p) {
  __shared__ float slab[kAaChunk][C][kAaTile];
  __shared__ __attribute__((aligned(16))) float tile[kAaBand * C * kAaTile];  // the outputs, in destination order
  const int n = blockIdx.y;
  const int H = p.H, W = p.W;
  const int tiles = (W + kAaTile - 1) / kAaTile;
  const int band0 = (int)(blockIdx.x / tiles) * kAaBand;
  const int x0 = (int)(blockIdx.x % tiles) * kAaTile;
  const int lane = threadIdx.x % kAaTile, wave = threadIdx.x / kAaTile;
  const int ih = p.h[n], iw = p.w[n], sc = p.c[n];
  const uint8_t* src = p.src[n];
  void* dst = p.dst[n];
  // channels after the adapt that are filtered: 3 -> 1 filters the mean, 1 -> 3 repeats at the end
  const int cs = sc == C ? C : 1;

  // a lane past the last column or row resamples the last one; the stores leave it out
  const Taps tx = aa_taps(x0 + lane < W ? x0 + lane : W - 1, iw, W);
  Taps ty[kAaRows];
  float acc[kAaRows][C];
  int sy[kAaRows];
#pragma unroll
  for (int m = 0; m < kAaRows; ++m) {
    const int i = band0 + wave + m * kAaWaves;
    ty[m] = aa_taps(i < H ? i : H - 1, ih, H);
    sy[m] = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[m][c] = 0.f;
  }
  const int rows = H - band0 < kAaBand ? H - band0 : kAaBand;
  const int r_first = aa_taps(band0, ih, H).lo, r_last = aa_taps(band0 + rows - 1, ih, H).hi;

  // the band's source rows [r_first, r_last], kAaChunk at a time; every bound here is the workgroup's
  for (int r0 = r_first; r0 <= r_last; r0 += kAaChunk) {
    for (int rr = wave; rr < kAaChunk && r0 + rr <= r_last; rr += kAaWaves) {
      const uint8_t* row = src + (size_t)(r0 + rr) * iw * sc;
      float a[C];
#pragma unroll
      for (int c = 0; c < C; ++c) a[c] = 0.f;
      int s = 0;
      if (sc == C) {
        for (int j = tx.lo; j <= tx.hi; ++j) {
          const int t = aa_t(tx, j, W);
          s += t;
#pragma unroll
          for (int c = 0; c < C; ++c) a[c] = fmaf((float)t, (float)row[(size_t)j * C + c], a[c]);
        }
      } else if (sc == 3) {
        for (int j = tx.lo; j <= tx.hi; ++j) {
          const int t = aa_t(tx, j, W);
          s += t;
          const uint8_t* px = row + (size_t)j * 3;
          a[0] = fmaf((float)t, (float)((int)px[0] + (int)px[1] + (int)px[2]), a[0]);
        }
        a[0] /= 3.f;
      } else {
        for (int j = tx.lo; j <= tx.hi; ++j) {
          const int t = aa_t(tx, j, W);
          s += t;
          a[0] = fmaf((float)t, (float)row[j], a[0]);
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < cs) slab[rr][c][lane] = a[c] / (float)s;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kAaRows; ++m) {
      const int ra = ty[m].lo > r0 ? ty[m].lo : r0;
      const int rb = ty[m].hi < r0 + kAaChunk - 1 ? ty[m].hi : r0 + kAaChunk - 1;
      for (int r = ra; r <= rb; ++r) {
        const int t = aa_t(ty[m], r, H);
        sy[m] += t;
#pragma unroll
        for (int c = 0; c < C; ++c)
          if (c < cs) acc[m][c] = fmaf((float)t, slab[r - r0][c][lane], acc[m][c]);
      }
    }
    __syncthreads();
  }

  // NCHW: segment (row, channel) of kAaTile floats; NHWC: segment (row) of kAaTile*C floats
#pragma unroll
  for (int m = 0; m < kAaRows; ++m) {
    const int lr = wave + m * kAaWaves;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float v = acc[m][c < cs ? c : 0] / (float)sy[m];
      tile[NHWC ? (lr * kAaTile + lane) * C + c : (lr * C + c) * kAaTile + lane] = v * p.scale[c] + p.bias[c];
    }
  }
  __syncthreads();
  const int tw = W - x0 < kAaTile ? W - x0 : kAaTile;
  const int nseg = NHWC ? rows : rows * C, seglen = NHWC ? tw * C : tw;
  constexpr int kSegMax = NHWC ? kAaTile * C : kAaTile;
  constexpr int kStep = VEC ? 4 : 1;  // VEC: tw % 4 == 0
  const int per = seglen / kStep;
  for (int q = threadIdx.x; q < nseg * per; q += kBlock) {
    const int seg = q / per, k = (q - seg * per) * kStep;
    const size_t e = NHWC ? ((size_t)(band0 + seg) * W + x0) * C + k
                          : (size_t)(seg % C) * H * W + (size_t)(band0 + seg / C) * W + x0 + k;
    const float* f = tile + seg * kSegMax + k;
    if constexpr (VEC) st4<DT>(dst, e, f, p.rne);
    else st1<DT>(dst, e, f[0], p.rne);
  }
}

template <int DT, int C, bool NHWC, bool AA>
void launch_vec(const ResizeParams& p, int n_imgs, bool vec, hipStream_t s) {
  if constexpr (AA) {
    const int tiles = (p.W + kAaTile - 1) / kAaTile, bands = (p.H + kAaBand - 1) / kAaBand;
    const dim3 grid((unsigned)(tiles * bands), (unsigned)n_imgs);
    if (vec) hipLaunchKernelGGL((resize_pack_aa<DT, C, NHWC, true>), grid, dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((resize_pack_aa<DT, C, NHWC, false>), grid, dim3(kBlock), 0, s, p);
  } else {
    const int xq = (p.W + kPix - 1) / kPix;
    const dim3 grid((unsigned)(((int64_t)p.H * xq + kBlock - 1) / kBlock), (unsigned)n_imgs);
    if (vec) hipLaunchKernelGGL((resize_pack<DT, C, NHWC, true>), grid, dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((resize_pack<DT, C, NHWC, false>), grid, dim3(kBlock), 0, s, p);
  }
}

template <int DT, bool AA>
void launch_dt(const ResizeParams& p, int n_imgs, int C, int nhwc, bool vec, hipStream_t s) {
  if (C == 3) {
    if (nhwc) launch_vec<DT, 3, true, AA>(p, n_imgs, vec, s);
    else launch_vec<DT, 3, false, AA>(p, n_imgs, vec, s);
  } else {
    // one channel: both layouts are the same memory
    launch_vec<DT, 1, false, AA>(p, n_imgs, vec, s);
  }
}

// the argument checks and the 64-image chunking that K20 and K21 share
template <bool AA>
int resize_entry(const void* const* srcs, const int32_t* src_h, const int32_t* src_w, const int32_t* src_c,
                 int n_imgs, void* const* dsts, int dst_dtype, int dst_layout, int C, int H, int W,
                 const float* scale, const float* bias, int rounding, void* stream) {
  if (n_imgs < 0) return hipErrorInvalidValue;
  if (n_imgs == 0) return hipSuccess;
  if (!srcs || !src_h || !src_w || !src_c || !dsts) return hipErrorInvalidValue;
  if ((C != 1 && C != 3) || H < 1 || W < 1 || H > kMaxDim || W > kMaxDim) return hipErrorInvalidValue;
  if (dst_layout != 0 && dst_layout != 1) return hipErrorInvalidValue;
  if (dst_dtype != kFP32 && dst_dtype != kFP16 && dst_dtype != kBF16) return hipErrorInvalidValue;
  const int esz = dtype_size(dst_dtype);
  bool vec = W % kPix == 0;
  for (int i = 0; i < n_imgs; ++i) {
    if (!srcs[i] || !dsts[i] || ((uintptr_t)dsts[i]) % esz) return hipErrorInvalidValue;
    if (src_h[i] < 1 || src_w[i] < 1 || src_h[i] > kMaxDim || src_w[i] > kMaxDim) return hipErrorInvalidValue;
    if (src_c[i] != 1 && src_c[i] != 3) return hipErrorInvalidValue;
    vec = vec && ((uintptr_t)dsts[i]) % 16 == 0;
  }
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n_imgs; base += kMaxImgs) {
    ResizeParams p;
    const int cnt = n_imgs - base < kMaxImgs ? n_imgs - base : kMaxImgs;
    for (int i = 0; i < kMaxImgs; ++i) {
      const int j = base + (i < cnt ? i : 0);
      p.src[i] = static_cast<const uint8_t*>(srcs[j]);
      p.dst[i] = dsts[j];
      p.h[i] = src_h[j];
      p.w[i] = src_w[j];
      p.c[i] = (uint8_t)src_c[j];
    }
    for (int c = 0; c < 3; ++c) {
      p.scale[c] = scale && c < C ? scale[c] : 1.0f;
      p.bias[c] = bias && c < C ? bias[c] : 0.0f;
    }
    p.H = H;
    p.W = W;
    p.rne = rounding;
    switch (dst_dtype) {
      case kFP32: launch_dt<kFP32, AA>(p, cnt, C, dst_layout, vec, s); break;
      case kFP16: launch_dt<kFP16, AA>(p, cnt, C, dst_layout, vec, s); break;
      default: launch_dt<kBF16, AA>(p, cnt, C, dst_layout, vec, s); break;
    }
    const int rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

}  // namespace

// srcs / src_h / src_w / src_c / dsts: host arrays of n_imgs entries.  srcs[i]
// is a device pointer (any alignment) to a uint8 HWC image of
// src_h[i] x src_w[i] x src_c[i], src_c 1 or 3; dsts[i] is a device pointer
// (aligned to the element size) to its own C*H*W outputs of dst_dtype (FP32 /
// FP16 / BF16) in dst_layout (0 = NCHW, 1 = NHWC), C 1 or 3.  scale / bias:
// host arrays of C floats or NULL.  A dimension above 16384, a channel count
// outside {1, 3} or a null table is hipErrorInvalidValue before any launch.
extern "C" int tcamd_resize_pack(const void* const* srcs, const int32_t* src_h, const int32_t* src_w,
                                 const int32_t* src_c, int n_imgs, void* const* dsts, int dst_dtype, int dst_layout,
                                 int C, int H, int W, const float* scale, const float* bias, int rounding,
                                 void* stream) {
  return resize_entry<false>(srcs, src_h, src_w, src_c, n_imgs, dsts, dst_dtype, dst_layout, C, H, W, scale, bias,
                             rounding, stream);
}

// K21: the same arguments and checks as tcamd_resize_pack, antialiased.
extern "C" int tcamd_resize_pack_aa(const void* const* srcs, const int32_t* src_h, const int32_t* src_w,
                                    const int32_t* src_c, int n_imgs, void* const* dsts, int dst_dtype,
                                    int dst_layout, int C, int H, int W, const float* scale, const float* bias,
                                    int rounding, void* stream) {
  return resize_entry<true>(srcs, src_h, src_w, src_c, n_imgs, dsts, dst_dtype, dst_layout, C, H, W, scale, bias,
                            rounding, stream);
}
