// K10c — batch-invariant fp32-parity classifier of the DenseNet-121 head
// (gfx950).
//
//   logits[b, N] = pooled[b, K] . W[N, K]^T + bias[N]
//
// as the split-precision product of the rest of the fp32 engine
// (csrc/kernels/densenet_x3.hip): a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on
// v_mfma_f32_16x16x32_bf16, fp32 accumulate, fp32 out.  The operand arrives
// already split (the x3_head_pool_split variant of K10x writes the pooled row as
// bf16 hi / lo planes [b][K]); W is split once at engine build into hi / lo
// planes [16 ceil(N / 16)][K] with zero rows past N (ops.hip
// x3_classifier_weights).
//
// The shape is [b <= 128, 1024] x [1024, 1000]: small, weight bound, N no
// multiple of a GEMM tile.  What the kernel is for is that the logits of a
// row are a function of that row alone -- the same bits at b = 1 and b = 128,
// at any position of the batch -- so a served row can be compared exactly
// whatever batch the server formed around it:
//   * weight-stationary column tiles: a workgroup owns 16 columns over the
//     whole of K and 32 rows; grid = ceil(N / 16) x ceil(b / 32), 63 x 4 at
//     the model's shape and b = 128 (one round of the 256 CUs);
//   * K split over the 4 waves in a fixed pattern: wave w takes the 64-deep
//     slices 4 t + w (t = 0, 1, ...), two 32-deep MFMA steps each, and
//     accumulates them in ascending t.  The pattern depends on K alone;
//   * the 4 partials are summed through LDS as ((w0 + w1) + w2) + w3, then
//     the bias: no atomics, no second workgroup touches an output;
//   * a row's accumulator is one MFMA output row: the matrix pipe computes
//     it from that row of the operand only, whatever the other 15 rows hold
//     and wherever the row sits in the tile.  Rows past b are staged as
//     zeros and never stored; columns past N meet zero weights and are never
//     stored either (out is the [b, ldc] buffer the server scatters from);
//   * staging, per wave and per slice, into the wave's own 16 KB of LDS (no
//     workgroup barrier inside the K loop): W by LDS-DMA
//     (global_load_lds_dwordx4) into a 2-slice ring, the next slice in
//     flight under the current one's MFMAs; the operand by 16-byte loads
//     held in registers one slice ahead (that is where rows past b become
//     zeros) and written to LDS when their slice comes up.  Rows are 128 B,
//     their 16-B chunks XOR-swizzled by (row >> 1) & 7 as in K18
//     (csrc/kernels/gemm_tiles.hip): every ds_read_b128 group of a fragment
//     read covers 16 distinct bank slots.
//
// This file is compiled without the packed fp32 VALU forms (see the
// Makefile): the epilogue's f32x4 sums are scalar v_add_f32.
//
// Reference analog: none (the reference client runs no model).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr int kBM = 32;                    // rows of a workgroup's tile
constexpr int kTN = 16;                    // its columns
constexpr int kWaves = 4;                  // K slices in flight side by side
constexpr int kKW = 64;                    // k of one slice
constexpr int kRow = kKW * 2;              // bytes of one staged row
constexpr int kWPlane = kTN * kRow;        // one W plane of a slice (2 KB)
constexpr int kWBuf = 2 * kWPlane;         // hi | lo
constexpr int kAPlane = kBM * kRow;        // one operand plane of a slice (4 KB)
constexpr int kWaveLds = 2 * kWBuf + 2 * kAPlane;  // W ring of 2 | A hi | A lo = 16 KB
constexpr int kWDma = 4;                   // LDS-DMAs of one W slice (1 KB each)
constexpr int kALoads = 8;                 // 16-byte loads of one operand slice per lane

struct X3ClassifierParams {
  const uint16_t* a_hi;  // [b][K] bf16
  const uint16_t* a_lo;
  const uint16_t* w_hi;  // [16 ceil(N / 16)][K] bf16, zero rows past N
  const uint16_t* w_lo;
  const float* bias;     // [N]
  float* out;            // [b][ldc]
  int b, N, K, ldc;
};

__device__ __forceinline__ v4u ld16(const void* p) { return *reinterpret_cast<const v4u*>(p); }
__device__ __forceinline__ bf16x8 fr(v4u v) { return __builtin_bit_cast(bf16x8, v); }

// 16-B chunk c of staged row r sits at chunk c ^ swz(r)
__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

// bf16x3 product, the two small cross terms first (as x3_16 of densenet_x3.hip)
__device__ __forceinline__ f32x4 x3_mma(v4u ah, v4u al, v4u bh, v4u bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr(al), fr(bh), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr(ah), fr(bl), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr(ah), fr(bh), c, 0, 0, 0);
}

__global__ void __launch_bounds__(64 * kWaves) x3_classifier_kernel(X3ClassifierParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaves * kWaveLds];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * kTN, m0 = blockIdx.y * kBM;
  uint8_t* wl = lds + wave * kWaveLds;  // this wave's W ring
  uint8_t* al = wl + 2 * kWBuf;         // ... and its operand slice, hi | lo
  const int r8 = lane >> 3, c8 = lane & 7;

  // W by LDS-DMA: instruction i fills rows 8 (i % 2) .. + 7 of plane i / 2
  // lane-linear (row r8, chunk' c8) from global chunk c8 ^ swz(row).  Every
  // row exists: the planes are padded to a multiple of 16 rows.
  const uint16_t* wsrc[kWDma];
#pragma unroll
  for (int i = 0; i < kWDma; ++i) {
    const int row = 8 * (i & 1) + r8;
    wsrc[i] = (i >> 1 ? p.w_lo : p.w_hi) + (size_t)(n0 + row) * p.K + kKW * wave + 8 * (c8 ^ swz(row));
  }
  // operand by 16-byte loads: load i covers rows 8 (i % 4) .. + 7 of plane
  // i / 4, a row's chunks on 8 consecutive lanes.  A row past b reads the
  // last real row (never memory past the operand) and is replaced by zeros
  // on its way to LDS.
  const uint16_t* asrc[kALoads];
  int adst[kALoads / 2];
  bool aok[kALoads / 2];
#pragma unroll
  for (int i = 0; i < kALoads / 2; ++i) {
    const int row = 8 * i + r8;
    aok[i] = m0 + row < p.b;
    const size_t at = (size_t)min(m0 + row, p.b - 1) * p.K + kKW * wave + 8 * c8;
    asrc[i] = p.a_hi + at;
    asrc[kALoads / 2 + i] = p.a_lo + at;
    adst[i] = row * kRow + ((c8 ^ swz(row)) << 4);
  }
  // fragment reads: lane (row lane % 16 of a 16-row block, k chunk 4 ks + lane / 16)
  int lofs[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) lofs[ks] = (lane & 15) * kRow + (((4 * ks + (lane >> 4)) ^ swz(lane & 15)) << 4);

  // this wave's slices: 4 t + wave < K / 64
  const int nt = (p.K / kKW - wave + kWaves - 1) / kWaves;
  constexpr int kStep = kWaves * kKW;  // elements between a wave's slices
  auto dma_w = [&](int t) {
    uint8_t* dst = wl + (t & 1) * kWBuf;
#pragma unroll
    for (int i = 0; i < kWDma; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(wsrc[i] + t * kStep), (void*)(dst + i * 1024), 16, 0, 0);
  };
  v4u ar[kALoads];
  auto load_a = [&](int t) {
#pragma unroll
    for (int i = 0; i < kALoads; ++i) ar[i] = ld16(asrc[i] + t * kStep);
  };

  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (nt > 0) {
    dma_w(0);
    load_a(0);
  }
  for (int t = 0; t < nt; ++t) {
    // slice t has landed: its W DMAs in LDS, its operand in registers
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const v4u zero = v4u{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kALoads / 2; ++i) {
      *reinterpret_cast<v4u*>(al + adst[i]) = aok[i] ? ar[i] : zero;
      *reinterpret_cast<v4u*>(al + kAPlane + adst[i]) = aok[i] ? ar[kALoads / 2 + i] : zero;
    }
    // slice t + 1 flies under slice t's LDS traffic and MFMAs; its ring slot
    // was read in slice t - 1, whose fragments are in registers
    if (t + 1 < nt) {  // wave-uniform
      dma_w(t + 1);
      load_a(t + 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the operand writes
    const uint8_t* wb = wl + (t & 1) * kWBuf;
    v4u ah[2][2], alo[2][2], wh[2], wlo[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      wh[ks] = ld16(wb + lofs[ks]);
      wlo[ks] = ld16(wb + kWPlane + lofs[ks]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        ah[ks][j] = ld16(al + j * 16 * kRow + lofs[ks]);
        alo[ks][j] = ld16(al + kAPlane + j * 16 * kRow + lofs[ks]);
      }
    }
    // operand A = the pooled rows, B = W: D row 4 (lane / 16) + e is a batch
    // row, D column lane % 16 an output column
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = x3_mma(ah[ks][j], alo[ks][j], wh[ks], wlo[ks], acc[j]);
    // the fragments are in registers before the next slice's operand writes
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // partials through each wave's own LDS (nobody else read it), one fixed order
  f32x4* part = reinterpret_cast<f32x4*>(wl);
  part[lane] = acc[0];
  part[64 + lane] = acc[1];
  __syncthreads();
  if (tid >= 128) return;
  const int j = tid >> 6;  // 16-row block: waves 0 and 1 finish one each
  f32x4 v = *reinterpret_cast<const f32x4*>(lds + (j * 64 + lane) * 16);
#pragma unroll
  for (int w = 1; w < kWaves; ++w) v = v + *reinterpret_cast<const f32x4*>(lds + w * kWaveLds + (j * 64 + lane) * 16);
  const int n = n0 + (lane & 15), row0 = m0 + 16 * j + 4 * (lane >> 4);
  if (n >= p.N) return;
  const float bn = p.bias[n];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (row0 + e < p.b) p.out[(size_t)(row0 + e) * p.ldc + n] = v[e] + bn;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" {

// logits[b][ldc] (fp32, columns 0 .. N - 1 written) = a[b][K] . w[N][K]^T + bias;
// a_hi / a_lo bf16 [b][K], w_hi / w_lo bf16 [16 ceil(N / 16)][K] (zero rows
// past N).  1 <= b <= 128, K a multiple of 64, ldc >= N.
int tcamd_x3_classifier(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                        float* out, int b, int N, int K, int ldc, void* stream) {
  if (b <= 0) return hipSuccess;
  if (b > 128 || N < 1 || K < kKW || K % kKW || ldc < N) return hipErrorInvalidValue;
  if (!a_hi || !a_lo || !w_hi || !w_lo || !bias || !out) return hipErrorInvalidValue;
  if (!aligned16(a_hi) || !aligned16(a_lo) || !aligned16(w_hi) || !aligned16(w_lo) || (uintptr_t)bias % 4 ||
      (uintptr_t)out % 4)
    return hipErrorInvalidValue;
  X3ClassifierParams p;
  p.a_hi = (const uint16_t*)a_hi;
  p.a_lo = (const uint16_t*)a_lo;
  p.w_hi = (const uint16_t*)w_hi;
  p.w_lo = (const uint16_t*)w_lo;
  p.bias = bias;
  p.out = out;
  p.b = b;
  p.N = N;
  p.K = K;
  p.ldc = ldc;
  hipLaunchKernelGGL(x3_classifier_kernel, dim3((N + kTN - 1) / kTN, (b + kBM - 1) / kBM), dim3(64 * kWaves), 0,
                     (hipStream_t)stream, p);
  return hipGetLastError();
}

}  // extern "C"
