// K19 topk_rows — per-row top-K selection of fp32 scores, the device half of
// the KServe `classification` extension (tcserve answers
// InferRequestedOutput("fc6_1", class_count=k) from the pairs this writes;
// csrc/cpp/server/classify.h is the host twin with the same ordering).
//
// Ordering contract (np.argsort(-row, kind="stable")[:k] on the fp32 row):
// scores descend, equal scores go to the lower index first, -0.0 == +0.0,
// +/-inf order as values, every NaN ranks below every number and NaNs keep
// index order.  Each element becomes a unique 64-bit key
//   monotone_u32(score) << 32 | (0xFFFFFFFF - index)
// (-0.0 folded into +0.0, NaN mapped to 0), so "largest key" is the whole
// contract and round j selects the largest key strictly below round j-1's:
// lanes keep no exclusion state.
//
// One wave64 per row, four rows per 256-thread workgroup.  A row of up to
// 1024 / 4096 elements is loaded once into registers (coalesced float4 when
// the base and the stride are 16-byte aligned, dwords otherwise); longer rows
// are re-read from L2 every round.  Each round: per-lane max over the held
// values below the bound, a 64-bit butterfly max over the wave, and the lane
// that owns the winner stores {score bits, index} with one 8-byte store.

#include "kernels/common.h"

using namespace tcamd;

#define TCAMD_TOPK_KMAX 64

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = kBlock / kWave;

__device__ __forceinline__ uint64_t topk_key(uint32_t bits, uint32_t idx) {
  uint32_t m;
  if ((bits & 0x7fffffffu) > 0x7f800000u) {
    m = 0u;  // NaN: below -inf (whose image is 0x007fffff)
  } else {
    if (bits == 0x80000000u) bits = 0u;  // -0.0 ties with +0.0
    m = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return ((uint64_t)m << 32) | (uint64_t)(0xFFFFFFFFu - idx);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, kWave);
    uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, kWave);
    uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

struct Pair {
  uint32_t score_bits;
  int32_t index;
};

// VPL: values per lane held in registers (0 = streaming, the row is re-read
// from memory every round).
template <int VPL>
__global__ void __launch_bounds__(kBlock)
topk_rows(const uint8_t* __restrict__ x, uint64_t row_stride, int rows, int C, const int32_t* __restrict__ k_row,
          int kmax, Pair* __restrict__ pairs) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  int k = k_row[r];
  if (k > C) k = C;
  if (k > kmax) k = kmax;
  if (k <= 0) return;
  const uint8_t* rowp = x + (uint64_t)r * row_stride;
  const uint32_t* row = reinterpret_cast<const uint32_t*>(rowp);
  Pair* out = pairs + (uint64_t)r * (uint64_t)kmax;
  const uint32_t uC = (uint32_t)C;

  if constexpr (VPL > 0) {
    // element e of this lane sits at index: float4 path 4*((e/4)*64+lane)+e%4, dword path e*64+lane
    const bool vec = ((((uintptr_t)x) | row_stride) & 15) == 0;
    uint32_t raw[VPL];
    if (vec) {
#pragma unroll
      for (int j = 0; j < VPL / 4; ++j) {
        const uint32_t base = 4u * (uint32_t)(j * kWave + lane);
        if (base + 3 < uC) {
          const uint4 v = *reinterpret_cast<const uint4*>(row + base);
          raw[4 * j + 0] = v.x;
          raw[4 * j + 1] = v.y;
          raw[4 * j + 2] = v.z;
          raw[4 * j + 3] = v.w;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) raw[4 * j + c] = base + c < uC ? row[base + c] : 0u;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < VPL; ++e) {
        const uint32_t idx = (uint32_t)(e * kWave + lane);
        raw[e] = idx < uC ? row[idx] : 0u;
      }
    }
    uint64_t bound = ~0ull;
    for (int j = 0; j < k; ++j) {
      uint64_t best = 0;
      uint32_t best_raw = 0;
#pragma unroll
      for (int e = 0; e < VPL; ++e) {
        const uint32_t idx = vec ? 4u * (uint32_t)((e >> 2) * kWave + lane) + (uint32_t)(e & 3)
                                 : (uint32_t)(e * kWave + lane);
        const uint64_t key = topk_key(raw[e], idx);
        if (idx < uC && key < bound && key > best) {
          best = key;
          best_raw = raw[e];
        }
      }
      const uint64_t win = wave_max_u64(best);
      if (win == 0) break;  // unreachable for k <= C; never spin on an empty round
      if (best == win) {
        Pair p;
        p.score_bits = best_raw;
        p.index = (int32_t)(0xFFFFFFFFu - (uint32_t)win);
        out[j] = p;
      }
      bound = win;
    }
  } else {
    uint64_t bound = ~0ull;
    for (int j = 0; j < k; ++j) {
      uint64_t best = 0;
      uint32_t best_raw = 0;
      for (uint32_t idx = (uint32_t)lane; idx < uC; idx += kWave) {
        const uint32_t bits = row[idx];
        const uint64_t key = topk_key(bits, idx);
        if (key < bound && key > best) {
          best = key;
          best_raw = bits;
        }
      }
      const uint64_t win = wave_max_u64(best);
      if (win == 0) break;
      if (best == win) {
        Pair p;
        p.score_bits = best_raw;
        p.index = (int32_t)(0xFFFFFFFFu - (uint32_t)win);
        out[j] = p;
      }
      bound = win;
    }
  }
}

}  // namespace

// x: device fp32 rows, row r at x + r * row_stride_bytes (a multiple of 4);
// k_row: device [rows], 0 = skip the row; pairs: device [rows][kmax] of
// {float score; int32 index}.  Row r gets its min(k_row[r], C, kmax) best
// entries; nothing else is written.  kmax > TCAMD_TOPK_KMAX is
// hipErrorInvalidValue (callers take the host routine, classify.h).
extern "C" int tcamd_topk_rows(const float* x, uint64_t row_stride_bytes, int32_t rows, int32_t C,
                               const int32_t* k_row, int32_t kmax, void* pairs, hipStream_t s) {
  if (rows < 0 || C < 1 || kmax < 1 || kmax > TCAMD_TOPK_KMAX) return hipErrorInvalidValue;
  if (!x || !k_row || !pairs || (row_stride_bytes & 3) || (((uintptr_t)x) & 3)) return hipErrorInvalidValue;
  if (rows > 1 && row_stride_bytes < (uint64_t)C * 4) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)), block(kBlock);
  const uint8_t* xb = reinterpret_cast<const uint8_t*>(x);
  Pair* p = static_cast<Pair*>(pairs);
  if (C <= 1024)
    hipLaunchKernelGGL(topk_rows<16>, grid, block, 0, s, xb, row_stride_bytes, rows, C, k_row, kmax, p);
  else if (C <= 4096)
    hipLaunchKernelGGL(topk_rows<64>, grid, block, 0, s, xb, row_stride_bytes, rows, C, k_row, kmax, p);
  else
    hipLaunchKernelGGL(topk_rows<0>, grid, block, 0, s, xb, row_stride_bytes, rows, C, k_row, kmax, p);
  return hipGetLastError();
}
