// K34 — embedding search over an int8 index, rescored exactly (gfx950).
//
// A variant beside K33 (csrc/kernels/embed_search.hip) for k <= 16: scan a
// compact index for a shortlist of 64 corpus rows per query, then give those 64
// K33's own bf16x3 score and select on that.  The final (index, score) pairs
// are K33's bits; what the int8 stage decides is only which 64 rows are looked
// at.  The caller holds both indexes (5 bytes an element): the gain is
// bandwidth, not memory.
//
// The int8 index (ops.hip.search_index_q8, search_quantize_q8 below, one wave
// a row): scales[n] = max|c[n]| / 127, codes[n][d] = clamp(rint(c[n][d] *
// (127 / max|c[n]|)), -127, 127), an all-zero row scale 0 and codes 0; codes
// int8 [64 ceil(N / 64)][D], scales fp32 [64 ceil(N / 64)], zero past N.  Pad
// rows are excluded by their index, never by their score.
//
// Three launches, no atomics; workspace = int32 [rows][64] shortlist, then u64
// [rows][slices][64] keys (tcamd_search_q8_workspace).
//
// 1. search_coarse_partial<NB>, grid = query groups (x) by corpus slices (y),
//    4 waves.  tcamd_search_q8_plan fixes both from (rows, N) alone: a group is
//    16 NB query rows, NB = 1 when rows <= 16, else 4; at most 256 / groups
//    slices of equal tile counts.
//    * The group's queries are quantised by the index rule on the way into LDS
//      (a wave a row: |max| by shuffles, then the multiply) and stay there as
//      int8: per 128-deep K slice NB blocks of 16 rows of 128 B, K33's chunk
//      swizzle.  The query's own scale is a positive constant of its ranking
//      and is dropped.
//    * Corpus tiles of 64 rows; wave w owns rows 16 w .. 16 w + 15 over the
//      whole of D and streams them by LDS-DMA (2 per K slice) through its own
//      3-slot ring of 2 KB slots, counted vmcnt, no barrier in the K loop, the
//      stream running on across tile ends -- K33's loop with a quarter of the
//      bytes.  A lane's 16-B fragment is one operand of
//      v_mfma_i32_16x16x64_i8: 2 MFMAs per slice and query block, NB i32
//      accumulators.  127 * 127 * 1024 < 2^24: the dot products are exact.
//    * coarse = (float)dot * scales[n]: an exact conversion and one fp32
//      multiply.  The wave fetches its 16 scales at the top of a tile with a
//      global_load_dword written in assembly, so that the compiler puts no
//      vmcnt(0) of its own into the stream for it; loads retire in order, so
//      the K loop's counted waits cover it from the second K step on, and a
//      one-step tile (D = 128) waits vmcnt(2) after its step.
//    * The scores go through an LDS tile [16 NB][64] (two, in turn, one
//      barrier a tile as in K33).  Wave w then owns queries 4 NB w .. + 4 NB
//      - 1 and keeps each one's best 64 keys sorted over its lanes (K33's
//      compare, ballot and insert; 32 VGPRs of keys at NB = 4).  The depth is
//      64 whatever k.
//    * Barriers: the tile loop's bounds come from blockIdx and the launch
//      parameters; the per-query branches enclose none.
//    LDS at D = 1024, NB = 4: 64 KB queries + 24 KB rings + 2 x 16 KB score
//    tiles = 120 KB.
// 2. search_shortlist, one wave a query row: K33's merge over the slices'
//    sorted lists, 64 rounds, the indices (-1 past min(N, 64)) to the
//    workspace.
// 3. search_rescore, one workgroup a query row, 4 waves.  Wave w gathers
//    shortlist entries 16 w .. + 15 from K33's hi / lo planes straight into
//    MFMA operands (lane = candidate lane % 16, d chunk lane / 16) and runs
//    K33's sequence: per 32-deep step lo*hi, hi*lo, hi*hi, d ascending, the
//    query split by split8 in operand row 0, one accumulator element per
//    candidate: the pair's K33 bits.  The 64 keys meet in LDS; wave 0 ranks
//    them (a key's rank = the keys above it) and writes the best min(k_row,
//    kmax), ranks at and past min(N, 64) as (-1, -FLT_MAX).
//
// Deviations from the plan of the issue: the scale fetch in assembly (above),
// and the final selection by rank instead of a sorted insert -- 64 keys, one
// pass, no loop-carried shuffles.
//
// Reference analog: none (the reference client runs no model).

#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <cstdint>

#include "kernels/embed_search_common.h"

#define TCAMD_SEARCH_Q8_KMAX 16

extern "C" int tcamd_search_q8_plan(int rows, int N, int* slices, int* group);

namespace {

using namespace tcamd_search;

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;                   // corpus rows of a tile
constexpr int kWaves = 4;                   // 16 corpus rows each
constexpr int kKW = 128;                    // k of one slice = bytes of one staged row
constexpr int kBlk = 16 * kKW;              // 16 rows of one K slice (2 KB): a ring slot, a query block
constexpr int kRing = 3;
constexpr int kAhead = kRing - 1;           // K slices in flight
constexpr int kDma = 2;                     // LDS-DMAs of one K slice (1 KB each)
constexpr int kShort = 64;                  // shortlist depth
constexpr int kMaxSlices = 256;             // 4 heads per lane in the merge
constexpr int kMaxRows = 128;
constexpr int kMaxDevices = 64;

constexpr size_t lds_bytes(int D, int NB) {
  return (size_t)(D / kKW) * NB * kBlk + kWaves * kRing * kBlk + 2 * (size_t)(16 * NB) * kTile * 4;
}

struct CoarseParams {
  const uint8_t* q;       // fp32 rows, q_stride bytes apart
  uint64_t q_stride;
  const int8_t* codes;    // [64 ceil(N / 64)][D]
  const float* scales;    // [64 ceil(N / 64)]
  const int32_t* k_row;   // [rows]
  uint64_t* keys;         // [rows][slices][64]
  int rows, N, D, slices, tps;
};

// A wave quantises one row: lane l holds x[16] = elements 16 l .. 16 l + 15
// (zeros past the row's end).  Returns the 16 codes and the row's max |x|.
__device__ __forceinline__ v4u quant16(const float* x, float& amax) {
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) m = fmaxf(m, fabsf(x[e]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  amax = m;
  const float inv = m > 0.f ? 127.0f / m : 0.f;
  v4u out;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t pack = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float r = fminf(fmaxf(__builtin_rintf(x[4 * w + b] * inv), -127.f), 127.f);
      pack |= ((uint32_t)(int)r & 0xffu) << (8 * b);
    }
    out[w] = pack;
  }
  return out;
}

__device__ __forceinline__ void load16(const float* src, float* x) {
#pragma unroll
  for (int e = 0; e < 4; ++e) *reinterpret_cast<f32x4*>(x + 4 * e) = *reinterpret_cast<const f32x4*>(src + 4 * e);
}

__global__ void __launch_bounds__(64 * kWaves)
search_quantize_q8_kernel(const float* __restrict__ src, int rows, int D, int8_t* __restrict__ codes,
                          float* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= rows) return;  // a whole wave
  float x[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = 0.f;
  const bool in = 16 * lane < D;
  if (in) load16(src + (size_t)r * D + 16 * lane, x);
  float amax;
  const v4u c = quant16(x, amax);
  if (in) *reinterpret_cast<v4u*>(codes + (size_t)r * D + 16 * lane) = c;
  if (lane == 0) scales[r] = amax / 127.0f;
}

template <int NB>
__global__ void __launch_bounds__(64 * kWaves) search_coarse_partial_kernel(CoarseParams p) {
  constexpr int G = 16 * NB;    // query rows of the workgroup
  constexpr int QPW = 4 * NB;   // queries a wave selects for
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.x * G, slice = blockIdx.y;
  const int nks = p.D / kKW;
  uint8_t* ql = lds;                                                   // queries: [nks][NB][16][128 B]
  uint8_t* ring = lds + (size_t)nks * NB * kBlk + wave * kRing * kBlk;  // this wave's ring
  float* sc = reinterpret_cast<float*>(lds + (size_t)nks * NB * kBlk + kWaves * kRing * kBlk);

  const int tiles = (p.N + kTile - 1) / kTile;
  const int t0 = slice * p.tps;
  const int nt = min(p.tps, tiles - t0);  // >= 1 by the plan
  const int total = nt * nks;             // K slices of this wave's stream

  // corpus by LDS-DMA: instruction i fills rows 8 i .. 8 i + 7 lane-linear
  // (row r8, chunk' c8) from global chunk c8 ^ swz(row).  Every row exists:
  // the codes are padded to a multiple of 64 rows.
  const int r8 = lane >> 3, c8 = lane & 7;
  const int8_t* csrc[kDma];
#pragma unroll
  for (int i = 0; i < kDma; ++i) {
    const int row = 8 * i + r8;
    csrc[i] = p.codes + ((size_t)t0 * kTile + 16 * wave + row) * p.D + 16 * (c8 ^ swz(row));
  }
  size_t iadd = 0;  // bytes from csrc to the next K slice to issue
  int issued = 0, ik = 0, islot = 0;
  auto issue = [&]() {
    uint8_t* dst = ring + islot * kBlk;
#pragma unroll
    for (int i = 0; i < kDma; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(csrc[i] + iadd), (void*)(dst + i * 1024), 16, 0, 0);
    ++issued;
    islot = islot + 1 == kRing ? 0 : islot + 1;
    iadd += kKW;
    if (++ik == nks) {  // on to the next tile: 64 rows further, k back to 0
      ik = 0;
      iadd += (size_t)(kTile - 1) * p.D;
    }
  };
#pragma unroll
  for (int s = 0; s < kAhead; ++s)
    if (issued < total) issue();  // wave-uniform

  // the queries, once, a wave a row: fp32 -> int8 by the index rule
  const int cpr = p.D / 16;  // 16-B chunks of a row
  for (int row = wave; row < G; row += kWaves) {
    float x[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = 0.f;
    if (lane < cpr && q0 + row < p.rows)
      load16(reinterpret_cast<const float*>(p.q + (size_t)(q0 + row) * p.q_stride) + 16 * lane, x);
    float amax;
    const v4u c = quant16(x, amax);
    if (lane < cpr)
      *reinterpret_cast<v4u*>(ql + (size_t)((lane >> 3) * NB + (row >> 4)) * kBlk + (row & 15) * kKW +
                              (((lane & 7) ^ swz(row & 15)) << 4)) = c;
  }

  // this wave's queries of the selection: rows q0 + QPW wave + i
  // (lane i < QPW reads row i's k_row: one load, then a ballot)
  const int myrow = q0 + QPW * wave + lane;
  const bool mine = lane < QPW && myrow < p.rows && p.k_row[myrow] > 0;
  const uint32_t live = (uint32_t)__ballot(mine);
  uint64_t kept[QPW];
#pragma unroll
  for (int i = 0; i < QPW; ++i) kept[i] = 0;

  // fragment reads: lane (row lane % 16 of a 16-row block, k chunk 4 s + lane / 16)
  int lofs[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) lofs[s] = (lane & 15) * kKW + (((4 * s + (lane >> 4)) ^ swz(lane & 15)) << 4);

  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the query writes
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  int rslot = 0;
  for (int t = 0; t < nt; ++t) {
    // this wave's 16 scales of the tile; see the header for the wait
    float sv;
    const float* sp = p.scales + (size_t)(t0 + t) * kTile + 16 * wave + (lane & 15);
    asm volatile("global_load_dword %0, %1, off" : "=&v"(sv) : "v"(sp) : "memory");

    v4i acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = v4i{0, 0, 0, 0};
    for (int ks = 0; ks < nks; ++ks) {
      // the slot read in the last step takes the K slice kAhead steps on; then
      // this step's slice has landed once at most kAhead slices are in flight
      if (issued < total) {  // wave-uniform
        issue();
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kAhead * kDma) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      const uint8_t* cb = ring + rslot * kBlk;
      const uint8_t* qb = ql + (size_t)ks * NB * kBlk;
      rslot = rslot + 1 == kRing ? 0 : rslot + 1;
      v4u cf[2], qf[NB][2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        cf[s] = ld16(cb + lofs[s]);
#pragma unroll
        for (int b = 0; b < NB; ++b) qf[b][s] = ld16(qb + b * kBlk + lofs[s]);
      }
      // the fragments are in registers before the next step's DMA takes the slot
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // operand A = the queries, B = the corpus rows: D row 4 (lane / 16) + e
      // is a query of block b, D column lane % 16 a corpus row of this wave
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(v4i, qf[b][s]),
                                                         __builtin_bit_cast(v4i, cf[s]), acc[b], 0, 0, 0);
    }
    if (nks == 1) {  // one step: at most one DMA older than the scale load is in flight, and 2 younger
      asm volatile("s_waitcnt vmcnt(%1)" : "+v"(sv) : "n"(kDma) : "memory");
    } else {
      asm volatile("" : "+v"(sv)::"memory");
    }

    float* st = sc + (t & 1) * (G * kTile);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        st[(16 * b + 4 * (lane >> 4) + e) * kTile + 16 * wave + (lane & 15)] = (float)acc[b][e] * sv;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the DMAs in flight go to the wave's own ring: no vmcnt wait here
    asm volatile("" ::: "memory");

    const uint32_t idx = (uint32_t)(t0 + t) * kTile + lane;
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
      if (!(live >> i & 1)) continue;  // wave-uniform
      const float s = st[(QPW * wave + i) * kTile + lane];
      const uint64_t key = idx < (uint32_t)p.N ? topk_key(__float_as_uint(s), idx) : 0;
      uint64_t thr = lane_u64(kept[i], kShort - 1);
      uint64_t m = __ballot(key > thr);
      while (m) {
        const int b = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint64_t cand = lane_u64(key, b);
        if (cand > thr) {
          kept[i] = insert_key(kept[i], cand, lane);
          thr = lane_u64(kept[i], kShort - 1);
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < QPW; ++i) {
    if (!(live >> i & 1)) continue;
    const size_t r = q0 + QPW * wave + i;
    p.keys[(r * p.slices + slice) * kShort + lane] = kept[i];
  }
}

// K33's merge (search_merge_kernel) at depth 64, the indices alone, to the workspace
__global__ void __launch_bounds__(64 * kWaves)
search_shortlist_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ k_row, int rows, int slices,
                        int32_t* __restrict__ shortlist) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= rows) return;
  if (k_row[r] <= 0) return;
  const uint64_t* row = keys + (size_t)r * slices * kShort;
  uint64_t head[kMaxSlices / 64];
  int at[kMaxSlices / 64];
#pragma unroll
  for (int i = 0; i < kMaxSlices / 64; ++i) {
    const int s = lane + 64 * i;
    at[i] = 0;
    head[i] = s < slices ? row[(size_t)s * kShort] : 0;
  }
  int j = 0;
  for (; j < kShort; ++j) {
    uint64_t best = 0;
#pragma unroll
    for (int i = 0; i < kMaxSlices / 64; ++i) best = head[i] > best ? head[i] : best;
    const uint64_t win = wave_max_u64(best);
    if (win == 0) break;  // the corpus has fewer than 64 rows
#pragma unroll
    for (int i = 0; i < kMaxSlices / 64; ++i) {
      if (head[i] != win) continue;  // keys are unique: one head of one lane
      shortlist[(size_t)r * kShort + j] = (int32_t)(0xFFFFFFFFu - (uint32_t)win);
      ++at[i];
      head[i] = at[i] < kShort ? row[(size_t)(lane + 64 * i) * kShort + at[i]] : 0;
    }
  }
  for (j += lane; j < kShort; j += 64) shortlist[(size_t)r * kShort + j] = -1;
}

struct RescoreParams {
  const uint8_t* q;
  uint64_t q_stride;
  const uint16_t* c_hi;   // K33's planes
  const uint16_t* c_lo;
  const int32_t* k_row;
  const int32_t* shortlist;  // [rows][64]
  int32_t* indices;          // [rows][slots]
  float* scores;
  int D, kmax, slots;
};

constexpr int kStep = 8;  // 32-deep steps whose candidate fragments are fetched together

__global__ void __launch_bounds__(64 * kWaves) search_rescore_kernel(RescoreParams p) {
  __shared__ uint64_t keys[kShort];
  __shared__ __attribute__((aligned(16))) uint16_t qs[2][1024];  // the query, hi | lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;
  const int k = min(p.k_row[r], p.kmax);
  if (k <= 0) return;  // the whole workgroup
  if (8 * tid < p.D) {
    const float* src = reinterpret_cast<const float*>(p.q + (size_t)r * p.q_stride) + 8 * tid;
    float f[8];
    *reinterpret_cast<f32x4*>(f) = *reinterpret_cast<const f32x4*>(src);
    *reinterpret_cast<f32x4*>(f + 4) = *reinterpret_cast<const f32x4*>(src + 4);
    v4u hi, lo;
    split8(f, hi, lo);
    *reinterpret_cast<v4u*>(&qs[0][8 * tid]) = hi;
    *reinterpret_cast<v4u*>(&qs[1][8 * tid]) = lo;
  }
  const int col = lane & 15, g = lane >> 4;
  const int cand = p.shortlist[(size_t)r * kShort + 16 * wave + col];
  const bool valid = cand >= 0;
  const size_t base = (size_t)(valid ? cand : 0) * p.D + 8 * g;
  const uint16_t* ch = p.c_hi + base;
  const uint16_t* cl = p.c_lo + base;
  __syncthreads();
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  // D / 32 steps, a multiple of 4; kStep at a time so that 2 kStep loads are in flight
  for (int m0 = 0; m0 < p.D / 32; m0 += kStep) {
    v4u bh[kStep], bl[kStep];
#pragma unroll
    for (int i = 0; i < kStep; ++i) {
      bh[i] = bl[i] = v4u{0u, 0u, 0u, 0u};
      if (valid && m0 + i < p.D / 32) {  // entries past the valid count are not gathered
        bh[i] = ld16(ch + 32 * (m0 + i));
        bl[i] = ld16(cl + 32 * (m0 + i));
      }
    }
#pragma unroll
    for (int i = 0; i < kStep; ++i) {
      if (m0 + i >= p.D / 32) break;  // workgroup-uniform
      v4u ah = v4u{0u, 0u, 0u, 0u}, al = ah;
      if (col == 0) {  // the query is row 0 of operand A
        ah = ld16(&qs[0][32 * (m0 + i) + 8 * g]);
        al = ld16(&qs[1][32 * (m0 + i) + 8 * g]);
      }
      acc = x3_mma(ah, al, bh[i], bl[i], acc);
    }
  }
  // D row 0, column lane % 16: element 0 of lanes 0 .. 15
  if (g == 0) keys[16 * wave + col] = valid ? topk_key(__float_as_uint(acc[0]), (uint32_t)cand) : 0;
  __syncthreads();
  if (wave != 0) return;
  const uint64_t mine = keys[lane];
  int rank = 0;
#pragma unroll 8
  for (int j = 0; j < kShort; ++j) rank += keys[j] > mine;
  const int have = __popcll(__ballot(mine != 0));  // min(N, 64)
  if (mine != 0 && rank < k) {
    p.indices[(size_t)r * p.slots + rank] = (int32_t)(0xFFFFFFFFu - (uint32_t)mine);
    p.scores[(size_t)r * p.slots + rank] = key_score(mine);
  }
  if (lane >= have && lane < k) {
    p.indices[(size_t)r * p.slots + lane] = -1;
    p.scores[(size_t)r * p.slots + lane] = -FLT_MAX;
  }
}

int lds_opt_in(const void* kernel, std::atomic<bool>* done, int bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done[dev].store(true, std::memory_order_release);
  return e;
}

// tcamd_search_topk_q8; `ev`, if given: events recorded before the coarse launch, after it and after the rescore
int topk_q8(const float* q, uint64_t q_stride_bytes, int rows, const void* codes, const float* scales,
            const void* idx_hi, const void* idx_lo, int N, int D, const int32_t* k_row, int kmax, int slots,
            void* workspace, int32_t* indices, float* scores, void* stream, hipEvent_t* ev) {
  if (rows < 0 || rows > kMaxRows || N < 1 || D < kKW || D > 1024 || D % kKW || kmax < 1 ||
      kmax > TCAMD_SEARCH_Q8_KMAX || slots < kmax || slots > kShort)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (!q || !codes || !scales || !idx_hi || !idx_lo || !k_row || !workspace || !indices || !scores)
    return hipErrorInvalidValue;
  if (((uintptr_t)q | (uintptr_t)codes | (uintptr_t)idx_hi | (uintptr_t)idx_lo | q_stride_bytes) % 16 ||
      (uintptr_t)workspace % 8 || ((uintptr_t)scales | (uintptr_t)k_row | (uintptr_t)indices | (uintptr_t)scores) % 4)
    return hipErrorInvalidValue;
  if (rows > 1 && q_stride_bytes < (uint64_t)D * 4) return hipErrorInvalidValue;
  CoarseParams p;
  int group = 0;
  if (const int e = tcamd_search_q8_plan(rows, N, &p.slices, &group)) return e;
  // the dynamic-LDS opt-in is per device and per template
  static std::atomic<bool> attr1[kMaxDevices], attr4[kMaxDevices];
  if (const int e = group == 16 ? lds_opt_in((const void*)search_coarse_partial_kernel<1>, attr1, (int)lds_bytes(1024, 1))
                                : lds_opt_in((const void*)search_coarse_partial_kernel<4>, attr4, (int)lds_bytes(1024, 4)))
    return e;
  const int tiles = (int)(((int64_t)N + kTile - 1) / kTile);
  p.tps = (tiles + p.slices - 1) / p.slices;
  p.q = reinterpret_cast<const uint8_t*>(q);
  p.q_stride = q_stride_bytes;
  p.codes = (const int8_t*)codes;
  p.scales = scales;
  p.k_row = k_row;
  int32_t* shortlist = (int32_t*)workspace;
  p.keys = (uint64_t*)((uint8_t*)workspace + (size_t)rows * kShort * 4);
  p.rows = rows;
  p.N = N;
  p.D = D;
  const dim3 grid((rows + group - 1) / group, p.slices), block(64 * kWaves);
  const hipStream_t s = (hipStream_t)stream;
  if (ev) (void)hipEventRecord(ev[0], s);
  if (group == 16)
    hipLaunchKernelGGL(search_coarse_partial_kernel<1>, grid, block, lds_bytes(D, 1), s, p);
  else
    hipLaunchKernelGGL(search_coarse_partial_kernel<4>, grid, block, lds_bytes(D, 4), s, p);
  if (const hipError_t e = hipGetLastError()) return e;
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(search_shortlist_kernel, dim3((rows + kWaves - 1) / kWaves), block, 0, s,
                     (const uint64_t*)p.keys, k_row, rows, p.slices, shortlist);
  if (const hipError_t e = hipGetLastError()) return e;
  RescoreParams rp;
  rp.q = p.q;
  rp.q_stride = q_stride_bytes;
  rp.c_hi = (const uint16_t*)idx_hi;
  rp.c_lo = (const uint16_t*)idx_lo;
  rp.k_row = k_row;
  rp.shortlist = shortlist;
  rp.indices = indices;
  rp.scores = scores;
  rp.D = D;
  rp.kmax = kmax;
  rp.slots = slots;
  hipLaunchKernelGGL(search_rescore_kernel, dim3(rows), block, 0, s, rp);
  if (const hipError_t e = hipGetLastError()) return e;
  if (ev) (void)hipEventRecord(ev[2], s);
  return hipSuccess;
}

}  // namespace

extern "C" {

// Rows of fp32 [rows][D] on the device -> int8 codes [rows][D] and fp32 scales
// [rows] by the index rule of the header.  D a multiple of 16 in [16, 1024],
// src and codes 16-byte aligned.
int tcamd_search_quantize_q8(const float* src, int rows, int D, void* codes, float* scales, void* stream) {
  if (rows < 0 || D < 16 || D > 1024 || D % 16) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (!src || !codes || !scales || ((uintptr_t)src | (uintptr_t)codes) % 16 || (uintptr_t)scales % 4)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(search_quantize_q8_kernel, dim3((rows + kWaves - 1) / kWaves), dim3(64 * kWaves), 0,
                     (hipStream_t)stream, src, rows, D, (int8_t*)codes, scales);
  return hipGetLastError();
}

// The launch plan of tcamd_search_topk_q8's first launch, a function of (rows,
// N) alone (host only): a group is 16 query rows when rows <= 16, else 64;
// `slices` corpus slices of equal tile counts (the last may be short), at most
// 256 / groups.
int tcamd_search_q8_plan(int rows, int N, int* slices, int* group) {
  if (rows < 0 || rows > kMaxRows || N < 1 || !slices || !group) return hipErrorInvalidValue;
  *group = rows <= 16 ? 16 : 64;
  *slices = 0;
  if (rows == 0) return hipSuccess;
  const int groups = (rows + *group - 1) / *group;
  const int tiles = (int)(((int64_t)N + kTile - 1) / kTile);
  const int cap = kMaxSlices / groups;
  const int tps = (tiles + cap - 1) / cap;
  *slices = (tiles + tps - 1) / tps;
  return hipSuccess;
}

// Bytes of workspace that serve tcamd_search_topk_q8 at (rows, N) and at every
// smaller rows and N: the [rows][64] int32 shortlist, then the key lists by
// their bound rows * min(tiles, 256) (the plan's own rows * slices halves from
// 64 rows to 65), 64 keys each.
uint64_t tcamd_search_q8_workspace(int rows, int N) {
  if (rows < 0 || rows > kMaxRows || N < 1) return 0;
  uint64_t tiles = ((uint64_t)N + kTile - 1) / kTile;
  if (tiles > kMaxSlices) tiles = kMaxSlices;
  return (uint64_t)rows * kShort * 4 + (uint64_t)rows * tiles * kShort * 8;
}

// Row r of q (fp32 [rows][D], rows q_stride_bytes apart): its min(k_row[r],
// kmax) best corpus rows among the 64 that the int8 index (codes, scales)
// ranks first, scored and ordered as tcamd_search_topk does on the planes
// idx_hi / idx_lo, at indices[r][0 ..] / scores[r][0 ..] (rows of `slots`
// elements); ranks at and past min(N, 64) as (-1, -FLT_MAX); k_row[r] == 0
// skips the row and slots past a row's count are not written.  rows <= 128, D
// a multiple of 128 in [128, 1024], 1 <= N < 2^31, 1 <= kmax <= 16, kmax <=
// slots <= 64; q, its stride, the codes and the planes 16-byte aligned, the
// workspace 8, the rest 4.
int tcamd_search_topk_q8(const float* q, uint64_t q_stride_bytes, int rows, const void* codes, const float* scales,
                         const void* idx_hi, const void* idx_lo, int N, int D, const int32_t* k_row, int kmax,
                         int slots, void* workspace, int32_t* indices, float* scores, void* stream) {
  return topk_q8(q, q_stride_bytes, rows, codes, scales, idx_hi, idx_lo, N, D, k_row, kmax, slots, workspace, indices,
                 scores, stream, nullptr);
}

// The same call once, then a wait for it: us[0] = microseconds of the coarse
// launch, us[1] = of the shortlist and rescore launches, between device events
// (tools/search_bench.py).
int tcamd_search_topk_q8_timed(const float* q, uint64_t q_stride_bytes, int rows, const void* codes,
                               const float* scales, const void* idx_hi, const void* idx_lo, int N, int D,
                               const int32_t* k_row, int kmax, int slots, void* workspace, int32_t* indices,
                               float* scores, void* stream, float* us) {
  if (!us || rows < 1) return hipErrorInvalidValue;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int e = hipSuccess;
  for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
  if (e == hipSuccess)
    e = topk_q8(q, q_stride_bytes, rows, codes, scales, idx_hi, idx_lo, N, D, k_row, kmax, slots, workspace, indices,
                scores, stream, ev);
  if (e == hipSuccess) e = hipEventSynchronize(ev[2]);
  float ms[2] = {0.f, 0.f};
  if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], ev[0], ev[1]);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms[1], ev[1], ev[2]);
  us[0] = ms[0] * 1e3f;
  us[1] = ms[1] * 1e3f;
  for (int i = 0; i < 3; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return e;
}

}  // extern "C"
