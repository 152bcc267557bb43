// K33 — embedding search: fused bf16x3 similarity + top-K (gfx950).
//
//   score(q, c) = sum_d q[d] * c[d]        q fp32 [rows <= 128][D], corpus [N][D]
//
// as the split-precision product of K10c (csrc/kernels/densenet_head.hip):
// q_lo*c_hi + q_hi*c_lo + q_hi*c_hi on v_mfma_f32_16x16x32_bf16, fp32
// accumulate.  Query row r gets its min(k_row[r], kmax) best corpus rows in
// K19's order (csrc/kernels/topk.hip): every (score, corpus index) becomes the
// unique 64-bit key  monotone_u32(score) << 32 | (0xFFFFFFFF - index)  and
// "largest key" is the whole contract.  The [rows, N] score matrix never
// exists: the corpus is read once per query group and what leaves the chip is
// kmax keys per (row, slice).
//
// The corpus is an index built once (ops.hip.search_index): bf16 hi / lo
// planes [64 ceil(N / 64)][D], RNE both, zero rows past N.  Pad rows are
// excluded by their index (>= N), never by their score.
//
// Two launches, no atomics, workspace u64 [rows][slices][kmax] from the caller
// (tcamd_search_workspace: a size that also covers every smaller batch).
//
// 1. search_partial, grid = query groups (x) by corpus slices (y), 4 waves.
//    tcamd_search_plan fixes both from (rows, N) alone: a group is 16 query
//    rows; the ceil(N / 64) tiles are dealt to at most 256 / groups slices of
//    equal tile counts (one workgroup per CU holds the LDS below, and x runs
//    fastest so that the groups of one slice read it at the same time).
//    * The workgroup's 16 queries stay in LDS for the whole launch: the fp32
//      rows are read once and split into hi / lo bf16 on the way in (rows past
//      `rows` become zeros).  Per 64-deep K slice a hi and a lo block of 16
//      rows of 128 B, the 16-B chunks XOR-swizzled by (row >> 1) & 7 as in
//      K18 / K10c.
//    * The slice is walked in tiles of 64 corpus rows.  Wave w owns rows
//      16 w .. 16 w + 15 of the tile over the whole of D and streams their
//      hi / lo planes by LDS-DMA (global_load_lds_dwordx4, 4 per K slice)
//      into a ring of its own: 3 slots of 4 KB, two K slices in flight under
//      the current one's MFMAs, the stream running on across tile ends.  The
//      wave waits on counted vmcnt; there is no workgroup barrier in the K
//      loop.  A score is one accumulator element of one wave, summed over d
//      in ascending order: K is not split, so its bits depend on the two
//      vectors alone -- not on the batch, the row's place in it, the corpus
//      index or the slice.
//    * After a tile the waves put the 16 x 64 scores into an LDS tile (two of
//      them, used in turn, so that one barrier per tile is enough: a tile is
//      rewritten two barriers after it was read).  Each wave then owns 4
//      queries and holds each one's best keys sorted over its 64 lanes (2
//      VGPRs per query, 0 = empty).  Lane j forms the key of score j with the
//      global corpus index, compares it with the query's worst kept key
//      (lane min(k_row, kmax) - 1), and a ballot gives the survivors; each is
//      inserted with two compares, one shift up by a lane and a select.
//    * The barrier is reached by every wave the same number of times: the
//      tile loop's bounds come from blockIdx and the launch parameters only,
//      and the branches on a query (row past `rows`, k_row == 0, survivors)
//      enclose no barrier.
//    LDS at D = 1024: queries 16 x 1024 x 2 planes x 2 B = 64 KB, rings
//    4 waves x 3 x 4 KB = 48 KB, score tiles 2 x 4 KB = 8 KB: 120 KB of the
//    160 KB.  A group of 32 would need 128 + 48 + 16 = 192 KB (176 KB with
//    rings of 2), so the group is 16.
// 2. search_merge, one wave per query row.  Every slice's keys are sorted, so
//    lane l keeps the heads of slices l, l + 64, ... (at most 4: slices <=
//    256) and round j takes the largest head by the 64-bit butterfly maximum
//    -- K19's "largest key strictly below round j - 1's" over sorted lists --
//    whose owner writes index and score (the fp32 bits back out of the key's
//    monotone image; both zeros come back as +0.0) and moves on.  Ranks at and
//    past N get (-1, -FLT_MAX), K27's convention; slots past a row's count
//    are never written, K19's.
//
// No fp32 VALU sum takes part in a score, so the file needs none of K10c's
// build flags.
//
// Reference analog: none (the reference client runs no model).

#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <cstdint>

#include "kernels/embed_search_common.h"

#define TCAMD_SEARCH_KMAX 64  // TCAMD_TOPK_KMAX

namespace {

using namespace tcamd_search;  // the helpers K34 shares: kernels/embed_search_common.h

constexpr int kG = 16;                      // query rows of a workgroup
constexpr int kTile = 64;                   // corpus rows of a tile
constexpr int kWaves = 4;                   // 16 corpus rows each
constexpr int kKW = 64;                     // k of one slice
constexpr int kRow = kKW * 2;               // bytes of one staged row
constexpr int kPlane = 16 * kRow;           // 16 rows of one plane (2 KB)
constexpr int kBuf = 2 * kPlane;            // hi | lo: one K slice of 16 rows (4 KB)
constexpr int kRing = 3;                    // ring slots of a wave
constexpr int kAhead = kRing - 1;           // K slices in flight
constexpr int kDma = 4;                     // LDS-DMAs of one K slice (1 KB each)
constexpr int kScore = kG * kTile * 4;      // one score tile (4 KB)
constexpr int kMaxSlices = 256;             // 4 heads per lane in the merge
constexpr int kMaxRows = 128;
constexpr int kMaxDevices = 64;             // host-side per-device cache of the LDS opt-in

constexpr size_t lds_bytes(int D) { return (size_t)(D / kKW) * kBuf + kWaves * kRing * kBuf + 2 * kScore; }

struct SearchParams {
  const uint8_t* q;       // fp32 rows, q_stride bytes apart
  uint64_t q_stride;
  const uint16_t* c_hi;   // [64 ceil(N / 64)][D] bf16
  const uint16_t* c_lo;
  const int32_t* k_row;   // [rows]
  uint64_t* ws;           // [rows][slices][kmax]
  int rows, N, D, kmax, slices, tps;  // tps: tiles per slice
};

__global__ void __launch_bounds__(64 * kWaves) search_partial_kernel(SearchParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.x * kG, slice = blockIdx.y;
  const int nks = p.D / kKW;
  uint8_t* ql = lds;                                          // queries: [nks][hi | lo][16][128 B]
  uint8_t* ring = lds + (size_t)nks * kBuf + wave * kRing * kBuf;  // this wave's ring
  float* sc = reinterpret_cast<float*>(lds + (size_t)nks * kBuf + kWaves * kRing * kBuf);

  const int tiles = (p.N + kTile - 1) / kTile;
  const int t0 = slice * p.tps;
  const int nt = min(p.tps, tiles - t0);  // >= 1 by the plan
  const int total = nt * nks;             // K slices of this wave's stream

  // corpus by LDS-DMA: instruction i fills rows 8 (i % 2) .. + 7 of plane i / 2
  // lane-linear (row r8, chunk' c8) from global chunk c8 ^ swz(row).  Every
  // row exists: the planes are padded to a multiple of 64 rows.
  const int r8 = lane >> 3, c8 = lane & 7;
  const uint16_t* csrc[kDma];
#pragma unroll
  for (int i = 0; i < kDma; ++i) {
    const int row = 8 * (i & 1) + r8;
    csrc[i] = (i >> 1 ? p.c_lo : p.c_hi) + ((size_t)t0 * kTile + 16 * wave + row) * p.D + 8 * (c8 ^ swz(row));
  }
  size_t iadd = 0;  // elements from csrc to the next K slice to issue
  int issued = 0, ik = 0, islot = 0;
  auto issue = [&]() {
    uint8_t* dst = ring + islot * kBuf;
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

  // the queries, once: thread -> (row, 8 consecutive d), fp32 -> hi / lo
  const int cpr = p.D / 8;  // 16-B bf16 chunks of a row
  for (int it = tid; it < kG * cpr; it += 64 * kWaves) {
    const int row = it / cpr, c = it - row * cpr;
    v4u hi = v4u{0u, 0u, 0u, 0u}, lo = hi;
    if (q0 + row < p.rows) {
      const float* src = reinterpret_cast<const float*>(p.q + (size_t)(q0 + row) * p.q_stride) + 8 * c;
      float f[8];
      *reinterpret_cast<f32x4*>(f) = *reinterpret_cast<const f32x4*>(src);
      *reinterpret_cast<f32x4*>(f + 4) = *reinterpret_cast<const f32x4*>(src + 4);
      split8(f, hi, lo);
    }
    uint8_t* dst = ql + (size_t)(c >> 3) * kBuf + row * kRow + (((c & 7) ^ swz(row)) << 4);
    *reinterpret_cast<v4u*>(dst) = hi;
    *reinterpret_cast<v4u*>(dst + kPlane) = lo;
  }

  // this wave's 4 queries of the selection: rows q0 + 4 wave + i
  int kk[4];
  uint64_t kept[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = q0 + 4 * wave + i;
    kk[i] = r < p.rows ? __builtin_amdgcn_readfirstlane(min(p.k_row[r], p.kmax)) : 0;
    kept[i] = 0;
  }

  // fragment reads: lane (row lane % 16 of a 16-row block, k chunk 4 ks + lane / 16)
  int lofs[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) lofs[ks] = (lane & 15) * kRow + (((4 * ks + (lane >> 4)) ^ swz(lane & 15)) << 4);

  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the query writes
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  int rslot = 0;
  for (int t = 0; t < nt; ++t) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nks; ++ks) {
      // the slot read in the last step takes the K slice kAhead steps on; then
      // this step's slice has landed once at most kAhead slices are in flight
      if (issued < total) {  // wave-uniform
        issue();
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kAhead * kDma) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      const uint8_t* cb = ring + rslot * kBuf;
      const uint8_t* qb = ql + (size_t)ks * kBuf;
      rslot = rslot + 1 == kRing ? 0 : rslot + 1;
      v4u qh[2], qlo[2], ch[2], clo[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        ch[s] = ld16(cb + lofs[s]);
        clo[s] = ld16(cb + kPlane + lofs[s]);
        qh[s] = ld16(qb + lofs[s]);
        qlo[s] = ld16(qb + kPlane + lofs[s]);
      }
      // the fragments are in registers before the next step's DMA takes the slot
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // operand A = the queries, B = the corpus rows: D row 4 (lane / 16) + e
      // is a query, D column lane % 16 a corpus row of this wave
#pragma unroll
      for (int s = 0; s < 2; ++s) acc = x3_mma(qh[s], qlo[s], ch[s], clo[s], acc);
    }

    float* st = sc + (t & 1) * (kG * kTile);
#pragma unroll
    for (int e = 0; e < 4; ++e) st[(4 * (lane >> 4) + e) * kTile + 16 * wave + (lane & 15)] = acc[e];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the DMAs in flight go to the wave's own ring: no vmcnt wait here
    asm volatile("" ::: "memory");

    const uint32_t idx = (uint32_t)(t0 + t) * kTile + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (kk[i] <= 0) continue;  // wave-uniform
      const float s = st[(4 * wave + i) * kTile + lane];
      const uint64_t key = idx < (uint32_t)p.N ? topk_key(__float_as_uint(s), idx) : 0;
      uint64_t thr = lane_u64(kept[i], kk[i] - 1);
      uint64_t m = __ballot(key > thr);
      while (m) {
        const int b = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint64_t cand = lane_u64(key, b);
        if (cand > thr) {
          kept[i] = insert_key(kept[i], cand, lane);
          thr = lane_u64(kept[i], kk[i] - 1);
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (kk[i] <= 0) continue;
    const size_t r = q0 + 4 * wave + i;
    if (lane < p.kmax) p.ws[(r * p.slices + slice) * p.kmax + lane] = kept[i];
  }
}

__global__ void __launch_bounds__(64 * kWaves)
search_merge_kernel(const uint64_t* __restrict__ ws, const int32_t* __restrict__ k_row, int rows, int slices, int kmax,
                    int32_t* __restrict__ indices, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int k = min(k_row[r], kmax);
  if (k <= 0) return;
  const uint64_t* row = ws + (size_t)r * slices * kmax;
  uint64_t head[kMaxSlices / 64];
  int at[kMaxSlices / 64];
#pragma unroll
  for (int i = 0; i < kMaxSlices / 64; ++i) {
    const int s = lane + 64 * i;
    at[i] = 0;
    head[i] = s < slices ? row[(size_t)s * kmax] : 0;
  }
  int j = 0;
  for (; j < k; ++j) {
    uint64_t best = 0;
#pragma unroll
    for (int i = 0; i < kMaxSlices / 64; ++i) best = head[i] > best ? head[i] : best;
    const uint64_t win = wave_max_u64(best);
    if (win == 0) break;  // the corpus has fewer than k rows
#pragma unroll
    for (int i = 0; i < kMaxSlices / 64; ++i) {
      if (head[i] != win) continue;  // keys are unique: one head of one lane
      const uint32_t m = (uint32_t)(win >> 32);
      indices[(size_t)r * kmax + j] = (int32_t)(0xFFFFFFFFu - (uint32_t)win);
      scores[(size_t)r * kmax + j] = __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
      ++at[i];
      head[i] = at[i] < kmax ? row[(size_t)(lane + 64 * i) * kmax + at[i]] : 0;
    }
  }
  for (j += lane; j < k; j += 64) {
    indices[(size_t)r * kmax + j] = -1;
    scores[(size_t)r * kmax + j] = -FLT_MAX;
  }
}

}  // namespace

extern "C" {

// The launch plan of tcamd_search_topk, a function of (rows, N) alone (host
// only): `slices` corpus slices of equal tile counts (the last may be short)
// by ceil(rows / group) query groups.
int tcamd_search_plan(int rows, int N, int* slices, int* group) {
  if (rows < 0 || rows > kMaxRows || N < 1 || !slices || !group) return hipErrorInvalidValue;
  *group = kG;
  *slices = 0;
  if (rows == 0) return hipSuccess;
  const int groups = (rows + kG - 1) / kG;
  const int tiles = (int)(((int64_t)N + kTile - 1) / kTile);
  const int cap = kMaxSlices / groups;
  const int tps = (tiles + cap - 1) / cap;
  *slices = (tiles + tps - 1) / tps;
  return hipSuccess;
}

// Bytes of workspace that serve tcamd_search_topk at (rows, N), whatever kmax,
// and at every smaller rows and N as well.  The plan's own rows * slices is
// not monotone in rows (fewer query groups get more slices), so the size goes
// by its bound: slices <= tiles, and rows * slices <= 16 groups * (256 /
// groups) = 4096 key lists; both grow with rows and with N.
uint64_t tcamd_search_workspace(int rows, int N) {
  if (rows < 0 || rows > kMaxRows || N < 1) return 0;
  const uint64_t tiles = ((uint64_t)N + kTile - 1) / kTile;
  uint64_t lists = (uint64_t)rows * tiles;
  if (lists > (uint64_t)kG * kMaxSlices) lists = (uint64_t)kG * kMaxSlices;
  return lists * TCAMD_SEARCH_KMAX * 8;
}

// The second launch alone, for K35 (embed_search_ivf.hip), whose key lists
// have K33's layout: ws u64 [rows][slices][kmax], every list sorted descending
// and 0 = empty, slices <= 256.  The caller has checked the other arguments.
int tcamd_search_merge(const void* ws, const int32_t* k_row, int rows, int slices, int kmax, int32_t* indices,
                       float* scores, void* stream) {
  if (slices < 1 || slices > kMaxSlices) return hipErrorInvalidValue;
  hipLaunchKernelGGL(search_merge_kernel, dim3((rows + kWaves - 1) / kWaves), dim3(64 * kWaves), 0,
                     (hipStream_t)stream, (const uint64_t*)ws, k_row, rows, slices, kmax, indices, scores);
  return hipGetLastError();
}

// Row r of q (fp32 [rows][D], rows q_stride_bytes apart) against the index
// planes idx_hi / idx_lo (bf16 [64 ceil(N / 64)][D], zero rows past N): its
// min(k_row[r], kmax) best corpus rows at indices[r][0 ..] / scores[r][0 ..]
// (rows of kmax slots), ranks at and past N as (-1, -FLT_MAX); k_row[r] == 0
// skips the row and slots past a row's count are not written.  rows <= 128,
// D a multiple of 64 in [64, 1024], 1 <= N < 2^31, 1 <= kmax <= 64; q, its
// stride and the planes 16-byte aligned, the workspace 8, the rest 4.
int tcamd_search_topk(const float* q, uint64_t q_stride_bytes, int rows, const void* idx_hi, const void* idx_lo, int N,
                      int D, const int32_t* k_row, int kmax, void* workspace, int32_t* indices, float* scores,
                      void* stream) {
  if (rows < 0 || rows > kMaxRows || N < 1 || D < kKW || D > 1024 || D % kKW || kmax < 1 || kmax > TCAMD_SEARCH_KMAX)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (!q || !idx_hi || !idx_lo || !k_row || !workspace || !indices || !scores) return hipErrorInvalidValue;
  if (((uintptr_t)q | (uintptr_t)idx_hi | (uintptr_t)idx_lo | q_stride_bytes) % 16 || (uintptr_t)workspace % 8 ||
      ((uintptr_t)k_row | (uintptr_t)indices | (uintptr_t)scores) % 4)
    return hipErrorInvalidValue;
  if (rows > 1 && q_stride_bytes < (uint64_t)D * 4) return hipErrorInvalidValue;
  // the dynamic-LDS opt-in is per device
  static std::atomic<bool> attr[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  if (!attr[dev].load(std::memory_order_acquire)) {
    const hipError_t e = hipFuncSetAttribute((const void*)search_partial_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(1024));
    if (e != hipSuccess) return e;
    attr[dev].store(true, std::memory_order_release);
  }
  SearchParams p;
  int group = 0;
  if (const int e = tcamd_search_plan(rows, N, &p.slices, &group)) return e;
  const int tiles = (int)(((int64_t)N + kTile - 1) / kTile);
  p.tps = (tiles + p.slices - 1) / p.slices;
  p.q = reinterpret_cast<const uint8_t*>(q);
  p.q_stride = q_stride_bytes;
  p.c_hi = (const uint16_t*)idx_hi;
  p.c_lo = (const uint16_t*)idx_lo;
  p.k_row = k_row;
  p.ws = (uint64_t*)workspace;
  p.rows = rows;
  p.N = N;
  p.D = D;
  p.kmax = kmax;
  hipLaunchKernelGGL(search_partial_kernel, dim3((rows + group - 1) / group, p.slices), dim3(64 * kWaves), lds_bytes(D),
                     (hipStream_t)stream, p);
  if (const hipError_t e = hipGetLastError()) return e;
  return tcamd_search_merge(workspace, k_row, rows, p.slices, kmax, indices, scores, stream);
}

}  // extern "C"
