// K35 — clustered (IVF) embedding search: list scan fused with top-K (gfx950).
//
// K33 (csrc/kernels/embed_search.hip) and K34 read the whole corpus for every
// query group.  Here the corpus is partitioned into nlist lists around
// centroids (ops.hip.search_index_ivf) and a query scans only the nprobe_row
// lists whose centroids K33 ranks first for it.  Row r gets K33's answer,
// indices and score bits, over the rows of those lists; with nprobe_row[r] ==
// nlist that is K33's answer over the whole corpus.
//
// The index: `cent`, K33's planes of the [nlist][D] centroids; `offsets` int32
// [nlist + 1] and `perm` int32 [N] (position p of list l, offsets[l] <= p <
// offsets[l + 1], holds original row perm[p], ascending inside a list); hi /
// lo planes of the permuted corpus, K33's split, zero rows up to 64 ceil(N /
// 64) + 64 so that a 64-row tile starting at any offsets[l] stays inside.
//
// Three launches, no atomics.  Workspace (tcamd_search_ivf_workspace): the
// probed list ids int32 [rows][64] and their scores fp32 [rows][64], then one
// area that first serves the coarse step as K33's workspace and then holds
// the scan's keys u64 [rows][pmax * parts][kmax].
//
// 1. Coarse: tcamd_search_topk itself over `cent` with k_row = nprobe_row and
//    kmax = pmax.  No device code of its own.
// 2. search_ivf_scan, grid (part, probe, row), 4 waves.  tcamd_search_ivf_plan
//    fixes parts = clamp(256 / (rows * pmax), 1, 4) from (rows, pmax) alone.
//    * A workgroup serves one query and one of `parts` equal runs of the tiles
//      of one probed list.  The list id and its offsets pair are read once,
//      wave-uniform.  A probe slot at or past min(nprobe_row, pmax), a list id
//      of -1 (K33's rank past nlist), k_row == 0 and a part with no tiles all
//      become "no tiles": the workgroup runs the same code, takes the same two
//      barriers and writes an all-zero key list.
//    * The query is split to hi / lo bf16 on the way into LDS, 256 B per
//      64-deep K slice (4 KB at D = 1024).  The A operand is K33's 16-row
//      block with the query in row 0: lanes with lane % 16 == 0 read their
//      16-B chunk, the others pass zero registers and read no LDS.
//    * Wave w streams rows 16 w .. + 15 of each 64-row tile of the list
//      through K33's ring (3 slots of 4 KB, LDS-DMA, two K slices in flight,
//      counted vmcnt, K33's chunk swizzle); the lane addresses start at row
//      offsets[l], not at a multiple of 64.
//    * A score is K33's own: x3_mma, the same operand roles, K ascending and
//      unsplit, one accumulator element (D row 0) of one wave.  So a (query,
//      corpus row) pair gets K33's bits whatever list, part or batch it is
//      met in.
//    * A tile gives a wave 16 scores (lanes 0 .. 15).  The wave holds back up
//      to four tiles, one per 16 lanes, and then selects on its own rows with
//      K33's compare, ballot and insert; there is no barrier in the tile loop.
//      Rows at or past the list's end belong to the next list or the padding
//      and are excluded by position, never by score.
//    * The four waves' sorted lists meet once in LDS (each wave's in its own
//      drained ring): a key's rank is its lane plus the keys above it in the
//      other three lists (binary searches), and ranks below kmax go to
//      ws[row][probe * parts + part].
//    LDS: D / 64 * 256 B + 48 KB, 52 KB at D = 1024: three workgroups a CU.
// 3. Merge: K33's search_merge_kernel (tcamd_search_merge) with slices = pmax
//    * parts <= 256.  Outputs are K33's: ranks past the candidates (-1,
//    -FLT_MAX), slots past a row's count unwritten.
//
// Deviation from the plan of the issue: while it selects, a wave keys a score
// with its position p, not with perm[p]; the survivors' positions are
// replaced by perm[p] once, before the four lists meet.  perm ascends inside
// a list, so the order and the keys that leave are the same, and no global
// load sits between the DMAs of the stream.
//
// Reference analog: none (the reference client runs no model).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/embed_search_common.h"

#define TCAMD_SEARCH_IVF_PMAX 64

extern "C" int tcamd_search_ivf_plan(int rows, int pmax, int* parts);

namespace {

using namespace tcamd_search;

constexpr int kTile = 64;                   // corpus rows of a tile
constexpr int kWaves = 4;                   // 16 corpus rows each
constexpr int kKW = 64;                     // k of one slice
constexpr int kRow = kKW * 2;               // bytes of one staged row
constexpr int kPlane = 16 * kRow;           // 16 rows of one plane (2 KB)
constexpr int kBuf = 2 * kPlane;            // hi | lo: one K slice of 16 rows (4 KB)
constexpr int kRing = 3;                    // ring slots of a wave
constexpr int kAhead = kRing - 1;           // K slices in flight
constexpr int kDma = 4;                     // LDS-DMAs of one K slice (1 KB each)
constexpr int kQ = 2 * kRow;                // the query's hi | lo of one K slice (256 B)
constexpr int kKmax = 64;                   // TCAMD_SEARCH_KMAX
constexpr int kMaxLists = 256;              // key lists of a row that the merge takes
constexpr int kMaxRows = 128;

constexpr size_t lds_bytes(int D) { return (size_t)(D / kKW) * kQ + kWaves * kRing * kBuf; }

struct IvfParams {
  const uint8_t* q;           // fp32 rows, q_stride bytes apart
  uint64_t q_stride;
  const uint16_t* c_hi;       // permuted planes [64 ceil(N / 64) + 64][D] bf16
  const uint16_t* c_lo;
  const int32_t* offsets;     // [nlist + 1]
  const int32_t* perm;        // [N]
  const int32_t* probes;      // [rows][pmax] list ids of the coarse step
  const int32_t* k_row;       // [rows]
  const int32_t* nprobe_row;  // [rows]
  uint64_t* ws;               // [rows][pmax * parts][kmax]
  int N, D, nlist, kmax, pmax, parts;
};

// keys above x in a list of 64 sorted descending (LDS)
__device__ __forceinline__ int above(const uint64_t* list, uint64_t x) {
  int n = 0;
#pragma unroll
  for (int step = 32; step > 0; step >>= 1)
    if (list[n + step - 1] > x) n += step;
  return n + (list[n] > x ? 1 : 0);  // n <= 63 here
}

__global__ void __launch_bounds__(64 * kWaves) search_ivf_scan_kernel(IvfParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int part = blockIdx.x, probe = blockIdx.y, row = blockIdx.z;
  const int nks = p.D / kKW;
  uint8_t* ql = lds;                                 // the query: [nks][hi | lo][128 B]
  uint8_t* rings = lds + (size_t)nks * kQ;
  uint8_t* ring = rings + wave * kRing * kBuf;       // this wave's ring

  // what this workgroup scans, wave-uniform: positions start .. end - 1 of the
  // permuted corpus, of which tiles t0 .. t0 + nt - 1 (64 positions from start)
  const int kk = __builtin_amdgcn_readfirstlane(min(p.k_row[row], p.kmax));
  const int np = __builtin_amdgcn_readfirstlane(min(p.nprobe_row[row], p.pmax));
  int start = 0, end = 0;
  if (kk > 0 && probe < np) {
    const int l = __builtin_amdgcn_readfirstlane(p.probes[(size_t)row * p.pmax + probe]);
    if (l >= 0 && l < p.nlist) {
      start = __builtin_amdgcn_readfirstlane(p.offsets[l]);
      end = __builtin_amdgcn_readfirstlane(p.offsets[l + 1]);
      if (start < 0 || end < start || end > p.N) start = end = 0;  // not an index of this corpus: nothing is read
    }
  }
  const int tiles = (end - start + kTile - 1) / kTile;
  const int tpp = (tiles + p.parts - 1) / p.parts;
  const int t0 = part * tpp;
  const int nt = max(0, min(tpp, tiles - t0));
  const int total = nt * nks;  // K slices of this wave's stream

  // corpus by LDS-DMA, K33's: instruction i fills rows 8 (i % 2) .. + 7 of
  // plane i / 2 lane-linear (row r8, chunk' c8) from global chunk c8 ^
  // swz(row).  Every row exists: a tile begins below N and the planes have 64
  // zero rows past 64 ceil(N / 64).
  const int r8 = lane >> 3, c8 = lane & 7;
  const uint16_t* csrc[kDma];
#pragma unroll
  for (int i = 0; i < kDma; ++i) {
    const int r = 8 * (i & 1) + r8;
    const size_t at = (size_t)start + (size_t)t0 * kTile + 16 * wave + r;  // this lane's row of the first tile
    csrc[i] = (i >> 1 ? p.c_lo : p.c_hi) + at * p.D + 8 * (c8 ^ swz(r));
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

  // the query, once: thread -> 8 consecutive d, fp32 -> hi / lo
  if (tid < p.D / 8) {
    const float* src = reinterpret_cast<const float*>(p.q + (size_t)row * p.q_stride) + 8 * tid;
    float f[8];
    *reinterpret_cast<f32x4*>(f) = *reinterpret_cast<const f32x4*>(src);
    *reinterpret_cast<f32x4*>(f + 4) = *reinterpret_cast<const f32x4*>(src + 4);
    v4u hi, lo;
    split8(f, hi, lo);
    uint8_t* dst = ql + (size_t)(tid >> 3) * kQ + ((tid & 7) << 4);
    *reinterpret_cast<v4u*>(dst) = hi;
    *reinterpret_cast<v4u*>(dst + kRow) = lo;
  }

  // fragment reads.  Corpus: lane (row lane % 16 of the 16-row block, k chunk
  // 4 ks + lane / 16).  Query: operand row 0 alone, so lanes 0, 16, 32, 48.
  int lofs[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) lofs[ks] = (lane & 15) * kRow + (((4 * ks + (lane >> 4)) ^ swz(lane & 15)) << 4);
  const bool qlane = (lane & 15) == 0;
  const int qofs = (lane >> 4) << 4;

  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the query writes
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  uint64_t kept = 0;  // this wave's best keys, sorted descending over the lanes, 0 = empty
  float pend = 0.f;   // the scores held back: tile (t & ~3) + lane / 16, row lane % 16 of this wave's 16
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
      const uint8_t* qb = ql + (size_t)ks * kQ + qofs;
      rslot = rslot + 1 == kRing ? 0 : rslot + 1;
      v4u qh[2], qlo[2], ch[2], clo[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        ch[s] = ld16(cb + lofs[s]);
        clo[s] = ld16(cb + kPlane + lofs[s]);
        qh[s] = qlo[s] = v4u{0u, 0u, 0u, 0u};
      }
      if (qlane) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          qh[s] = ld16(qb + 64 * s);
          qlo[s] = ld16(qb + kRow + 64 * s);
        }
      }
      // the fragments are in registers before the next step's DMA takes the slot
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // operand A = the query in row 0, B = the corpus rows: D row 0 (element 0
      // of lanes 0 .. 15), column lane % 16 a corpus row of this wave
#pragma unroll
      for (int s = 0; s < 2; ++s) acc = x3_mma(qh[s], qlo[s], ch[s], clo[s], acc);
    }

    const float v = __shfl(acc[0], lane & 15, 64);
    if ((lane >> 4) == (t & 3)) pend = v;
    if ((t & 3) != 3 && t != nt - 1) continue;  // wave-uniform: hold the tile back
    const int tl = (t & ~3) + (lane >> 4);
    const uint32_t pos = (uint32_t)start + (uint32_t)(t0 + tl) * kTile + 16 * wave + (lane & 15);
    const uint64_t key = tl <= t && pos < (uint32_t)end ? topk_key(__float_as_uint(pend), pos) : 0;
    uint64_t thr = lane_u64(kept, kk - 1);  // nt > 0 only where kk > 0
    uint64_t m = __ballot(key > thr);
    while (m) {
      const int b = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const uint64_t cand = lane_u64(key, b);
      if (cand > thr) {
        kept = insert_key(kept, cand, lane);
        thr = lane_u64(kept, kk - 1);
      }
    }
  }

  // positions -> original rows (perm ascends inside a list: the order stays),
  // then the four sorted lists meet, each in its wave's ring: the stream has
  // drained (the last step waited for vmcnt(0)) and its fragments are read
  if (kept) {
    const uint32_t pos = 0xFFFFFFFFu - (uint32_t)kept;  // < end <= N
    kept = (kept & 0xFFFFFFFF00000000ull) | (uint64_t)(0xFFFFFFFFu - (uint32_t)p.perm[pos]);
  }
  reinterpret_cast<uint64_t*>(ring)[lane] = kept;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  // keys are unique, so the nonzero ranks are; an empty slot's rank is at or
  // past the number of keys, and the empty slots of a wave cover every rank
  // from there to 63 at least: each of the kmax slots is written
  int rank = lane;
#pragma unroll
  for (int w = 0; w < kWaves; ++w)
    if (w != wave) rank += above(reinterpret_cast<const uint64_t*>(rings + w * kRing * kBuf), kept);
  const size_t list = ((size_t)row * p.pmax + probe) * p.parts + part;
  if (rank < p.kmax) p.ws[list * p.kmax + rank] = kept;
}

// per row: the probed list ids, and as much again for their scores
constexpr uint64_t kProbeBytes = (uint64_t)TCAMD_SEARCH_IVF_PMAX * 4;

}  // namespace

extern "C" {

// The launch plan of tcamd_search_topk_ivf's scan, a function of (rows, pmax)
// alone (host only): each probed list is dealt to `parts` workgroups.
int tcamd_search_ivf_plan(int rows, int pmax, int* parts) {
  if (rows < 0 || rows > kMaxRows || pmax < 1 || pmax > TCAMD_SEARCH_IVF_PMAX || !parts) return hipErrorInvalidValue;
  *parts = 0;
  if (rows == 0) return hipSuccess;
  const int n = kMaxLists / (rows * pmax);
  *parts = n < 1 ? 1 : (n > 4 ? 4 : n);
  return hipSuccess;
}

// Bytes of workspace that serve tcamd_search_topk_ivf at (rows, nlist),
// whatever pmax and kmax, and at every smaller rows as well: the probed list
// ids and scores, then the larger of the coarse step's K33 workspace and 256
// key lists a row.  Every term grows with rows.
uint64_t tcamd_search_ivf_workspace(int rows, int nlist) {
  if (rows < 0 || rows > kMaxRows || nlist < 1) return 0;
  const uint64_t coarse = tcamd_search_workspace(rows, nlist);
  const uint64_t keys = (uint64_t)rows * kMaxLists * kKmax * 8;
  return 2 * rows * kProbeBytes + (coarse > keys ? coarse : keys);
}

// tcamd_search_topk over the rows of the nprobe_row[r] lists (at most pmax)
// whose centroids K33 ranks first for row r.  q, q_stride_bytes, rows, D,
// k_row, kmax, indices, scores and stream are tcamd_search_topk's.  cent_hi /
// cent_lo: K33's planes of the [nlist][D] centroids; idx_hi / idx_lo: planes
// of the permuted corpus [64 ceil(N / 64) + 64][D]; offsets int32 [nlist + 1],
// perm int32 [N], nprobe_row int32 [rows], all on the device.  1 <= pmax <= 64,
// 1 <= nlist <= N; the alignment rules are K33's, 4 bytes for offsets, perm
// and nprobe_row; workspace of tcamd_search_ivf_workspace(rows, nlist) bytes.
int tcamd_search_topk_ivf(const float* q, uint64_t q_stride_bytes, int rows, const void* cent_hi, const void* cent_lo,
                          int nlist, const void* idx_hi, const void* idx_lo, const int32_t* offsets,
                          const int32_t* perm, int N, int D, const int32_t* k_row, const int32_t* nprobe_row, int kmax,
                          int pmax, void* workspace, int32_t* indices, float* scores, void* stream) {
  if (rows < 0 || rows > kMaxRows || N < 1 || nlist < 1 || nlist > N || D < kKW || D > 1024 || D % kKW || kmax < 1 ||
      kmax > kKmax || pmax < 1 || pmax > TCAMD_SEARCH_IVF_PMAX)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (!q || !cent_hi || !cent_lo || !idx_hi || !idx_lo || !offsets || !perm || !k_row || !nprobe_row || !workspace ||
      !indices || !scores)
    return hipErrorInvalidValue;
  if (((uintptr_t)q | (uintptr_t)cent_hi | (uintptr_t)cent_lo | (uintptr_t)idx_hi | (uintptr_t)idx_lo |
       q_stride_bytes) % 16 ||
      (uintptr_t)workspace % 8 ||
      ((uintptr_t)offsets | (uintptr_t)perm | (uintptr_t)k_row | (uintptr_t)nprobe_row | (uintptr_t)indices |
       (uintptr_t)scores) % 4)
    return hipErrorInvalidValue;
  if (rows > 1 && q_stride_bytes < (uint64_t)D * 4) return hipErrorInvalidValue;
  IvfParams p;
  if (const int e = tcamd_search_ivf_plan(rows, pmax, &p.parts)) return e;
  uint8_t* ws = (uint8_t*)workspace;
  int32_t* probes = (int32_t*)ws;
  float* probe_scores = (float*)(ws + rows * kProbeBytes);
  uint64_t* keys = (uint64_t*)(ws + 2 * rows * kProbeBytes);
  // 1. the lists to probe: K33 over the centroids (its workspace is free again
  //    when its merge has run, before the scan writes its keys there)
  if (const int e = tcamd_search_topk(q, q_stride_bytes, rows, cent_hi, cent_lo, nlist, D, nprobe_row, pmax, keys,
                                      probes, probe_scores, stream))
    return e;
  p.q = reinterpret_cast<const uint8_t*>(q);
  p.q_stride = q_stride_bytes;
  p.c_hi = (const uint16_t*)idx_hi;
  p.c_lo = (const uint16_t*)idx_lo;
  p.offsets = offsets;
  p.perm = perm;
  p.probes = probes;
  p.k_row = k_row;
  p.nprobe_row = nprobe_row;
  p.ws = keys;
  p.N = N;
  p.D = D;
  p.nlist = nlist;
  p.kmax = kmax;
  p.pmax = pmax;
  hipLaunchKernelGGL(search_ivf_scan_kernel, dim3(p.parts, pmax, rows), dim3(64 * kWaves), lds_bytes(D),
                     (hipStream_t)stream, p);
  if (const hipError_t e = hipGetLastError()) return e;
  return tcamd_search_merge(keys, k_row, rows, pmax * p.parts, kmax, indices, scores, stream);
}

}  // extern "C"
