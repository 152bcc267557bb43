// K26 compare_expected — outputs against their expectations, both in device
// memory, by the rule of kernels/compare_math.h (which the host compiles too:
// csrc/host/compare.cc; contract: tests/compare_cases.py).  One launch takes a
// table of up to 64 pairs {got, expected, count, dtype}, a request's outputs,
// and writes one record per pair: the mismatches, the lowest mismatching element
// index, the largest |got - exp| over the finite pairs, and the bits of the two
// elements at that index.
//
// The kernel is bound by memory and by its launch.  A pair of up to kBlockBytes
// takes one workgroup, a larger one a workgroup per kBlockBytes (at most
// kMaxBlocksPerPair, grid-strided beyond).  A workgroup finds its pair in a table
// of first-block numbers in the kernel arguments.
//
// A pointer may sit at any element-aligned address.  The elements before got's
// first 16-byte boundary (fewer than 16) and those after its last whole 16 bytes
// go one per lane; the body is read 16 bytes a lane, got with aligned loads and
// expected with the widest loads its own address allows when got's is aligned
// (16, 8, 4, 2 or 1 bytes: the two pointers may be misaligned differently).
// Units whose bytes are all equal are not looked at element by element.
//
// Every lane keeps a count, a lowest index and a largest difference; they are
// reduced in the wave by shuffles, across the four waves through LDS, and lane 0
// finishes.  When every pair of the call has one workgroup, that is a plain
// store of the whole record, the two elements included, and the call is one
// launch.  Otherwise the records are cleared by a launch before, each workgroup
// issues at most one atomic add, one atomic min and one atomic max, and a launch
// after fetches the two elements of each pair's lowest index.

#include "kernels/common.h"
#include "kernels/compare_math.h"

using namespace tcamd;
using namespace tcamd_cmp;

namespace {

constexpr int kUnit = 16;                          // bytes a lane reads of got per step
constexpr uint64_t kBlockBytes = 32 * 1024;        // of got, per workgroup
constexpr uint32_t kMaxBlocksPerPair = 1024;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;

struct CompareParams {
  const uint8_t* got[kMaxPairs];
  const uint8_t* exp[kMaxPairs];
  uint64_t count[kMaxPairs];
  uint32_t first_block[kMaxPairs + 1];  // pair p owns blocks [first_block[p], first_block[p + 1])
  int8_t kind[kMaxPairs];
  int32_t n_pairs;
  int32_t atomic;  // several workgroups on some pair: accumulate into cleared records
  Tol tol;
  TcamdCompareRecord* rec;
};

struct Acc {
  uint64_t n, first;
  double maxd;
};

template <int A>
struct __attribute__((packed, aligned(A))) Vec16 {
  uint64_t q[2];
};

// 16 bytes at p, which is aligned to `align` (a power of two up to 16)
__device__ __forceinline__ void load16(const uint8_t* p, int align, uint64_t* q) {
  if (align >= 16) {
    const Vec16<16> v = *reinterpret_cast<const Vec16<16>*>(p);
    q[0] = v.q[0], q[1] = v.q[1];
  } else if (align == 8) {
    const Vec16<8> v = *reinterpret_cast<const Vec16<8>*>(p);
    q[0] = v.q[0], q[1] = v.q[1];
  } else if (align == 4) {
    const Vec16<4> v = *reinterpret_cast<const Vec16<4>*>(p);
    q[0] = v.q[0], q[1] = v.q[1];
  } else if (align == 2) {
    const Vec16<2> v = *reinterpret_cast<const Vec16<2>*>(p);
    q[0] = v.q[0], q[1] = v.q[1];
  } else {
    const Vec16<1> v = *reinterpret_cast<const Vec16<1>*>(p);
    q[0] = v.q[0], q[1] = v.q[1];
  }
}

template <int KIND>
__device__ __forceinline__ void fold(Acc& a, uint64_t idx, uint64_t g, uint64_t e, const Tol& t) {
  double d;
  if (!pass_bits<KIND>(g, e, t, &d)) {
    ++a.n;
    if (idx < a.first) a.first = idx;
  }
  if (d > a.maxd) a.maxd = d;
}

template <int KIND>
__device__ __forceinline__ void compare_pair(Acc& a, const uint8_t* got, const uint8_t* exp, uint64_t count,
                                             uint32_t blk, uint32_t nblk, const Tol& t) {
  constexpr int W = (KIND == kBytes1) ? 1 : (KIND == kBytes2 || KIND == kF16 || KIND == kB16) ? 2
                    : (KIND == kBytes4 || KIND == kF32) ? 4 : 8;
  constexpr int PER = kUnit / W;  // elements of a unit
  constexpr uint64_t MASK = W == 8 ? ~0ull : ((1ull << (8 * (W & 7))) - 1);
  const uint64_t bytes = count * W;
  uint64_t head = (uint64_t)(-(intptr_t)(uintptr_t)got) & (kUnit - 1);  // a multiple of W: got is element-aligned
  if (head > bytes) head = bytes;
  const uint64_t head_elems = head / W;
  const uint64_t units = (bytes - head) / kUnit;
  const uint64_t tail0 = head_elems + units * PER;  // first element of the tail
  const uint8_t* gb = got + head;
  const uint8_t* eb = exp + head;
  const uintptr_t lowbits = (uintptr_t)eb & (kUnit - 1);
  const int ealign = lowbits ? (int)(lowbits & (~lowbits + 1)) : kUnit;

  // the body: units blk * kBlock + tid, then every nblk * kBlock further
  for (uint64_t u = (uint64_t)blk * kBlock + threadIdx.x; u < units; u += (uint64_t)nblk * kBlock) {
    const Vec16<16> gv = *reinterpret_cast<const Vec16<16>*>(gb + u * kUnit);
    uint64_t ev[2];
    load16(eb + u * kUnit, ealign, ev);
    if (gv.q[0] == ev[0] && gv.q[1] == ev[1]) continue;  // equal bits pass and differ by 0 (or are not finite)
    const uint64_t i0 = head_elems + u * PER;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int q = k * W / 8, sh = (k * W % 8) * 8;
      fold<KIND>(a, i0 + k, (gv.q[q] >> sh) & MASK, (ev[q] >> sh) & MASK, t);
    }
  }
  // head and tail: fewer than 16 elements each, one per lane of the pair's first workgroup
  if (blk == 0) {
    const uint64_t tail_elems = count - tail0;
    if (threadIdx.x < head_elems) {
      const uint64_t i = threadIdx.x;
      fold<KIND>(a, i, load_bits(got + i * W, W), load_bits(exp + i * W, W), t);
    } else if (threadIdx.x >= kWave && threadIdx.x - kWave < tail_elems) {
      const uint64_t i = tail0 + (threadIdx.x - kWave);
      fold<KIND>(a, i, load_bits(got + i * W, W), load_bits(exp + i * W, W), t);
    }
  }
}

__global__ void __launch_bounds__(kBlock) compare_expected(CompareParams p) {
  __shared__ Acc part[kWaves];
  int pair = 0;
  while (pair + 1 < p.n_pairs && blockIdx.x >= p.first_block[pair + 1]) ++pair;
  const uint32_t blk = blockIdx.x - p.first_block[pair];
  const uint32_t nblk = p.first_block[pair + 1] - p.first_block[pair];
  const uint8_t* got = p.got[pair];
  const uint8_t* exp = p.exp[pair];
  const uint64_t count = p.count[pair];
  const int kind = p.kind[pair];

  Acc a = {0, kNoIndex, 0.0};
  switch (kind) {
    case kBytes1: compare_pair<kBytes1>(a, got, exp, count, blk, nblk, p.tol); break;
    case kBytes2: compare_pair<kBytes2>(a, got, exp, count, blk, nblk, p.tol); break;
    case kBytes4: compare_pair<kBytes4>(a, got, exp, count, blk, nblk, p.tol); break;
    case kBytes8: compare_pair<kBytes8>(a, got, exp, count, blk, nblk, p.tol); break;
    case kF16: compare_pair<kF16>(a, got, exp, count, blk, nblk, p.tol); break;
    case kB16: compare_pair<kB16>(a, got, exp, count, blk, nblk, p.tol); break;
    case kF32: compare_pair<kF32>(a, got, exp, count, blk, nblk, p.tol); break;
    default: compare_pair<kF64>(a, got, exp, count, blk, nblk, p.tol); break;
  }

#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const uint64_t n = __shfl_down((unsigned long long)a.n, off);
    const uint64_t f = __shfl_down((unsigned long long)a.first, off);
    const double d = __shfl_down(a.maxd, off);
    a.n += n;
    if (f < a.first) a.first = f;
    if (d > a.maxd) a.maxd = d;
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) part[wave] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < kWaves; ++w) {
    a.n += part[w].n;
    if (part[w].first < a.first) a.first = part[w].first;
    if (part[w].maxd > a.maxd) a.maxd = part[w].maxd;
  }
  TcamdCompareRecord* r = p.rec + pair;
  if (!p.atomic) {
    const int w = kind_width(kind);
    TcamdCompareRecord out;
    out.mismatches = a.n;
    out.first_index = a.first;
    out.max_abs_diff = a.maxd;
    out.got_bits = a.first != kNoIndex ? load_bits(got + a.first * w, w) : 0;
    out.expected_bits = a.first != kNoIndex ? load_bits(exp + a.first * w, w) : 0;
    *r = out;
    return;
  }
  // the differences are not negative, so their bits order as unsigned integers do
  if (a.n) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->mismatches), (unsigned long long)a.n);
    atomicMin(reinterpret_cast<unsigned long long*>(&r->first_index), (unsigned long long)a.first);
  }
  if (a.maxd > 0.0)
    atomicMax(reinterpret_cast<unsigned long long*>(&r->max_abs_diff),
              (unsigned long long)__double_as_longlong(a.maxd));
}

__global__ void compare_clear(TcamdCompareRecord* rec, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) record_clear(rec + i);
}

// after the atomics of compare_expected (stream order): the elements at each pair's lowest index
__global__ void compare_fetch(CompareParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_pairs) return;
  const uint64_t f = p.rec[i].first_index;
  if (f == kNoIndex) return;
  const int w = kind_width(p.kind[i]);
  p.rec[i].got_bits = load_bits(p.got[i] + f * w, w);
  p.rec[i].expected_bits = load_bits(p.exp[i] + f * w, w);
}

}  // namespace

// The kernel's decomposition, for the tests that sit on its edges: bytes of got
// a lane reads per step, bytes per workgroup, workgroups per pair at most.
extern "C" void tcamd_compare_geometry(uint64_t* out3) {
  out3[0] = kUnit;
  out3[1] = kBlockBytes;
  out3[2] = kMaxBlocksPerPair;
}

// pairs: a host table of n_pairs (0..64) entries of device pointers; records: a
// device pointer to n_pairs TcamdCompareRecord, written in stream order.  A
// pointer that is null (with count > 0) or not aligned to its element, a dtype
// the rule does not know, a count whose bytes do not fit 64 bits, a tolerance
// that is negative or not finite, or more than 64 pairs is hipErrorInvalidValue
// before any launch.
extern "C" int tcamd_compare_expected(const TcamdComparePair* pairs, int n_pairs, double atol, double rtol,
                                      TcamdCompareRecord* records, void* stream) {
  if (n_pairs < 0 || n_pairs > kMaxPairs || !tol_valid(atol, rtol)) return hipErrorInvalidValue;
  if (n_pairs == 0) return hipSuccess;
  if (!pairs || !records) return hipErrorInvalidValue;
  CompareParams p;
  uint32_t blocks = 0;
  bool multi = false;
  for (int i = 0; i < kMaxPairs; ++i) {
    if (i >= n_pairs) {
      p.got[i] = p.exp[i] = nullptr;
      p.count[i] = 0;
      p.kind[i] = kBytes1;
      p.first_block[i + 1] = blocks;
      continue;
    }
    const TcamdComparePair& q = pairs[i];
    const int kind = kind_of(q.dtype);
    if (kind == kBadKind) return hipErrorInvalidValue;
    const uint64_t w = (uint64_t)kind_width(kind);
    if (q.count > (~0ull >> 4) / w) return hipErrorInvalidValue;
    if (q.count && (!q.got || !q.expected)) return hipErrorInvalidValue;
    if (((uintptr_t)q.got | (uintptr_t)q.expected) % w) return hipErrorInvalidValue;
    p.got[i] = static_cast<const uint8_t*>(q.got);
    p.exp[i] = static_cast<const uint8_t*>(q.expected);
    p.count[i] = q.count;
    p.kind[i] = (int8_t)kind;
    uint64_t nb = (q.count * w + kBlockBytes - 1) / kBlockBytes;
    nb = nb < 1 ? 1 : nb > kMaxBlocksPerPair ? kMaxBlocksPerPair : nb;
    multi = multi || nb > 1;
    p.first_block[i] = blocks;
    blocks += (uint32_t)nb;
    p.first_block[i + 1] = blocks;
  }
  p.n_pairs = n_pairs;
  p.atomic = multi ? 1 : 0;
  p.tol = make_tol(atol, rtol);
  p.rec = records;
  hipStream_t s = (hipStream_t)stream;
  if (multi) {
    hipLaunchKernelGGL(compare_clear, dim3(1), dim3(kMaxPairs), 0, s, records, n_pairs);
    int rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  hipLaunchKernelGGL(compare_expected, dim3(blocks), dim3(kBlock), 0, s, p);
  int rc = hipGetLastError();
  if (rc != hipSuccess || !multi) return rc;
  hipLaunchKernelGGL(compare_fetch, dim3(1), dim3(kMaxPairs), 0, s, p);
  return hipGetLastError();
}
