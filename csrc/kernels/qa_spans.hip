// K27 qa_spans — the n best answer spans of every row of a batch of
// question-answering logits, the device half of the `qa_spans` model
// (server/gpu_models.py QaSpans; csrc/host/qa_spans.cc is the host twin).  The
// rule — eligible tokens, candidates, the score, the order, the filler — is
// kernels/qa_span_math.h, which both compile.
//
// One 256-thread workgroup per row.  The row's start and end bits and one
// byte per token (bit 0 eligible, bit 1 may start a span: every eligible token
// without a start mask, those with start_ok >= 1 with one) go into LDS once
// (9 bytes per token, 9.3 KB at S = 1024).  Thread t owns the starts t,
// t + 256, t + 512 and t + 768 and
// keeps the best key of each one's window [s, min(s + L, S)) in four 64-bit
// registers: one pass of about S * L / 256 evaluations per thread.  Then k
// rounds.  A round takes the workgroup maximum of the per-start keys (64-bit
// butterfly shuffles inside a wave as in K19, one LDS slot per wave across the
// four), thread 0 stores the winner, the whole workgroup rescans the winner's
// window alone for that start's best key strictly below the winner, and the
// start's owner takes it.  A start's keys are unique and come out in descending
// order, so "strictly below" needs no exclusion state.  A round costs S / 256
// + L / 256 evaluations per thread and two barriers, never a pass over the
// S * L candidates.
//
// Why no thread can miss a barrier.  A workgroup is always 256 threads, four
// full waves, and every exit and every branch that encloses a barrier or a
// shuffle is taken by all of them or by none:
//   * k and L come from k_row[r] and len_row[r], one address for the whole
//     workgroup; the two early returns (k == 0, L == 0) sit before the first
//     barrier;
//   * the round loop runs j < k, and its only break tests `win`, which every
//     thread computes from the same four LDS words after the same barrier;
//   * the loops between the barriers (the load, the first pass, the rescan)
//     have per-thread bounds and contain no barrier and no shuffle; the start
//     mask is read in the load alone and decides only which starts of the
//     first pass have candidates;
//   * the two reduction arrays alternate: red[0] is written before the first
//     barrier of a round and read after it, red[1] before and after the second,
//     so a slot is never rewritten before every thread has passed the barrier
//     that follows its last read.
// Nothing waits on another workgroup, and no loop is unbounded.

#include "kernels/common.h"
#include "kernels/qa_span_math.h"

using namespace tcamd;
using namespace tcamd_qa;

namespace {

constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kStartsPerThread = kMaxSeq / kBlock;

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

__global__ void __launch_bounds__(kBlock)
qa_spans_rows(const uint8_t* __restrict__ start, const uint8_t* __restrict__ end, uint64_t logit_stride,
              const uint8_t* __restrict__ mask, const uint8_t* __restrict__ ttype, uint64_t ids_stride, int S,
              const uint8_t* __restrict__ start_ok, const int32_t* __restrict__ k_row,
              const int32_t* __restrict__ len_row, int kmax, int32_t* __restrict__ spans,
              uint32_t* __restrict__ scores, uint32_t* __restrict__ null_score) {
  __shared__ uint32_t s_start[kMaxSeq];
  __shared__ uint32_t s_end[kMaxSeq];
  __shared__ uint8_t s_ok[kMaxSeq];
  __shared__ uint64_t s_red[2][kWaves];

  const int t = threadIdx.x;
  const int lane = t & (kWave - 1);
  const int wave = t >> 6;
  const uint64_t r = blockIdx.x;
  const int k = __builtin_amdgcn_readfirstlane(clamp_k(k_row[r], kmax));
  if (k == 0) return;  // the row is skipped: nothing of it is written
  const uint32_t* st = reinterpret_cast<const uint32_t*>(start + r * logit_stride);
  const uint32_t* en = reinterpret_cast<const uint32_t*>(end + r * logit_stride);
  const int32_t* mk = reinterpret_cast<const int32_t*>(mask + r * ids_stride);
  const int32_t* tt = reinterpret_cast<const int32_t*>(ttype + r * ids_stride);
  const int32_t* so = start_ok ? reinterpret_cast<const int32_t*>(start_ok + r * ids_stride) : nullptr;
  int32_t* out_spans = spans + r * (uint64_t)kmax * 2;
  uint32_t* out_scores = scores + r * (uint64_t)kmax;
  if (t == 0) null_score[r] = score_bits(st[0], en[0]);
  const int L = __builtin_amdgcn_readfirstlane(clamp_len(len_row[r], S));
  if (L == 0) {  // no candidate: filler alone
    if (t < k) {
      out_spans[2 * t] = kFillerIndex;
      out_spans[2 * t + 1] = kFillerIndex;
      out_scores[t] = kFillerBits;
    }
    return;
  }
  for (int i = t; i < S; i += kBlock) {
    s_start[i] = st[i];
    s_end[i] = en[i];
    s_ok[i] = token_bits(mk[i], tt[i], so != nullptr, so ? so[i] : 0);
  }
  __syncthreads();

  // the best key of each start this thread owns
  uint64_t mine[kStartsPerThread];
#pragma unroll
  for (int i = 0; i < kStartsPerThread; ++i) {
    const int s = t + i * kBlock;
    uint64_t best = 0;
    if (s < S && (s_ok[s] & kTokStart)) {
      const uint32_t sb = s_start[s];
      const int hi = s + L < S ? s + L : S;
      const uint32_t base = (uint32_t)s * (uint32_t)S;
      for (int e = s; e < hi; ++e) {
        if (!s_ok[e]) continue;
        const uint64_t key = span_key(score_bits(sb, s_end[e]), base + (uint32_t)e);
        best = key > best ? key : best;
      }
    }
    mine[i] = best;
  }

  int j = 0;
  for (; j < k; ++j) {
    uint64_t v = mine[0];
#pragma unroll
    for (int i = 1; i < kStartsPerThread; ++i) v = mine[i] > v ? mine[i] : v;
    v = wave_max_u64(v);
    if (lane == 0) s_red[0][wave] = v;
    __syncthreads();
    uint64_t win = s_red[0][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) win = s_red[0][w] > win ? s_red[0][w] : win;
    if (win == 0) break;  // the candidates ran out: the same four words for every thread
    const uint32_t idx = key_index(win);
    const int ws = (int)(idx / (uint32_t)S);
    const int we = (int)(idx - (uint32_t)ws * (uint32_t)S);
    const uint32_t sb = s_start[ws];
    if (t == 0) {
      out_spans[2 * j] = ws;
      out_spans[2 * j + 1] = we;
      out_scores[j] = score_bits(sb, s_end[we]);
    }
    // the winner's start: its best key strictly below the winner
    const int hi = ws + L < S ? ws + L : S;
    const uint32_t base = (uint32_t)ws * (uint32_t)S;
    uint64_t nb = 0;
    for (int e = ws + t; e < hi; e += kBlock) {
      if (!s_ok[e]) continue;
      const uint64_t key = span_key(score_bits(sb, s_end[e]), base + (uint32_t)e);
      if (key < win && key > nb) nb = key;
    }
    nb = wave_max_u64(nb);
    if (lane == 0) s_red[1][wave] = nb;
    __syncthreads();
    nb = s_red[1][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) nb = s_red[1][w] > nb ? s_red[1][w] : nb;
#pragma unroll
    for (int i = 0; i < kStartsPerThread; ++i)
      if (t + i * kBlock == ws) mine[i] = nb;
  }
  // fewer than k candidates: ranks j .. k - 1 are filler
  if (t >= j && t < k) {
    out_spans[2 * t] = kFillerIndex;
    out_spans[2 * t + 1] = kFillerIndex;
    out_scores[t] = kFillerBits;
  }
}

}  // namespace

// start / end: device fp32 rows, row r at base + r * logit_stride_bytes; mask /
// ttype: device int32 rows, ids_stride_bytes apart; k_row / len_row: device
// [rows], the answers and the longest answer of each row.  Row r gets its first
// min(k_row[r], kmax) ranks at spans[r][:][2] / scores[r][:] (rows kmax apart)
// and null_score[r]; k_row[r] < 1 skips the row; nothing else is written.  What
// kernels/qa_span_math.h args_valid refuses is hipErrorInvalidValue before any
// launch; rows == 0 is success without one.
extern "C" int tcamd_qa_spans(const float* start, const float* end, uint64_t logit_stride_bytes, const int32_t* mask,
                              const int32_t* ttype, uint64_t ids_stride_bytes, int32_t rows, int32_t S,
                              const int32_t* k_row, const int32_t* len_row, int32_t kmax, int32_t* spans,
                              float* scores, float* null_score, hipStream_t s) {
  if (!args_valid(start, end, logit_stride_bytes, mask, ttype, ids_stride_bytes, rows, S, k_row, len_row, kmax, spans,
                  scores, null_score))
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(qa_spans_rows, dim3((unsigned)rows), dim3(kBlock), 0, s, reinterpret_cast<const uint8_t*>(start),
                     reinterpret_cast<const uint8_t*>(end), logit_stride_bytes, reinterpret_cast<const uint8_t*>(mask),
                     reinterpret_cast<const uint8_t*>(ttype), ids_stride_bytes, (int)S,
                     static_cast<const uint8_t*>(nullptr), k_row, len_row, (int)kmax, spans,
                     reinterpret_cast<uint32_t*>(scores), reinterpret_cast<uint32_t*>(null_score));
  return hipGetLastError();
}

// tcamd_qa_spans with a start mask: start_ok, device int32 rows ids_stride_bytes
// apart like mask / ttype; a span may start only where start_ok >= 1.
extern "C" int tcamd_qa_spans_masked(const float* start, const float* end, uint64_t logit_stride_bytes,
                                     const int32_t* mask, const int32_t* ttype, const int32_t* start_ok,
                                     uint64_t ids_stride_bytes, int32_t rows, int32_t S, const int32_t* k_row,
                                     const int32_t* len_row, int32_t kmax, int32_t* spans, float* scores,
                                     float* null_score, hipStream_t s) {
  if (!args_valid(start, end, logit_stride_bytes, mask, ttype, ids_stride_bytes, rows, S, k_row, len_row, kmax, spans,
                  scores, null_score) ||
      !start_ok || ((uintptr_t)start_ok & 3))
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(qa_spans_rows, dim3((unsigned)rows), dim3(kBlock), 0, s, reinterpret_cast<const uint8_t*>(start),
                     reinterpret_cast<const uint8_t*>(end), logit_stride_bytes, reinterpret_cast<const uint8_t*>(mask),
                     reinterpret_cast<const uint8_t*>(ttype), ids_stride_bytes, (int)S,
                     reinterpret_cast<const uint8_t*>(start_ok), k_row, len_row, (int)kmax, spans,
                     reinterpret_cast<uint32_t*>(scores), reinterpret_cast<uint32_t*>(null_score));
  return hipGetLastError();
}
