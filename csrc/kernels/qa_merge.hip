// K29 qa_merge — the n best answer spans of a document from the n best of each
// of its doc-stride windows, the second device step of the `qa_doc_spans` model
// (server/gpu_models.py QaDocSpans; csrc/host/qa_merge.cc is the host twin).
// The rule — which rows a document owns, the key, the order, the null score,
// the filler — is kernels/qa_span_math.h, which both compile.
//
// The input is what K27 with a start mask (tcamd_qa_spans_masked) left for the
// rows K28w (tcamd_wordpiece_windows) made: per row kmax ranks of (span, score)
// and a null score, with window_info per row and doc_info per document.  The
// start mask gives each document start to one window, so every row's list is
// already sorted by the merge key, and the document's k best are a k-way merge
// of list heads.
//
// One workgroup of 128 threads (two waves) per document, thread t on window t
// of the document (at most 128).  A thread keeps the key of the head of its
// list in a register.  k rounds: the workgroup maximum of the heads (64-bit
// butterfly shuffles inside a wave as in K27, one LDS slot per wave across the
// two), then the lowest thread that holds it (a ballot per wave, one LDS slot
// per wave), which stores the rank and advances its head.  Equal keys in two
// rows, which the start mask excludes but arbitrary inputs do not, come out
// lowest row first in successive rounds.  LDS is 24 bytes.
//
// Why no thread can miss a barrier.  A workgroup is always 128 threads, two full
// waves.  k comes from k_doc[d] and the document's rows from doc_info[d]: one
// address each for the whole workgroup, and the only early return (k == 0)
// sits before the first barrier.  The round loop runs j < k and its only break
// tests `win`, which every thread computes from the same two LDS words after
// the same barrier.  s_red is written before the first barrier of a round and
// read after it, s_who before and after the second, so a slot is never
// rewritten before every thread has passed the barrier behind its last read.
// Threads past the document's windows carry key 0 and take every barrier.
// Nothing waits on another workgroup; no loop is unbounded.  Every store is a
// vector store; there is no atomic.

#include "kernels/common.h"
#include "kernels/qa_span_math.h"

using namespace tcamd_qa;

namespace {

constexpr int kWave = 64;
constexpr int kThreads = kMergeMaxRows;
constexpr int kWaves = kThreads / kWave;

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

__global__ void __launch_bounds__(kThreads)
qa_merge_docs(const int32_t* __restrict__ spans, const uint32_t* __restrict__ scores,
              const uint32_t* __restrict__ null_score, int rows, const int32_t* __restrict__ window_info,
              const uint32_t* __restrict__ doc_info, const int32_t* __restrict__ k_doc, int kmax,
              int32_t* __restrict__ out_spans, int32_t* __restrict__ out_windows, uint32_t* __restrict__ out_scores,
              uint32_t* __restrict__ out_null) {
  __shared__ uint64_t s_red[kWaves];
  __shared__ uint32_t s_who[kWaves];

  const int t = threadIdx.x;
  const int lane = t & (kWave - 1);
  const int wave = t >> 6;
  const int d = blockIdx.x;
  const int k = __builtin_amdgcn_readfirstlane(clamp_k(k_doc[d], kmax));
  if (k == 0) return;  // the document is skipped: nothing of it is written
  int first;
  const int W = merge_rows(doc_info, d, rows, &first);
  const bool live = t < W;
  const uint64_t r = (uint64_t)(first + (live ? t : 0));
  const int32_t* my_spans = spans + r * (uint64_t)kmax * 2;
  const uint32_t* my_scores = scores + r * (uint64_t)kmax;
  const int32_t* wi = window_info + r * 4;
  int32_t* o_spans = out_spans + (uint64_t)d * (uint64_t)kmax * 2;
  int32_t* o_windows = out_windows + (uint64_t)d * (uint64_t)kmax;
  uint32_t* o_scores = out_scores + (uint64_t)d * (uint64_t)kmax;

  // the head of this window's list, and the lowest null score (the highest inverted image, the lowest row)
  int h = 0;
  uint64_t cur = 0, nk = 0;
  uint32_t nb = kFillerBits;
  if (live) {
    cur = merge_key(my_spans[0], my_spans[1], my_scores[0], wi);
    nb = null_score[r];
    nk = ((uint64_t)~null_image(nb) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)t);
  }
  nk = wave_max_u64(nk);
  if (lane == 0) s_red[wave] = nk;
  __syncthreads();
  nk = s_red[0] > s_red[1] ? s_red[0] : s_red[1];
  __syncthreads();  // s_red is written again below
  if (W == 0) {
    if (t == 0) out_null[d] = kFillerBits;
  } else if (live && (uint32_t)t == 0xFFFFFFFFu - (uint32_t)nk) {
    out_null[d] = (nb & 0x7fffffffu) > 0x7f800000u ? kCanonNan : nb;
  }

  int j = 0;
  for (; j < k; ++j) {
    const uint64_t v = wave_max_u64(cur);
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    const uint64_t win = s_red[0] > s_red[1] ? s_red[0] : s_red[1];
    if (win == 0) break;  // the lists ran out: the same two words for every thread
    const uint64_t held = __ballot(cur == win);
    if (lane == 0) s_who[wave] = held ? (uint32_t)(wave * kWave + __builtin_ctzll(held)) : 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t who = s_who[0] < s_who[1] ? s_who[0] : s_who[1];
    if ((uint32_t)t == who) {
      const uint32_t b = my_scores[h];
      o_spans[2 * j] = my_spans[2 * h];
      o_spans[2 * j + 1] = my_spans[2 * h + 1];
      o_windows[j] = (int32_t)r;
      o_scores[j] = (b & 0x7fffffffu) > 0x7f800000u ? kCanonNan : b;
      ++h;
      cur = h < k ? merge_key(my_spans[2 * h], my_spans[2 * h + 1], my_scores[h], wi) : 0;
    }
  }
  // fewer than k candidates: ranks j .. k - 1 are filler
  if (t >= j && t < k) {
    o_spans[2 * t] = kFillerIndex;
    o_spans[2 * t + 1] = kFillerIndex;
    o_windows[t] = kFillerIndex;
    o_scores[t] = kFillerBits;
  }
}

}  // namespace

// spans / scores / null_score: device [rows][kmax][2], [rows][kmax], [rows], as
// tcamd_qa_spans_masked wrote them with k_row = the document's k; window_info:
// device int32 [rows][4] and doc_info: device uint32 [docs][4], as
// tcamd_wordpiece_windows wrote them; k_doc: device int32 [docs].  Document d
// gets its first min(k_doc[d], kmax) ranks at out_spans[d][:][2] /
// out_windows[d][:] / out_scores[d][:] (documents kmax apart) and out_null[d];
// k_doc[d] < 1 skips the document; nothing else is written.  What
// kernels/qa_span_math.h merge_args_valid refuses is hipErrorInvalidValue before
// any launch; docs == 0 is success without one.
extern "C" int tcamd_qa_merge(const int32_t* spans, const float* scores, const float* null_score, int32_t rows,
                              const int32_t* window_info, const uint32_t* doc_info, int32_t docs, const int32_t* k_doc,
                              int32_t kmax, int32_t* out_spans, int32_t* out_windows, float* out_scores,
                              float* out_null, hipStream_t s) {
  if (!merge_args_valid(spans, scores, null_score, rows, window_info, doc_info, docs, k_doc, kmax, out_spans,
                        out_windows, out_scores, out_null))
    return hipErrorInvalidValue;
  if (docs == 0) return hipSuccess;
  hipLaunchKernelGGL(qa_merge_docs, dim3((unsigned)docs), dim3(kThreads), 0, s, spans,
                     reinterpret_cast<const uint32_t*>(scores), reinterpret_cast<const uint32_t*>(null_score),
                     (int)rows, window_info, doc_info, k_doc, (int)kmax, out_spans, out_windows,
                     reinterpret_cast<uint32_t*>(out_scores), reinterpret_cast<uint32_t*>(out_null));
  return hipGetLastError();
}
