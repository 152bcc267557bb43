// K28 wordpiece — UTF-8 questions and contexts to BERT question-answering rows
// (input_ids, attention_mask, token_type_ids, byte offsets, overflow, a status
// word), the device half of the `bert_tokenizer` model (server/gpu_models.py
// BertTokenizer; csrc/host/wordpiece.cc is the host twin).  The rule — the fold,
// words, greedy longest-match pieces, offsets, the row, what is invalid — is
// kernels/wordpiece_core.h over the table kernels/wordpiece_table.h, which both
// compile; what a thread does in each phase is a function of that header, and
// this file adds the grids and the workgroup scans.
//
// A call handles up to 128 rows, that is 256 texts (text 2 r the question of row
// r, 2 r + 1 its context), in ten launches on the caller's stream.  A workgroup
// is 256 threads and owns one chunk of 1024 bytes (then: 1024 folded positions)
// of one text; the grid is (chunks of the longest possible text, texts), and a
// workgroup whose chunk lies behind its text's end returns at once.
//   clear     one workgroup per row: the outputs are zero, so a padded or a
//             refused row is all zeros
//   plan      one workgroup: each text's status before a byte is read, and its
//             base in the folded arrays (an exclusive scan of the lengths; a
//             fold never has more code points than its source has bytes)
//   count     a thread decodes and folds its 4 bytes; a sequence belongs to the
//             thread of its first byte, which reads the bytes behind the chunk
//             edge itself; the chunk's count of folded code points, and the
//             text's lowest invalid byte by one atomic minimum per thread that
//             saw one
//   scan      one workgroup per text: chunk counts to chunk bases
//   emit      decode again and write each folded code point and its origin at
//             base + chunk base + the workgroup scan of the threads' counts
//   match     per folded position: word-start bit, rest of the word, and the
//             longest vocabulary piece starting here (first piece at a word
//             start, "##" piece elsewhere) by an incrementally extended hash,
//             every hit confirmed by comparing the code points
//   walk      the thread of a word start follows p -> p + len[p] and marks the
//             piece starts, or the word as one [UNK]; it writes inside its word
//             only, and the word may cross chunk edges, hence a launch of its own
//   pieces    the chunk's count of piece starts;   scan   again, to bases
//   assemble  a piece's rank is its chunk base plus the workgroup scan; the
//             position that starts a piece stores id, mask, type and begin, the
//             position that ends one stores end; one thread per text stores the
//             special tokens, overflow and the status word
// Nothing is computed on the host.
//
// K28w, tcamd_wordpiece_windows, is the same call for contexts longer than a
// row (rule 8 of the header: doc-stride windows).  A row of the table is a
// document; its launches are the ten above over a clear of the call's row
// capacity, with two changes:
//   windows   one workgroup, between the second scan and the assemble: thread d
//             turns t_npiece into document d's W, a workgroup scan of the W that
//             passed max_windows gives the row bases, a second one of the rows
//             that fit gives n_rows; the thread writes doc_info and the
//             window_info of its rows
//   assemble  windowed: the position that starts or ends context piece k finds
//             the windows w_lo .. w_hi that hold k, at most ceil(cap / stride),
//             the best of them by the max-context score in one loop, and stores
//             into each in a second (O(windows) per piece); a question piece
//             goes into every row of its document; one thread per text stores
//             the special tokens of the document's rows
// doc_info is the hand-over between the two: the assemble reads first row, W, P
// and status from the output the windows launch finished, so the workspace does
// not grow (tcamd_wordpiece_windows_workspace is tcamd_wordpiece_workspace).
//
// LDS is four words per workgroup whatever the text length; everything else is
// in the caller's workspace (tcamd_wordpiece_workspace: 16 bytes per text byte
// plus 135 KB).  Every store is a vector store; the only atomic is count's
// atomicMin.
//
// Why no thread can miss a barrier.  The only barriers are the two inside
// block_scan.  A workgroup is always 256 threads, and every return that precedes
// a block_scan tests blockIdx, a per-text word of the workspace that an earlier
// launch finished writing (t_stat, t_err, t_nfold) or the row table: the same
// addresses for all 256 threads, never threadIdx.  count reads t_stat only, not
// t_err, which that launch itself updates.  The per-thread bounds (i < len,
// p < n) guard loads and stores, never a block_scan.  K28w adds two kernels.
// wp_windows is one workgroup that returns nowhere: threads past the documents
// carry zeros through both block_scans, and the per-thread loop over a
// document's windows between them holds no barrier.  wp_assemble_windows returns, ahead of its block_scan, on
// blockIdx, on doc_info[d][3] (the status the windows launch finished, one
// address for the workgroup) and on t_nfold; a document with status 0 is not
// dead, so t_nfold and t_base are what the earlier launches left.  The loops
// over windows are bounded by W <= 128.  No workgroup waits on
// another inside a launch: what one needs from others (chunk bases, match
// lengths of the next chunk, piece marks) it reads after a kernel boundary.
// No loop is unbounded: probes stop after `slots` steps, words after 101.

#include "kernels/common.h"

#define TCAMD_WP_TABLE_ATTR __device__
#include "kernels/wordpiece_core.h"
#include "kernels/wordpiece_table.h"

using namespace tcamd_wp;

namespace {

constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;

__device__ __forceinline__ FoldTable dev_table() { return FoldTable{kWpStages.stage1, kWpStages.stage2, kWpEntries, kWpExt}; }

// Exclusive scan of v over the 256 threads; *total is the sum.  Two barriers,
// the second so that s_w may be used again at once.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, off, kWave);
    if (lane >= off) incl += o;
  }
  if (lane == kWave - 1) s_w[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t x = s_w[w];
    if (w < wave) before += x;
    all += x;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// One workgroup per row: the row's outputs are zero before anything else writes them.
__global__ void __launch_bounds__(kBlock) wp_clear(Ctx c) {
  const uint64_t row = (uint64_t)blockIdx.x * (uint64_t)c.S;
  for (int i = threadIdx.x; i < c.S; i += kBlock) {
    c.ids[row + i] = 0;
    c.mask[row + i] = 0;
    c.type_ids[row + i] = 0;
    c.offsets[2 * (row + i)] = 0;
    c.offsets[2 * (row + i) + 1] = 0;
  }
  if (threadIdx.x == 0) c.overflow[blockIdx.x] = 0;
}

__global__ void __launch_bounds__(kBlock) wp_plan(Ctx c) {
  __shared__ uint32_t s_w[kWaves];
  const int t = threadIdx.x, texts = 2 * c.rows;
  const bool vocab_ok = vocab_header_valid(c.vocab, c.vocab_words);
  const uint32_t want = t < texts ? plan_text(c, t, vocab_ok) : 0u;
  uint32_t total;
  const uint32_t base = block_scan(want, s_w, &total);
  if (t < texts) plan_place(c, t, base, want);
}

__global__ void __launch_bounds__(kBlock) wp_count(Ctx c) {
  __shared__ uint32_t s_w[kWaves];
  const int t = blockIdx.y;
  const uint32_t ch = blockIdx.x;
  if (c.t_stat[t] != kStOk) return;
  const uint32_t len = text_len(c, t);
  if (ch * kChunk >= len) return;
  c.tab = dev_table();
  const uint8_t* tx = c.text + text_off(c, t);
  uint32_t cnt = 0, bad = kNone;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t i = ch * kChunk + threadIdx.x * kPerThread + j;
    if (i >= len) break;
    uint32_t f[3], org;
    bool err;
    cnt += (uint32_t)item_at(c.tab, tx, len, i, f, &org, &err);
    if (err && i < bad) bad = i;
  }
  if (bad != kNone) atomicMin(&c.t_err[t], bad);
  uint32_t total;
  block_scan(cnt, s_w, &total);
  if (threadIdx.x == 0) c.ch_fold[t * kMaxChunks + ch] = total;
}

// pieces == 0: ch_fold over the text's bytes -> t_nfold; 1: ch_piece over its folded positions -> t_npiece
__global__ void __launch_bounds__(kBlock) wp_scan(Ctx c, int pieces) {
  __shared__ uint32_t s_w[kWaves];
  const int t = blockIdx.x;
  if (pieces ? row_dead(c, t >> 1) : c.t_stat[t] != kStOk) return;
  uint32_t* arr = (pieces ? c.ch_piece : c.ch_fold) + t * kMaxChunks;
  const uint32_t nch = chunks_of(pieces ? c.t_nfold[t] : text_len(c, t));
  const uint32_t v = threadIdx.x < nch ? arr[threadIdx.x] : 0u;
  uint32_t total;
  const uint32_t excl = block_scan(v, s_w, &total);
  if (threadIdx.x < nch) arr[threadIdx.x] = excl;
  if (threadIdx.x == 0) (pieces ? c.t_npiece : c.t_nfold)[t] = total;
}

__global__ void __launch_bounds__(kBlock) wp_emit(Ctx c) {
  __shared__ uint32_t s_w[kWaves];
  const int t = blockIdx.y;
  const uint32_t ch = blockIdx.x;
  if (row_dead(c, t >> 1)) return;
  const uint32_t len = text_len(c, t);
  if (ch * kChunk >= len) return;
  c.tab = dev_table();
  const uint8_t* tx = c.text + text_off(c, t);
  uint32_t f[kPerThread][3], org[kPerThread];
  int n[kPerThread];
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t i = ch * kChunk + threadIdx.x * kPerThread + j;
    n[j] = 0;
    org[j] = 0;
    if (i < len) {
      bool err;
      n[j] = item_at(c.tab, tx, len, i, f[j], &org[j], &err);
    }
    cnt += (uint32_t)n[j];
  }
  uint32_t total;
  uint32_t at = c.t_base[t] + c.ch_fold[t * kMaxChunks + ch] + block_scan(cnt, s_w, &total);
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    for (int k = 0; k < n[j]; ++k, ++at) {
      c.cp[at] = f[j][k];
      c.org[at] = org[j];
    }
}

__global__ void __launch_bounds__(kBlock) wp_match(Ctx c) {
  const int t = blockIdx.y;
  if (row_dead(c, t >> 1)) return;
  const uint32_t n = c.t_nfold[t], base = c.t_base[t];
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t p = blockIdx.x * kChunk + j * kBlock + threadIdx.x;
    if (p < n) match_item(c, base, n, p);
  }
}

__global__ void __launch_bounds__(kBlock) wp_walk(Ctx c) {
  const int t = blockIdx.y;
  if (row_dead(c, t >> 1)) return;
  const uint32_t n = c.t_nfold[t], base = c.t_base[t];
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t p = blockIdx.x * kChunk + j * kBlock + threadIdx.x;
    if (p < n) walk_item(c, base, p);
  }
}

__global__ void __launch_bounds__(kBlock) wp_pieces(Ctx c) {
  __shared__ uint32_t s_w[kWaves];
  const int t = blockIdx.y;
  const uint32_t ch = blockIdx.x;
  if (row_dead(c, t >> 1)) return;
  const uint32_t n = c.t_nfold[t], base = c.t_base[t];
  if (ch * kChunk >= n) return;
  uint32_t cnt = 0;
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t p = ch * kChunk + j * kBlock + threadIdx.x;
    if (p < n) cnt += piece_at(c, base, p);
  }
  uint32_t total;
  block_scan(cnt, s_w, &total);
  if (threadIdx.x == 0) c.ch_piece[t * kMaxChunks + ch] = total;
}

__global__ void __launch_bounds__(kBlock) wp_assemble(Ctx c) {
  __shared__ uint32_t s_w[kWaves];
  const int t = blockIdx.y;
  const uint32_t ch = blockIdx.x;
  if (ch == 0 && threadIdx.x == 0) assemble_text(c, t);
  if (row_dead(c, t >> 1)) return;
  const uint32_t n = c.t_nfold[t], base = c.t_base[t];
  if (ch * kChunk >= n) return;
  const uint32_t p0 = ch * kChunk + threadIdx.x * kPerThread;
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (p0 + j < n) cnt += piece_at(c, base, p0 + j);
  uint32_t total;
  uint32_t incl = c.ch_piece[t * kMaxChunks + ch] + block_scan(cnt, s_w, &total);
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (p0 + j < n) {
      incl += piece_at(c, base, p0 + j);
      assemble_item(c, t, base, n, p0 + j, incl);
    }
}

// ---- K28w -------------------------------------------------------------------------
// One workgroup per row of the call's capacity: zero before anything else writes.
__global__ void __launch_bounds__(kBlock) wp_clear_windows(Ctx c) {
  const uint64_t row = (uint64_t)blockIdx.x * (uint64_t)c.S;
  for (int i = threadIdx.x; i < c.S; i += kBlock) {
    c.ids[row + i] = 0;
    c.mask[row + i] = 0;
    c.type_ids[row + i] = 0;
    c.start_mask[row + i] = 0;
    c.offsets[2 * (row + i)] = 0;
    c.offsets[2 * (row + i) + 1] = 0;
  }
  if (threadIdx.x < 4) c.window_info[4 * blockIdx.x + threadIdx.x] = 0;
}

__global__ void __launch_bounds__(kBlock) wp_windows(Ctx c) {
  __shared__ uint32_t s_w[kWaves];
  const int d = threadIdx.x;
  uint32_t st = kStOk, P = 0, W = 0, total;
  const uint32_t want = d < c.rows ? windows_doc(c, d, &st, &P, &W) : 0u;
  const uint32_t base = block_scan(want, s_w, &total);
  const uint32_t got = d < c.rows ? windows_place(c, d, st, P, W, base) : 0u;
  block_scan(got, s_w, &total);
  if (d == 0) c.n_rows[0] = (int32_t)total;
}

__global__ void __launch_bounds__(kBlock) wp_assemble_windows(Ctx c) {
  __shared__ uint32_t s_w[kWaves];
  const int t = blockIdx.y;
  const uint32_t ch = blockIdx.x;
  if (c.doc_info[4 * (t >> 1) + 3] != kStOk) return;
  if (ch == 0 && threadIdx.x == 0) windows_text(c, t);
  const uint32_t n = c.t_nfold[t], base = c.t_base[t];
  if (ch * kChunk >= n) return;
  const uint32_t p0 = ch * kChunk + threadIdx.x * kPerThread;
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (p0 + j < n) cnt += piece_at(c, base, p0 + j);
  uint32_t total;
  uint32_t incl = c.ch_piece[t * kMaxChunks + ch] + block_scan(cnt, s_w, &total);
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (p0 + j < n) {
      incl += piece_at(c, base, p0 + j);
      windows_item(c, t, base, n, p0 + j, incl);
    }
}

}  // namespace

extern "C" uint64_t tcamd_wordpiece_workspace(int32_t rows, uint64_t text_bytes) {
  return workspace_bytes(rows, text_bytes);
}

// {chunk bytes, block threads, longest text, longest word, most rows, chunks per text}
extern "C" void tcamd_wordpiece_geometry(int32_t* g) {
  g[0] = kChunk, g[1] = kBlock, g[2] = (int32_t)kMaxTextBytes, g[3] = kMaxWordChars, g[4] = kMaxRows, g[5] = kMaxChunks;
}

// text: device bytes holding every text of the call; row_table: device uint32
// [rows][4] = {question_off, question_len, context_off, context_len} into it;
// maxq_row: device int32 [rows]; vocab: the device copy of the vocabulary image
// (vocab_words 32-bit words); ws: device workspace of at least
// tcamd_wordpiece_workspace(rows, sum of the text lengths) bytes.  Row r gets
// ids / mask / type_ids [S], offsets [S][2], overflow and status (rows are S
// apart).  What kernels/wordpiece_core.h args_valid refuses, or a workspace
// below the fixed part, is hipErrorInvalidValue before any launch; rows == 0 is
// success without one.  A text that is too long, out of the buffer or past the
// workspace, a max_query_length outside 1 .. S - 3 and an image with a broken
// header are refused per row, in status.
extern "C" int tcamd_wordpiece_tokenize(const uint8_t* text, uint64_t text_bytes, const uint32_t* row_table,
                                        const int32_t* maxq_row, int32_t rows, int32_t S, const uint32_t* vocab,
                                        uint64_t vocab_words, void* ws, uint64_t ws_bytes, int32_t* ids, int32_t* mask,
                                        int32_t* type_ids, int32_t* offsets, int32_t* overflow, uint32_t* status,
                                        hipStream_t s) {
  if (!args_valid(text, row_table, maxq_row, rows, S, vocab, vocab_words, ws, ids, mask, type_ids, offsets, overflow,
                  status))
    return hipErrorInvalidValue;
  Ctx c{};
  if (!ctx_place(&c, ws, ws_bytes)) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  c.text = text, c.text_bytes = text_bytes, c.row_table = row_table, c.maxq_row = maxq_row, c.rows = rows, c.S = S;
  c.vocab = vocab, c.vocab_words = vocab_words;
  c.ids = ids, c.mask = mask, c.type_ids = type_ids, c.offsets = offsets, c.overflow = overflow, c.status = status;
  const uint64_t longest = text_bytes < kMaxTextBytes ? text_bytes : kMaxTextBytes;
  const unsigned chunks = longest ? (unsigned)chunks_of((uint32_t)longest) : 1u;
  const dim3 grid(chunks, 2u * (unsigned)rows), one(2u * (unsigned)rows), block(kBlock);
  hipLaunchKernelGGL(wp_clear, dim3((unsigned)rows), block, 0, s, c);
  hipLaunchKernelGGL(wp_plan, dim3(1), block, 0, s, c);
  hipLaunchKernelGGL(wp_count, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_scan, one, block, 0, s, c, 0);
  hipLaunchKernelGGL(wp_emit, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_match, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_walk, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_pieces, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_scan, one, block, 0, s, c, 1);
  hipLaunchKernelGGL(wp_assemble, grid, block, 0, s, c);
  return hipGetLastError();
}

extern "C" uint64_t tcamd_wordpiece_windows_workspace(int32_t docs, uint64_t text_bytes) {
  return workspace_bytes(docs, text_bytes);
}

// K28w.  The inputs of tcamd_wordpiece_tokenize, a row of the table being a
// document, and per document doc_stride (stride_row, 1 .. S - 3) and
// max_windows (maxw_row, 1 .. 128), device int32 [docs]; out_rows <= 128 is the
// row capacity of the outputs.  ids / mask / type_ids / start_mask
// [out_rows][S], offsets [out_rows][S][2], window_info [out_rows][4], doc_info
// [docs][4] and n_rows [1] are as rule 8 of kernels/wordpiece_core.h has them;
// rows from n_rows on are zero.  Refusals as tcamd_wordpiece_tokenize, and
// out_rows outside 1 .. 128; docs == 0 is success without a launch.
extern "C" int tcamd_wordpiece_windows(const uint8_t* text, uint64_t text_bytes, const uint32_t* row_table,
                                       const int32_t* maxq_row, const int32_t* stride_row, const int32_t* maxw_row,
                                       int32_t docs, int32_t S, const uint32_t* vocab, uint64_t vocab_words, void* ws,
                                       uint64_t ws_bytes, int32_t out_rows, int32_t* ids, int32_t* mask,
                                       int32_t* type_ids, int32_t* start_mask, int32_t* offsets, int32_t* window_info,
                                       uint32_t* doc_info, int32_t* n_rows, hipStream_t s) {
  if (!args_valid(text, row_table, maxq_row, docs, S, vocab, vocab_words, ws, ids, mask, type_ids, offsets, n_rows,
                  doc_info) ||
      !window_args_valid(stride_row, maxw_row, out_rows, start_mask, window_info, doc_info, n_rows))
    return hipErrorInvalidValue;
  Ctx c{};
  if (!ctx_place(&c, ws, ws_bytes)) return hipErrorInvalidValue;
  if (docs == 0) return hipSuccess;
  c.text = text, c.text_bytes = text_bytes, c.row_table = row_table, c.maxq_row = maxq_row, c.rows = docs, c.S = S;
  c.vocab = vocab, c.vocab_words = vocab_words;
  c.ids = ids, c.mask = mask, c.type_ids = type_ids, c.offsets = offsets;
  c.stride_row = stride_row, c.maxw_row = maxw_row, c.out_rows = out_rows;
  c.start_mask = start_mask, c.window_info = window_info, c.doc_info = doc_info, c.n_rows = n_rows;
  const uint64_t longest = text_bytes < kMaxTextBytes ? text_bytes : kMaxTextBytes;
  const unsigned chunks = longest ? (unsigned)chunks_of((uint32_t)longest) : 1u;
  const dim3 grid(chunks, 2u * (unsigned)docs), one(2u * (unsigned)docs), block(kBlock);
  hipLaunchKernelGGL(wp_clear_windows, dim3((unsigned)out_rows), block, 0, s, c);
  hipLaunchKernelGGL(wp_plan, dim3(1), block, 0, s, c);
  hipLaunchKernelGGL(wp_count, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_scan, one, block, 0, s, c, 0);
  hipLaunchKernelGGL(wp_emit, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_match, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_walk, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_pieces, grid, block, 0, s, c);
  hipLaunchKernelGGL(wp_scan, one, block, 0, s, c, 1);
  hipLaunchKernelGGL(wp_windows, dim3(1), block, 0, s, c);
  hipLaunchKernelGGL(wp_assemble_windows, grid, block, 0, s, c);
  return hipGetLastError();
}
