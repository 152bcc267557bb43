// The host twin of K28 wordpiece (csrc/kernels/wordpiece.hip): the same
// arguments on host pointers, the same ids, offsets, overflow and status words,
// by the rule both compile from kernels/wordpiece_core.h over the table in
// kernels/wordpiece_table.h.  tcamd_host_wordpiece_tokenize walks each text
// front to back, word by word, as a tokenizer is usually written;
// tcamd_host_wordpiece_emulate runs the kernel's own phases (plan, count, emit,
// match, walk, pieces, assemble) in the kernel's workspace layout with loops
// where the kernel has workgroups, so the phase code is tested without a GPU.
// tcamd_host_wordpiece_windows and tcamd_host_wordpiece_windows_emulate are the
// same pair for K28w (rule 8, doc-stride windows): the walk lays windows out one
// after the other and asks run_squad's question "is this the max-context window
// of this piece" of every window, where the kernel computes the range in closed
// form.
#include <string.h>

#include <vector>

#include "../kernels/wordpiece_core.h"
#include "../kernels/wordpiece_table.h"

namespace {

using namespace tcamd_wp;

const FoldTable kTable = {kWpStages.stage1, kWpStages.stage2, kWpEntries, kWpExt};

struct Piece {
  uint32_t id, begin, end;
};

// One text front to back.  False where it is invalid (*err = the byte).
bool tokenize_text(const uint32_t* vocab, const uint8_t* t, uint32_t len, std::vector<Piece>* out, uint32_t* err) {
  std::vector<uint32_t> cp, org;
  for (uint32_t i = 0; i < len;) {
    uint32_t c = 0, sl = 0, f[3];
    if (decode_at(t, len, i, &c, &sl) != 1) {
      *err = i;
      return false;
    }
    const int n = fold_cp(kTable, c, f);
    for (int k = 0; k < n; ++k) {
      cp.push_back(f[k]);
      org.push_back(org_pack(i, sl));
    }
    i += sl;
  }
  const uint32_t n = (uint32_t)cp.size(), unk = vocab[8];
  uint32_t longest = vocab[11] < (uint32_t)kMaxWordChars ? vocab[11] : (uint32_t)kMaxWordChars;
  uint32_t hashes[kMaxWordChars + 1];
  for (uint32_t ws = 0; ws < n;) {
    if (cp[ws] & kSpace) {
      ++ws;
      continue;
    }
    uint32_t we = ws + 1;
    if (!(cp[ws] & kIso))
      while (we < n && !(cp[we] & (kSpace | kIso))) ++we;
    const size_t mark = out->size();
    bool ok = we - ws <= (uint32_t)kMaxWordChars;
    for (uint32_t p = ws; ok && p < we;) {
      const uint32_t lim = we - p < longest ? we - p : longest;
      uint32_t h = p == ws ? kHashFirst : kHashCont;
      for (uint32_t k = 1; k <= lim; ++k) hashes[k] = h = hash_step(h, cp[p + k - 1] & kCpMask);
      uint32_t k = lim;
      int32_t id = -1;
      for (; k >= 1; --k)
        if ((id = vocab_find(vocab, cp.data() + p, k, p != ws, hashes[k])) >= 0) break;
      if (id < 0) {
        ok = false;
        break;
      }
      out->push_back({(uint32_t)id, org_begin(org[p]), org_end(org[p + k - 1])});
      p += k;
    }
    if (!ok) {
      out->resize(mark);
      out->push_back({unk, org_begin(org[ws]), org_end(org[we - 1])});
    }
    ws = we;
  }
  return true;
}

void zero_outputs(int32_t rows, int32_t S, int32_t* ids, int32_t* mask, int32_t* type_ids, int32_t* offsets,
                  int32_t* overflow, uint32_t* status) {
  const size_t n = (size_t)rows * (size_t)S;
  memset(ids, 0, n * 4), memset(mask, 0, n * 4), memset(type_ids, 0, n * 4), memset(offsets, 0, n * 8);
  memset(overflow, 0, (size_t)rows * 4), memset(status, 0, (size_t)rows * 4);
}

// plan to the second scan, as the kernel's launches, on a placed Ctx
void run_phases(const Ctx& c) {
  const uint8_t* text = c.text;
  const uint32_t* vocab = c.vocab;
  const uint64_t vocab_words = c.vocab_words;
  const int texts = 2 * c.rows;
  // plan
  const bool vocab_ok = vocab_header_valid(vocab, vocab_words);
  uint32_t base = 0;
  for (int t = 0; t < texts; ++t) {
    const uint32_t want = plan_text(c, t, vocab_ok);
    plan_place(c, t, base, want);
    base += want;  // an exclusive scan of what the texts ask for, as the kernel's
  }
  // count, scan
  for (int t = 0; t < texts; ++t) {
    if (c.t_stat[t] != kStOk) continue;
    const uint8_t* tx = text + text_off(c, t);
    const uint32_t len = text_len(c, t);
    uint32_t total = 0;
    for (uint32_t ch = 0; ch < chunks_of(len); ++ch) {
      uint32_t cnt = 0;
      for (uint32_t i = ch * kChunk; i < len && i < (ch + 1) * kChunk; ++i) {
        uint32_t f[3], org;
        bool err;
        cnt += (uint32_t)item_at(c.tab, tx, len, i, f, &org, &err);
        if (err && i < c.t_err[t]) c.t_err[t] = i;
      }
      c.ch_fold[t * kMaxChunks + ch] = total;
      total += cnt;
    }
    c.t_nfold[t] = total;
  }
  // emit
  for (int t = 0; t < texts; ++t) {
    if (row_dead(c, t >> 1)) continue;
    const uint8_t* tx = text + text_off(c, t);
    const uint32_t len = text_len(c, t);
    for (uint32_t ch = 0; ch < chunks_of(len); ++ch) {
      uint32_t at = c.t_base[t] + c.ch_fold[t * kMaxChunks + ch];
      for (uint32_t i = ch * kChunk; i < len && i < (ch + 1) * kChunk; ++i) {
        uint32_t f[3], org;
        bool err;
        const int n = item_at(c.tab, tx, len, i, f, &org, &err);
        for (int k = 0; k < n; ++k, ++at) c.cp[at] = f[k], c.org[at] = org;
      }
    }
  }
  // match, walk, pieces, scan
  for (int t = 0; t < texts; ++t)
    if (!row_dead(c, t >> 1))
      for (uint32_t p = 0; p < c.t_nfold[t]; ++p) match_item(c, c.t_base[t], c.t_nfold[t], p);
  for (int t = 0; t < texts; ++t)
    if (!row_dead(c, t >> 1))
      for (uint32_t p = 0; p < c.t_nfold[t]; ++p) walk_item(c, c.t_base[t], p);
  for (int t = 0; t < texts; ++t) {
    if (row_dead(c, t >> 1)) continue;
    uint32_t total = 0;
    for (uint32_t ch = 0; ch < chunks_of(c.t_nfold[t]); ++ch) {
      c.ch_piece[t * kMaxChunks + ch] = total;
      for (uint32_t p = ch * kChunk; p < c.t_nfold[t] && p < (ch + 1) * kChunk; ++p) total += piece_at(c, c.t_base[t], p);
    }
    c.t_npiece[t] = total;
  }
}

void zero_window_outputs(int32_t out_rows, int32_t S, int32_t* ids, int32_t* mask, int32_t* type_ids,
                         int32_t* start_mask, int32_t* offsets, int32_t* window_info) {
  const size_t n = (size_t)out_rows * (size_t)S;
  memset(ids, 0, n * 4), memset(mask, 0, n * 4), memset(type_ids, 0, n * 4), memset(start_mask, 0, n * 4);
  memset(offsets, 0, n * 8), memset(window_info, 0, (size_t)out_rows * 16);
}

}  // namespace

extern "C" {

uint64_t tcamd_host_wordpiece_workspace(int32_t rows, uint64_t text_bytes) { return workspace_bytes(rows, text_bytes); }

// {chunk bytes, block threads, longest text, longest word, most rows, chunks per text}
void tcamd_host_wordpiece_geometry(int32_t* g) {
  g[0] = kChunk, g[1] = kBlock, g[2] = (int32_t)kMaxTextBytes, g[3] = kMaxWordChars, g[4] = kMaxRows, g[5] = kMaxChunks;
}

// What a code point folds to: the count, out[3] with kIso (bit 30) or kSpace (bit 31).
int tcamd_host_wordpiece_fold(uint32_t cp, uint32_t* out) { return cp > 0x10FFFF ? -1 : fold_cp(kTable, cp, out); }

// 1 when the image's header is one the tokenizers accept.
int tcamd_host_wordpiece_vocab_check(const uint32_t* vocab, uint64_t vocab_words) {
  return vocab && vocab_header_valid(vocab, vocab_words) ? 1 : 0;
}

// Returns 0, or 1 (the value of hipErrorInvalidValue) for what the device entry
// refuses too; then nothing is written.  No workspace: the arguments are the
// device entry's without ws / ws_bytes / stream.
int tcamd_host_wordpiece_tokenize(const uint8_t* text, uint64_t text_bytes, const uint32_t* row_table,
                                  const int32_t* maxq_row, int32_t rows, int32_t S, const uint32_t* vocab,
                                  uint64_t vocab_words, int32_t* ids, int32_t* mask, int32_t* type_ids,
                                  int32_t* offsets, int32_t* overflow, uint32_t* status) {
  if (!args_valid(text, row_table, maxq_row, rows, S, vocab, vocab_words, status, ids, mask, type_ids, offsets, overflow,
                  status))
    return 1;
  zero_outputs(rows, S, ids, mask, type_ids, offsets, overflow, status);
  const bool vocab_ok = vocab_header_valid(vocab, vocab_words);
  std::vector<Piece> pieces[2];
  for (int32_t r = 0; r < rows; ++r) {
    const int32_t mq = maxq_row[r];
    uint32_t st = kStOk;
    for (int f = 0; f < 2 && st == kStOk; ++f) {
      const uint32_t off = row_table[4 * r + 2 * f], len = row_table[4 * r + 2 * f + 1];
      if (!vocab_ok) st = kStVocab | ((uint32_t)f << 8);
      else if (mq < 1 || mq > S - 3) st = kStParam | ((uint32_t)f << 8);
      else if (len > kMaxTextBytes) st = kStTooLong | ((uint32_t)f << 8);
      else if ((uint64_t)off + len > text_bytes) st = kStRange | ((uint32_t)f << 8);
    }
    for (int f = 0; f < 2 && st == kStOk; ++f) {
      pieces[f].clear();
      uint32_t err = 0;
      if (!tokenize_text(vocab, text + row_table[4 * r + 2 * f], row_table[4 * r + 2 * f + 1], &pieces[f], &err))
        st = kStInvalid | ((uint32_t)f << 8) | (err << 12);
    }
    status[r] = st;
    if (st != kStOk) continue;
    const size_t row = (size_t)r * (size_t)S;
    const uint32_t qn = pieces[0].size() < (size_t)mq ? (uint32_t)pieces[0].size() : (uint32_t)mq;
    const uint32_t room = (uint32_t)S - 3 - qn;
    const uint32_t cn = pieces[1].size() < room ? (uint32_t)pieces[1].size() : room;
    size_t at = row;
    ids[at++] = (int32_t)vocab[9];
    for (uint32_t k = 0; k < qn; ++k) ids[at++] = (int32_t)pieces[0][k].id;
    ids[at++] = (int32_t)vocab[10];
    for (uint32_t k = 0; k < cn; ++k, ++at) {
      ids[at] = (int32_t)pieces[1][k].id;
      type_ids[at] = 1;
      offsets[2 * at] = (int32_t)pieces[1][k].begin;
      offsets[2 * at + 1] = (int32_t)pieces[1][k].end;
    }
    ids[at++] = (int32_t)vocab[10];
    for (size_t k = row; k < at; ++k) mask[k] = 1;
    overflow[r] = (int32_t)(pieces[1].size() - cn);
  }
  return 0;
}

// The device entry's arguments on host pointers (no stream), run phase by phase
// as the kernel does.  Returns 0, or 1 for what the device entry refuses.
int tcamd_host_wordpiece_emulate(const uint8_t* text, uint64_t text_bytes, const uint32_t* row_table,
                                 const int32_t* maxq_row, int32_t rows, int32_t S, const uint32_t* vocab,
                                 uint64_t vocab_words, void* ws, uint64_t ws_bytes, int32_t* ids, int32_t* mask,
                                 int32_t* type_ids, int32_t* offsets, int32_t* overflow, uint32_t* status) {
  if (!args_valid(text, row_table, maxq_row, rows, S, vocab, vocab_words, ws, ids, mask, type_ids, offsets, overflow,
                  status))
    return 1;
  Ctx c{};
  if (!ctx_place(&c, ws, ws_bytes)) return 1;
  c.text = text, c.text_bytes = text_bytes, c.row_table = row_table, c.maxq_row = maxq_row, c.rows = rows, c.S = S;
  c.vocab = vocab, c.vocab_words = vocab_words, c.tab = kTable;
  c.ids = ids, c.mask = mask, c.type_ids = type_ids, c.offsets = offsets, c.overflow = overflow, c.status = status;
  zero_outputs(rows, S, ids, mask, type_ids, offsets, overflow, status);
  const int texts = 2 * rows;
  run_phases(c);
  // assemble
  for (int t = 0; t < texts; ++t) {
    assemble_text(c, t);
    if (row_dead(c, t >> 1)) continue;
    for (uint32_t ch = 0; ch < chunks_of(c.t_nfold[t]); ++ch) {
      uint32_t incl = c.ch_piece[t * kMaxChunks + ch];
      for (uint32_t p = ch * kChunk; p < c.t_nfold[t] && p < (ch + 1) * kChunk; ++p) {
        incl += piece_at(c, c.t_base[t], p);
        assemble_item(c, t, c.t_base[t], c.t_nfold[t], p, incl);
      }
    }
  }
  return 0;
}

uint64_t tcamd_host_wordpiece_windows_workspace(int32_t docs, uint64_t text_bytes) {
  return workspace_bytes(docs, text_bytes);
}

// K28w's arguments on host pointers without ws / ws_bytes / stream.  Returns 0,
// or 1 for what the device entry refuses; then nothing is written.
int tcamd_host_wordpiece_windows(const uint8_t* text, uint64_t text_bytes, const uint32_t* row_table,
                                 const int32_t* maxq_row, const int32_t* stride_row, const int32_t* maxw_row,
                                 int32_t docs, int32_t S, const uint32_t* vocab, uint64_t vocab_words, int32_t out_rows,
                                 int32_t* ids, int32_t* mask, int32_t* type_ids, int32_t* start_mask, int32_t* offsets,
                                 int32_t* window_info, uint32_t* doc_info, int32_t* n_rows) {
  if (!args_valid(text, row_table, maxq_row, docs, S, vocab, vocab_words, n_rows, ids, mask, type_ids, offsets, n_rows,
                  doc_info) ||
      !window_args_valid(stride_row, maxw_row, out_rows, start_mask, window_info, doc_info, n_rows))
    return 1;
  if (docs == 0) return 0;
  zero_window_outputs(out_rows, S, ids, mask, type_ids, start_mask, offsets, window_info);
  const bool vocab_ok = vocab_header_valid(vocab, vocab_words);
  std::vector<Piece> pieces[2];
  struct Win {
    uint32_t start, len;
  };
  std::vector<Win> wins;
  uint32_t next = 0;     // rows asked for by the documents that passed max_windows
  bool full = false;     // a document did not fit: no later one does
  uint32_t used = 0;
  for (int32_t d = 0; d < docs; ++d) {
    uint32_t* di = doc_info + 4 * d;
    di[0] = di[1] = di[2] = 0;
    const int32_t mq = maxq_row[d];
    uint32_t st = kStOk;
    for (int f = 0; f < 2 && st == kStOk; ++f) {
      const uint32_t off = row_table[4 * d + 2 * f], len = row_table[4 * d + 2 * f + 1];
      if (!vocab_ok) st = kStVocab | ((uint32_t)f << 8);
      else if (mq < 1 || mq > S - 3) st = kStParam | ((uint32_t)f << 8);
      else if (len > kMaxTextBytes) st = kStTooLong | ((uint32_t)f << 8);
      else if ((uint64_t)off + len > text_bytes) st = kStRange | ((uint32_t)f << 8);
    }
    for (int f = 0; f < 2 && st == kStOk; ++f) {
      pieces[f].clear();
      uint32_t err = 0;
      if (!tokenize_text(vocab, text + row_table[4 * d + 2 * f], row_table[4 * d + 2 * f + 1], &pieces[f], &err))
        st = kStInvalid | ((uint32_t)f << 8) | (err << 12);
    }
    if (st == kStOk && (stride_row[d] < 1 || stride_row[d] > S - 3 || maxw_row[d] < 1 || maxw_row[d] > kMaxWindows))
      st = kStParam | (2u << 8);
    di[3] = st;
    if (st != kStOk) continue;
    const uint32_t qn = pieces[0].size() < (size_t)mq ? (uint32_t)pieces[0].size() : (uint32_t)mq;
    const uint32_t cap = (uint32_t)S - 3 - qn, P = (uint32_t)pieces[1].size();
    const uint32_t stride = (uint32_t)stride_row[d] < cap ? (uint32_t)stride_row[d] : cap;
    // the windows, one after the other, as run_squad lays them out (but one for P == 0)
    wins.clear();
    uint32_t W = 0;
    if (cap == 0 && P > 0) {
      W = kWindowsNever;
    } else {
      for (uint32_t start = 0;; start += stride) {
        const uint32_t len = P - start < cap ? P - start : cap;
        if (wins.size() <= (size_t)kMaxWindows) wins.push_back({start, len});
        ++W;
        if (start + len >= P) break;
      }
    }
    di[1] = W, di[2] = P;
    if (W > (uint32_t)maxw_row[d]) {
      di[3] = kStWindows;
      continue;
    }
    const uint32_t base = next;
    next += W;
    if (full || base + W > (uint32_t)out_rows) {
      full = true;
      di[3] = kStWindows;
      continue;
    }
    di[0] = base;
    used = base + W;
    for (uint32_t w = 0; w < W; ++w) {
      const size_t r = base + w, row = r * (size_t)S;
      int32_t* wi = window_info + 4 * r;
      wi[0] = d, wi[1] = (int32_t)wins[w].start, wi[2] = (int32_t)wins[w].len, wi[3] = (int32_t)(2 + qn);
      size_t at = row;
      ids[at++] = (int32_t)vocab[9];
      for (uint32_t k = 0; k < qn; ++k) ids[at++] = (int32_t)pieces[0][k].id;
      ids[at++] = (int32_t)vocab[10];
      for (uint32_t j = 0; j < wins[w].len; ++j, ++at) {
        const uint32_t k = wins[w].start + j;
        ids[at] = (int32_t)pieces[1][k].id;
        type_ids[at] = 1;
        offsets[2 * at] = (int32_t)pieces[1][k].begin;
        offsets[2 * at + 1] = (int32_t)pieces[1][k].end;
        // _check_is_max_context: no window scores higher, and none before w as high
        uint32_t best = 0, best_score = 0;
        bool any = false;
        for (uint32_t v = 0; v < W; ++v) {
          if (k < wins[v].start || k >= wins[v].start + wins[v].len) continue;
          const uint32_t l = k - wins[v].start, rr = wins[v].start + wins[v].len - 1 - k;
          const uint32_t sc = 100u * (l < rr ? l : rr) + wins[v].len;
          if (!any || sc > best_score) best = v, best_score = sc, any = true;
        }
        start_mask[at] = best == w ? 1 : 0;
      }
      ids[at++] = (int32_t)vocab[10];
      for (size_t k = row; k < at; ++k) mask[k] = 1;
    }
  }
  n_rows[0] = (int32_t)used;
  return 0;
}

// K28w's arguments on host pointers (no stream), run phase by phase as the
// kernel does.  Returns 0, or 1 for what the device entry refuses.
int tcamd_host_wordpiece_windows_emulate(const uint8_t* text, uint64_t text_bytes, const uint32_t* row_table,
                                         const int32_t* maxq_row, const int32_t* stride_row, const int32_t* maxw_row,
                                         int32_t docs, int32_t S, const uint32_t* vocab, uint64_t vocab_words, void* ws,
                                         uint64_t ws_bytes, int32_t out_rows, int32_t* ids, int32_t* mask,
                                         int32_t* type_ids, int32_t* start_mask, int32_t* offsets, int32_t* window_info,
                                         uint32_t* doc_info, int32_t* n_rows) {
  if (!args_valid(text, row_table, maxq_row, docs, S, vocab, vocab_words, ws, ids, mask, type_ids, offsets, n_rows,
                  doc_info) ||
      !window_args_valid(stride_row, maxw_row, out_rows, start_mask, window_info, doc_info, n_rows))
    return 1;
  Ctx c{};
  if (!ctx_place(&c, ws, ws_bytes)) return 1;
  if (docs == 0) return 0;
  c.text = text, c.text_bytes = text_bytes, c.row_table = row_table, c.maxq_row = maxq_row, c.rows = docs, c.S = S;
  c.vocab = vocab, c.vocab_words = vocab_words, c.tab = kTable;
  c.ids = ids, c.mask = mask, c.type_ids = type_ids, c.offsets = offsets;
  c.stride_row = stride_row, c.maxw_row = maxw_row, c.out_rows = out_rows;
  c.start_mask = start_mask, c.window_info = window_info, c.doc_info = doc_info, c.n_rows = n_rows;
  zero_window_outputs(out_rows, S, ids, mask, type_ids, start_mask, offsets, window_info);
  const int texts = 2 * docs;
  run_phases(c);
  // windows: two exclusive scans, as the kernel's
  std::vector<uint32_t> st(docs), P(docs), W(docs), want(docs);
  for (int d = 0; d < docs; ++d) want[d] = windows_doc(c, d, &st[d], &P[d], &W[d]);
  uint32_t base = 0, total = 0;
  for (int d = 0; d < docs; ++d) {
    total += windows_place(c, d, st[d], P[d], W[d], base);
    base += want[d];
  }
  n_rows[0] = (int32_t)total;
  // windowed assemble
  for (int t = 0; t < texts; ++t) {
    if (doc_info[4 * (t >> 1) + 3] != kStOk) continue;
    windows_text(c, t);
    for (uint32_t ch = 0; ch < chunks_of(c.t_nfold[t]); ++ch) {
      uint32_t incl = c.ch_piece[t * kMaxChunks + ch];
      for (uint32_t p = ch * kChunk; p < c.t_nfold[t] && p < (ch + 1) * kChunk; ++p) {
        incl += piece_at(c, c.t_base[t], p);
        windows_item(c, t, c.t_base[t], c.t_nfold[t], p, incl);
      }
    }
  }
  return 0;
}

}  // extern "C"
