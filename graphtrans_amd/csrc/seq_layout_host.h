// seq_layout_host.h — the token layout built on the HOST, the one statement of it (gt_seq_layout_host; gt_model_prepare builds with
// it into its staging slot, graphtrans_amd/graph.py:SeqLayout calls the entry).  The reference's pad_batch bookkeeping
// (modules/utils.py:5-29) + the CLS position of modules/transformer_encoder.py:50-55, as ONE blob for one H2D copy:
//   seq_desc [B][4] int32 = {row0, npos, kv_off, kv_len} at offset 0, last_rows [B] int64 (token row of the last position of every
//   sequence: the pooled row) and the attention work list [num_work][2] int32, each at the next multiple of 16 bytes.
// Pure host code.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/graphtrans_hip.h"

struct SeqBlob {
  size_t o_last, o_work, bytes;
};
// the blob's offsets (work_items: entries the work list has room for; a blob is never empty)
static inline SeqBlob seq_blob(int64_t B, int64_t work_items) {
  SeqBlob s;
  s.o_last = ((size_t)B * 16 + 15) / 16 * 16;
  s.o_work = (s.o_last + (size_t)B * 8 + 15) / 16 * 16;
  s.bytes = std::max(s.o_work + (size_t)work_items * 8, (size_t)16);
  return s;
}

struct SeqHostLayout {
  int kind;
  int64_t B, S, rows, max_npos, num_work, row_stride;
  SeqBlob blob;
  std::vector<int64_t> kv;       // kv_len of every sequence
  std::vector<int32_t> order;    // the sequences by descending npos (ties: by index)
  int64_t npos(int64_t b) const { return kind == GT_SEQ_PADDED ? max_npos : kv[(size_t)b]; }
};

// Sizes and the length ranking; seq_layout_fill writes the blob from them.
// Attention work list: {sequence, 64-position tile} for every tile that exists.  Longest sequences FIRST: a block walks all keys
// (queries) of its sequence tile by tile, so the longest sequence's blocks are a serial chain several times the typical one
// (Code2-like: 418 against 126 tokens) -- started last it was the tail of every attention launch.  The kernels give XCD x the x-th
// contiguous eighth of the list (one L2 per sequence) and dispatch each eighth front to back: sequences are dealt to the eighths by
// length rank, each eighth holds its own in descending length, padded with {-1, 0} entries (skipped) to equal size.
static inline SeqHostLayout seq_layout_rank(int kind, const int64_t* n, int64_t B, int64_t max_input_len, int cls) {
  SeqHostLayout h{};
  h.kind = kind;
  h.B = B;
  for (int64_t b = 0; b < B; ++b) h.S = std::max(h.S, n[b]);
  h.S = std::min(h.S, max_input_len);   // modules/utils.py:16
  h.kv.resize((size_t)B);
  int64_t sum = 0, longest = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t k = h.kv[(size_t)b] = std::min(n[b], h.S) + cls;
    sum += k;
    longest = std::max(longest, k);
  }
  if (kind == GT_SEQ_PADDED) {
    h.max_npos = h.S + cls;
    h.rows = h.max_npos * B;
    h.row_stride = B;
  } else {
    h.max_npos = longest;
    h.rows = sum;
    h.row_stride = 1;
  }
  h.order.resize((size_t)B);
  for (int64_t b = 0; b < B; ++b) h.order[(size_t)b] = (int32_t)b;
  if (kind != GT_SEQ_PADDED)   // (padded: every npos is the same, the order by index stands)
    std::stable_sort(h.order.begin(), h.order.end(), [&](int32_t a, int32_t c) { return h.kv[(size_t)a] > h.kv[(size_t)c]; });
  int64_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // tiles per eighth
  for (int64_t r = 0; r < B; ++r) cnt[r % 8] += (h.npos(h.order[(size_t)r]) + 63) / 64;
  h.num_work = B ? 8 * *std::max_element(cnt, cnt + 8) : 0;
  h.blob = seq_blob(B, h.num_work);
  return h;
}

static inline void seq_layout_fill(const SeqHostLayout& h, char* dst) {
  int32_t* desc = (int32_t*)dst;
  int64_t* last = (int64_t*)(dst + h.blob.o_last);
  int32_t* work = (int32_t*)(dst + h.blob.o_work);
  const int64_t B = h.B;
  int64_t row = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t k = h.kv[(size_t)b], np = h.npos(b);
    desc[b * 4 + 0] = (int32_t)(h.kind == GT_SEQ_PADDED ? b : row);
    desc[b * 4 + 1] = (int32_t)np;
    desc[b * 4 + 2] = (int32_t)(np - k);
    desc[b * 4 + 3] = (int32_t)k;
    last[b] = desc[b * 4] + (np - 1) * h.row_stride;
    row += k;
  }
  const int64_t wpx = h.num_work / 8;
  for (int64_t i = 0; i < h.num_work; ++i) { work[2 * i] = -1; work[2 * i + 1] = 0; }
  for (int x = 0; x < 8; ++x) {
    int64_t pos = (int64_t)x * wpx;
    for (int64_t r = x; r < B; r += 8) {
      const int32_t s = h.order[(size_t)r];
      const int64_t t = (h.npos(s) + 63) / 64;
      for (int64_t j = 0; j < t; ++j) { work[2 * pos] = s; work[2 * pos + 1] = (int32_t)j; ++pos; }
    }
  }
}
