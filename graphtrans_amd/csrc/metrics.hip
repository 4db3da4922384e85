// metrics.hip — the evaluation metrics of the three dataset families on the device, with no host round trip per batch.
//
// The reference's `eval` (dataset/code.py:49-78, dataset/mol.py:36-58, dataset/tud.py:33-43) copies every batch of logits to the
// host: torch.argmax per head + a Python loop over graphs with `set`s (Code2 F1), 128 scikit-learn average_precision_score calls
// (Molpcba AP), `.item()` per batch (TU accuracy).  Here a batch costs two small launches behind the forward and the one
// synchronisation of a pass is the read of the final numbers:
//   k_argmax_block / k_argmax_wave : pred[b][h] = argmax of head h's C logits (torch.argmax's rule)   -- the hot kernel, HBM-bound
//   k_seq_f1                       : per graph: decode at __EOS__, set precision / recall / F1 in float64 (the OGB F1 evaluator)
//   k_rows_mean                    : mean (or plain sum) of the per-graph rows, float64, fixed order
//   k_count_correct                : count += #{pred == y}                                          (TU accuracy)
//   k_ap_sorted                    : average precision of one task per block over its scores sorted descending (Molpcba AP)
//   k_auc_sorted                   : ROC-AUC of one task per block over the same sorted table, in integers (Molhiv ROC-AUC)
// No kernel uses an atomic; every sum has a fixed order, so two runs are bit-identical.
#include "gt_common.h"

#pragma clang fp contract(off)   // the float64 metric arithmetic is the statement's: one correctly rounded operation each

namespace {

constexpr int MT = 256;
constexpr int ARGMAX_WAVE_MAX_C = 1024;   // up to here one wave per (b, h) row (four rows per block), above one block per row
constexpr int EVAL_MAX_H = 16, EVAL_MAX_R = 64;

// ---- argmax ------------------------------------------------------------------------------------------------------------------
// torch.argmax: the first maximum in column order; a NaN counts as the maximum and the first NaN wins; -0 == +0.
// In a thread the columns come in ascending order, so "strictly better" keeps the first.
__device__ __forceinline__ void am_take(float& bv, int& bi, float v, int i) {
  if (v > bv || (v != v && bv == bv)) { bv = v; bi = i; }
}
__device__ __forceinline__ void am_take4(float& bv, int& bi, float4 v, int i) {
  am_take(bv, bi, v.x, i);
  am_take(bv, bi, v.y, i + 1);
  am_take(bv, bi, v.z, i + 2);
  am_take(bv, bi, v.w, i + 3);
}
// (value, index) as one integer whose maximum is the winner among threads: the value's order-preserving image in the high word
// (NaN above +inf, the two zeros equal), the complemented index in the low word (the smaller index wins a tie)
__device__ __forceinline__ uint64_t am_pack(float v, int i) {
  uint32_t k;
  if (v != v) k = 0xffffffffu;
  else {
    const uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((uint64_t)k << 32) | (uint32_t)(0x7fffffff - i);
}
__device__ __forceinline__ int am_index(uint64_t key) { return 0x7fffffff - (int)(uint32_t)(key & 0xffffffffu); }
__device__ __forceinline__ uint64_t am_wave_max(uint64_t k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor(k, o, 64);
    k = u > k ? u : k;
  }
  return k;
}

// One row of C floats by NT threads.  The row starts at any 4-byte boundary (5002-column heads do): the columns between its first
// and its last 16-byte boundary are read with 16-byte loads, the at most 3 + 3 columns outside one by one -- a row that holds no whole
// 16-byte piece (C < 4, or an offset base with C < 7) is read scalar altogether.  One load per trip: the 20 waves a CU holds keep
// enough in flight; 2 and 4 loads in flight per thread measured 4 % slower per Code2 batch, 8 a further 22 % (profiles/LOG.md).
// A thread that sees no column reports (-inf, 0): it loses to anything but an all -inf row, whose answer is 0.
template <int NT>
__device__ __forceinline__ uint64_t am_row(const float* __restrict__ x, int C, int tid) {
  float bv = -INFINITY;
  int bi = 0;
  int head = (int)((4u - (unsigned)(((uintptr_t)x >> 2) & 3u)) & 3u);
  head = head < C ? head : C;
  if (tid < head) am_take(bv, bi, x[tid], tid);
  const int nvec = (C - head) >> 2;
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);
#pragma unroll 1
  for (int i = tid; i < nvec; i += NT) am_take4(bv, bi, xv[i], head + 4 * i);
  const int t = head + 4 * nvec + tid;
  if (t < C) am_take(bv, bi, x[t], t);
  return am_pack(bv, bi);
}

__global__ void __launch_bounds__(MT) k_argmax_block(const float* __restrict__ logits, int H, int C, int64_t ld, int64_t head_stride,
                                                     int32_t* __restrict__ pred) {
  __shared__ uint64_t red[MT / 64];
  const int64_t row = blockIdx.x, b = row / H, h = row % H;
  uint64_t k = am_wave_max(am_row<MT>(logits + b * ld + h * head_stride, C, threadIdx.x));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < MT / 64; ++w) k = red[w] > k ? red[w] : k;
    pred[row] = am_index(k);
  }
}

__global__ void __launch_bounds__(MT) k_argmax_wave(const float* __restrict__ logits, int64_t rows, int H, int C, int64_t ld,
                                                    int64_t head_stride, int32_t* __restrict__ pred) {
  const int64_t row = (int64_t)blockIdx.x * (MT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;   // the same in every lane of a wave; no barrier below
  const int64_t b = row / H, h = row % H;
  const uint64_t k = am_wave_max(am_row<64>(logits + b * ld + h * head_stride, C, threadIdx.x & 63));
  if ((threadIdx.x & 63) == 0) pred[row] = am_index(k);
}

// ---- block-wide helpers (MT threads, every thread calls) -----------------------------------------------------------------------
__device__ __forceinline__ int blk_sum_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}
__device__ __forceinline__ int64_t blk_sum_i64(int64_t v, int64_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}
__device__ __forceinline__ double blk_sum_f64(double v, double* red) {   // a fixed tree: the same bits in every thread, every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}
// inclusive and exclusive scan over the block's threads of non-negative ints (identity 0), by + or by max; total = all threads
template <bool MAX>
__device__ __forceinline__ int scan_op(int a, int b) { return MAX ? (a > b ? a : b) : a + b; }
template <bool MAX>
__device__ __forceinline__ void blk_scan(int v, int* red, int& incl, int& excl, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v = scan_op<MAX>(v, u);
  }
  const int left = __shfl_up(v, 1, 64);
  if (lane == 63) red[w] = v;
  __syncthreads();
  int pre = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < MT / 64; ++k) {
    const int r = red[k];
    if (k < w) pre = scan_op<MAX>(pre, r);
    total = scan_op<MAX>(total, r);
  }
  __syncthreads();
  incl = scan_op<MAX>(pre, v);
  excl = lane == 0 ? pre : scan_op<MAX>(pre, left);
}

// ---- Code2: set precision / recall / F1 of every graph ----------------------------------------------------------------------
// One thread per graph; the prediction is at most 16 ids and the reference set at most 64, so everything is re-read from L1.
__global__ void __launch_bounds__(MT) k_seq_f1(const int32_t* __restrict__ pred, int64_t B, int H, int C,
                                               const int32_t* __restrict__ ref_ids, const int32_t* __restrict__ n_ref, int R, int64_t G,
                                               const int64_t* __restrict__ graph_ids, double* __restrict__ rows) {
  const int64_t b = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (b >= B) return;
  double* o = rows + 3 * b;
  const int64_t g = graph_ids ? graph_ids[b] : b;
  if (g < 0 || g >= G) {   // no reference for this graph: poison the row, the mean shows it
    o[0] = o[1] = o[2] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const int32_t* p = pred + b * H;
  const int32_t* ref = ref_ids + g * R;
  const int eos = C - 1, unk = C - 2;
  int npred = 0, tp = 0;
  for (int l = 0; l < H; ++l) {
    const int w = p[l];
    if (w == eos) break;   // decode_arr_to_seq: cut at the first __EOS__
    bool dup = false;
    for (int j = 0; j < l; ++j) dup |= p[j] == w;
    if (dup) continue;     // a set: duplicates collapse
    ++npred;
    if (w == unk) continue;   // the word "__UNK__" matches no reference word
    bool hit = false;
    for (int r = 0; r < R; ++r) hit |= ref[r] == w;   // ids are >= 0, the -1 padding never matches
    tp += hit ? 1 : 0;
  }
  const int fp = npred - tp, fn = n_ref[g] - tp;
  const double precision = tp + fp > 0 ? (double)tp / (double)(tp + fp) : 0.0;
  const double recall = tp + fn > 0 ? (double)tp / (double)(tp + fn) : 0.0;
  const double f1 = precision + recall > 0.0 ? 2.0 * precision * recall / (precision + recall) : 0.0;
  o[0] = precision;
  o[1] = recall;
  o[2] = f1;
}

// out[k] = (sum_i rows[i][k]) / n: thread t adds rows t, t + MT, ... in order, then the fixed tree; depends on n alone.
// MEAN = false leaves the division out: the sums that ranks exchange (a mean of means is not the mean).
template <bool MEAN>
__global__ void __launch_bounds__(MT) k_rows_mean(const double* __restrict__ rows, int64_t n, double* __restrict__ out) {
  __shared__ double red[MT / 64];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += MT) {
    s0 += rows[3 * i];
    s1 += rows[3 * i + 1];
    s2 += rows[3 * i + 2];
  }
  s0 = blk_sum_f64(s0, red);
  s1 = blk_sum_f64(s1, red);
  s2 = blk_sum_f64(s2, red);
  if (threadIdx.x == 0) {
    out[0] = MEAN ? s0 / (double)n : s0;
    out[1] = MEAN ? s1 / (double)n : s1;
    out[2] = MEAN ? s2 / (double)n : s2;
  }
}

// one block, one writer: launches on one stream accumulate exactly
__global__ void __launch_bounds__(MT) k_count_correct(const int32_t* __restrict__ pred, const int64_t* __restrict__ y, int64_t B,
                                                      int64_t* __restrict__ count) {
  __shared__ int red[MT / 64];
  int64_t total = 0;
  for (int64_t base = 0; base < B; base += (int64_t)MT * 4096) {   // an int per trip cannot overflow
    const int64_t end = base + (int64_t)MT * 4096 < B ? base + (int64_t)MT * 4096 : B;
    int c = 0;
    for (int64_t i = base + threadIdx.x; i < end; i += MT) c += (int64_t)pred[i] == y[i] ? 1 : 0;
    total += blk_sum_int(c, red);
  }
  if (threadIdx.x == 0) count[0] += total;
}

// ---- Molpcba: average precision of one task per block -----------------------------------------------------------------------
// scores sorted descending, labels in the same order (NaN = unlabelled, skipped wherever it stands).  With tp_i, fp_i the labelled
// positives / negatives among entries 0..i, and the thresholds at the ends of the runs of equal scores,
//   AP = sum over run ends e of (tp_e / P - tp_e' / P) * tp_e / (tp_e + fp_e),   e' = the run end before e (tp = 0 before the first)
// A run without a labelled positive adds nothing, so runs of unlabelled entries and scikit-learn's thresholds "at the distinct
// scores of the labelled entries" give the same sum.  The block walks the task in chunks of MT entries: a + scan gives tp_i, fp_i
// (carried from chunk to chunk), and since tp never falls, tp_e' is the running maximum of tp over the run ends before i -- a max
// scan, carried as well, so a tie run that crosses a chunk border is one threshold like any other.
__global__ void __launch_bounds__(MT) k_ap_sorted(const float* __restrict__ scores, const float* __restrict__ labels, int64_t n,
                                                  int64_t ld, double* __restrict__ ap, uint8_t* __restrict__ valid) {
  __shared__ int red[MT / 64];
  __shared__ double redd[MT / 64];
  const int64_t t = blockIdx.x;
  const float* __restrict__ sc = scores + t * ld;
  const float* __restrict__ lb = labels + t * ld;
  int pos = 0, neg = 0, bad = 0;
  for (int64_t i = threadIdx.x; i < n; i += MT) {
    const float y = lb[i], s = sc[i];
    if (y == y) {
      pos += y == 1.f ? 1 : 0;
      neg += y == 1.f ? 0 : 1;
      bad += s != s ? 1 : 0;
    }
  }
  const int P = blk_sum_int(pos, red), N = blk_sum_int(neg, red);
  bad = blk_sum_int(bad, red);
  if (bad || P == 0 || N == 0) {   // the same in every thread
    if (threadIdx.x == 0) {
      ap[t] = 0.0;
      valid[t] = bad ? 2 : 0;   // 2: a labelled entry has a NaN score
    }
    return;
  }
  int tp_c = 0, fp_c = 0, m_c = 0;
  double sum = 0.0;
  for (int64_t base = 0; base < n; base += MT) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < n;
    const float s = in ? sc[i] : 0.f;
    const float y = in ? lb[i] : 0.f;
    const bool lab = in && y == y, p1 = lab && y == 1.f, n1 = lab && !p1;
    const bool end = in && (i == n - 1 || sc[i + 1] != s);
    int inc, exc, tot;
    blk_scan<false>((p1 ? 1 : 0) | (n1 ? 1 << 16 : 0), red, inc, exc, tot);   // a chunk holds at most 256 of either
    const int tp = tp_c + (inc & 0xffff), fp = fp_c + (inc >> 16);
    int minc, mexc, mtot;
    blk_scan<true>(end ? tp : 0, red, minc, mexc, mtot);
    const int tp_prev = m_c > mexc ? m_c : mexc;
    double term = 0.0;
    if (end && tp > tp_prev)
      term = ((double)tp / (double)P - (double)tp_prev / (double)P) * ((double)tp / (double)(tp + fp));
    sum += blk_sum_f64(term, redd);
    tp_c += tot & 0xffff;
    fp_c += tot >> 16;
    m_c = m_c > mtot ? m_c : mtot;
  }
  if (threadIdx.x == 0) {
    ap[t] = sum;
    valid[t] = 1;
  }
}

// ---- Molhiv: ROC-AUC of one task per block ----------------------------------------------------------------------------------
// The table of k_ap_sorted.  With tp_e, fp_e the labelled positives / negatives among entries 0..e at the end e of a run of equal
// scores and tp_e', fp_e' the same at the run end before it (0 before the first), the trapezoids of scikit-learn's roc_auc_score are
//   AUC = num / (2 P N),   num = sum over run ends e of (fp_e - fp_e') * (tp_e + tp_e')
// an integer below n^2 / 2 < 2^61, kept in int64 (it passes 2^32 at n = 100 000).  A run without a labelled negative adds nothing,
// so unlabelled entries may stand anywhere.  tp and fp never fall, so their values at the previous run end are running maxima over
// the run ends before i: two max scans, carried from chunk to chunk like the + scan's totals -- a tie run over any number of chunk
// borders is one threshold.  The one floating-point operation is the division: for 2 P N < 2^53 the correctly rounded quotient.
__global__ void __launch_bounds__(MT) k_auc_sorted(const float* __restrict__ scores, const float* __restrict__ labels, int64_t n,
                                                   int64_t ld, double* __restrict__ auc, uint8_t* __restrict__ valid) {
  __shared__ int red[MT / 64];
  __shared__ int64_t redl[MT / 64];
  const int64_t t = blockIdx.x;
  const float* __restrict__ sc = scores + t * ld;
  const float* __restrict__ lb = labels + t * ld;
  int pos = 0, neg = 0, bad = 0;
  for (int64_t i = threadIdx.x; i < n; i += MT) {
    const float y = lb[i], s = sc[i];
    if (y == y) {
      pos += y == 1.f ? 1 : 0;
      neg += y == 1.f ? 0 : 1;
      bad += s != s ? 1 : 0;
    }
  }
  const int P = blk_sum_int(pos, red), N = blk_sum_int(neg, red);
  bad = blk_sum_int(bad, red);
  if (bad || P == 0 || N == 0) {   // the same in every thread
    if (threadIdx.x == 0) {
      auc[t] = 0.0;
      valid[t] = bad ? 2 : 0;   // 2: a labelled entry has a NaN score
    }
    return;
  }
  int tp_c = 0, fp_c = 0, mt_c = 0, mf_c = 0;
  int64_t num = 0;   // this thread's terms; one block sum behind the walk
  for (int64_t base = 0; base < n; base += MT) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < n;
    const float s = in ? sc[i] : 0.f;
    const float y = in ? lb[i] : 0.f;
    const bool lab = in && y == y, p1 = lab && y == 1.f, n1 = lab && !p1;
    const bool end = in && (i == n - 1 || sc[i + 1] != s);
    int inc, exc, tot;
    blk_scan<false>((p1 ? 1 : 0) | (n1 ? 1 << 16 : 0), red, inc, exc, tot);   // a chunk holds at most 256 of either
    const int tp = tp_c + (inc & 0xffff), fp = fp_c + (inc >> 16);
    int tinc, texc, ttot, finc, fexc, ftot;
    blk_scan<true>(end ? tp : 0, red, tinc, texc, ttot);
    blk_scan<true>(end ? fp : 0, red, finc, fexc, ftot);
    const int tp_prev = mt_c > texc ? mt_c : texc, fp_prev = mf_c > fexc ? mf_c : fexc;
    if (end) num += (int64_t)(fp - fp_prev) * (int64_t)(tp + tp_prev);
    tp_c += tot & 0xffff;
    fp_c += tot >> 16;
    mt_c = mt_c > ttot ? mt_c : ttot;
    mf_c = mf_c > ftot ? mf_c : ftot;
  }
  num = blk_sum_i64(num, redl);
  if (threadIdx.x == 0) {
    auc[t] = (double)num / (double)(2 * (int64_t)P * (int64_t)N);
    valid[t] = 1;
  }
}

}  // namespace

extern "C" int gt_eval_argmax(const float* logits, int64_t B, int64_t H, int64_t C, int64_t ld, int64_t head_stride,
                              int32_t* pred, gt_stream_t stream_) {
  if (H > EVAL_MAX_H || C < 1) {
    gt_set_error("gt_eval_argmax: 1 <= C and H <= 16 heads are built");
    return GT_ERR_UNSUPPORTED;
  }
  GT_CHECK_ARG(B > 0 && H > 0 && C < INT32_MAX && B * H < INT32_MAX, "bad sizes");
  GT_CHECK_ARG(head_stride >= C && ld >= (H - 1) * head_stride + C, "heads overlap or pass the row");
  GT_CHECK_ARG(logits && pred && !((uintptr_t)logits & 3), "null or unaligned buffer");
  hipStream_t stream = (hipStream_t)stream_;
  GtProfScope prof__(GT_PROF_NORM, "gt_eval_argmax", stream_, {B, H, C});
  const int64_t rows = B * H;
  if (C <= ARGMAX_WAVE_MAX_C)
    hipLaunchKernelGGL(k_argmax_wave, dim3((unsigned)gt_cdiv(rows, MT / 64)), dim3(MT), 0, stream, logits, rows, (int)H, (int)C, ld,
                       head_stride, pred);
  else
    hipLaunchKernelGGL(k_argmax_block, dim3((unsigned)rows), dim3(MT), 0, stream, logits, (int)H, (int)C, ld, head_stride, pred);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_eval_seq_f1(const int32_t* pred, int64_t B, int64_t H, int64_t C, const int32_t* ref_ids, const int32_t* n_ref,
                              int64_t R, int64_t G, const int64_t* graph_ids, double* rows, int64_t row_off, int64_t rows_cap,
                              gt_stream_t stream_) {
  if (H > EVAL_MAX_H || R > EVAL_MAX_R) {
    gt_set_error("gt_eval_seq_f1: H <= 16 positions and R <= 64 reference words are built");
    return GT_ERR_UNSUPPORTED;
  }
  GT_CHECK_ARG(B > 0 && H > 0 && R > 0 && C >= 2 && C < INT32_MAX && G > 0, "bad sizes");
  GT_CHECK_ARG(pred && ref_ids && n_ref && rows, "null buffer");
  GT_CHECK_ARG(row_off >= 0 && row_off + B <= rows_cap, "rows [row_off, row_off + B) pass the end of the row buffer");
  GT_CHECK_ARG(graph_ids || B <= G, "without graph_ids the batch is graphs 0..B-1 of the reference table");
  GtProfScope prof__(GT_PROF_NORM, "gt_eval_seq_f1", stream_, {B, H, R});
  hipLaunchKernelGGL(k_seq_f1, dim3((unsigned)gt_cdiv(B, MT)), dim3(MT), 0, (hipStream_t)stream_, pred, B, (int)H, (int)C, ref_ids,
                     n_ref, (int)R, G, graph_ids, rows + 3 * row_off);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_eval_rows_mean_f64(const double* rows, int64_t n, double* out, gt_stream_t stream_) {
  GT_CHECK_ARG(n > 0, "no rows");
  GT_CHECK_ARG(rows && out, "null buffer");
  hipLaunchKernelGGL(k_rows_mean<true>, dim3(1), dim3(MT), 0, (hipStream_t)stream_, rows, n, out);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_eval_rows_sum_f64(const double* rows, int64_t n, double* out, gt_stream_t stream_) {
  GT_CHECK_ARG(n > 0, "no rows");
  GT_CHECK_ARG(rows && out, "null buffer");
  hipLaunchKernelGGL(k_rows_mean<false>, dim3(1), dim3(MT), 0, (hipStream_t)stream_, rows, n, out);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_eval_count_correct(const int32_t* pred, const int64_t* y, int64_t B, int64_t* count, gt_stream_t stream_) {
  GT_CHECK_ARG(B > 0, "bad sizes");
  GT_CHECK_ARG(pred && y && count, "null buffer");
  hipLaunchKernelGGL(k_count_correct, dim3(1), dim3(MT), 0, (hipStream_t)stream_, pred, y, B, count);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_eval_ap_sorted(const float* scores, const float* labels, int64_t T, int64_t n, int64_t ld, double* ap,
                                 uint8_t* valid, gt_stream_t stream_) {
  GT_CHECK_ARG(T > 0 && T < INT32_MAX && n > 0 && n < INT32_MAX && ld >= n, "bad sizes");
  GT_CHECK_ARG(scores && labels && ap && valid, "null buffer");
  GtProfScope prof__(GT_PROF_NORM, "gt_eval_ap_sorted", stream_, {T, n});
  hipLaunchKernelGGL(k_ap_sorted, dim3((unsigned)T), dim3(MT), 0, (hipStream_t)stream_, scores, labels, n, ld, ap, valid);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_eval_auc_sorted(const float* scores, const float* labels, int64_t T, int64_t n, int64_t ld, double* auc,
                                  uint8_t* valid, gt_stream_t stream_) {
  GT_CHECK_ARG(T > 0 && T < INT32_MAX && n > 0 && n < INT32_MAX && ld >= n, "bad sizes");
  GT_CHECK_ARG(scores && labels && auc && valid, "null buffer");
  GtProfScope prof__(GT_PROF_NORM, "gt_eval_auc_sorted", stream_, {T, n});
  hipLaunchKernelGGL(k_auc_sorted, dim3((unsigned)T), dim3(MT), 0, (hipStream_t)stream_, scores, labels, n, ld, auc, valid);
  GT_CHECK_LAUNCH();
  return GT_OK;
}
