// segment_sum.h -- the per-graph sum kernels of segment.hip, shared with graph_pool.hip (whose sum / mean read-outs ARE these kernels;
// MEAN divides by the graph's row count where the result is written).  `batch` is sorted, so every graph is the contiguous row range
// [gptr[b], gptr[b+1]): no atomics, fixed summation order.
#pragma once
#include "gt_common.h"

namespace {

constexpr int SEG_THREADS = 256;

// out[b] = add[b] + sum_{n in graph b} x[n] ; grid (column tiles of 64 chunks, B); 4 waves stride rows.
// MEAN (gt_graph_pool_fwd): the sum divided by max(n_b, 1) where it is written.
template <typename T, bool MEAN = false>
__global__ void __launch_bounds__(SEG_THREADS) k_segment_sum(const T* __restrict__ x, const T* __restrict__ add,
                                                             const int32_t* __restrict__ gptr, int64_t D,
                                                             T* __restrict__ out) {
  __shared__ float4 sm[4][64];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * 4;
  const bool act = c < D;
  const int beg = gptr[b], end = gptr[b + 1];
  float4 acc = gt_zero4();
  if (act) {
    int r = beg + wid;
    // 8 independent row loads in flight per wave (a serial chain of L2 round trips otherwise)
    for (; r + 28 < end; r += 32) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = gt_load4<T>(x + (int64_t)(r + 4 * u) * D + c);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = gt_add4(acc, v[u]);
    }
    for (; r < end; r += 4) acc = gt_add4(acc, gt_load4<T>(x + (int64_t)r * D + c));
  }
  sm[wid][lane] = acc;
  __syncthreads();
  if (wid == 0 && act) {
    float4 t = gt_add4(gt_add4(sm[0][lane], sm[1][lane]), gt_add4(sm[2][lane], sm[3][lane]));
    if (add) t = gt_add4(t, gt_load4<T>(add + (int64_t)b * D + c));
    if constexpr (MEAN) {
      const float n = (float)(end - beg > 1 ? end - beg : 1);
      t = make_float4(t.x / n, t.y / n, t.z / n, t.w / n);
    }
    gt_store4<T>(out + (int64_t)b * D + c, t);
  }
}

// ---- the same sum in two load-balanced phases (needs a workspace): graph sizes are ragged (11 .. 2000 nodes in
// a Code2 batch) and with one block per graph the largest graph is the kernel's tail (2.4 MB through one CU).
// Phase 1: a block walks SS_CH consecutive ROWS with the running sum in a register (8 rows in flight), starting
// a new sum at every graph boundary; graphs inside the chunk are stored directly, the (at most two) graphs
// that cross its ends leave head / tail partials.  Phase 2: one block per graph adds its partials in chunk
// order (and handles empty graphs).  Fixed order -> reproducible.
constexpr int SS_CH = 64, SS_T = 320;

template <typename T>
__device__ __forceinline__ float ldf(const T* p) {
  if constexpr (sizeof(T) == 4) return (float)*reinterpret_cast<const float*>(p);
  else return gt_bf16_to_f32(*reinterpret_cast<const gt_bf16*>(p));
}
template <typename T>
__device__ __forceinline__ void stf(T* p, float v) {
  if constexpr (sizeof(T) == 4) *reinterpret_cast<float*>(p) = v;
  else *reinterpret_cast<gt_bf16*>(p) = gt_f32_to_bf16(v);
}

template <typename T, bool MEAN = false>
__global__ void __launch_bounds__(SS_T) k_segsum_chunks(const T* __restrict__ x, const T* __restrict__ add,
                                                        const int32_t* __restrict__ gptr, int B, int64_t N, int64_t D,
                                                        T* __restrict__ out, float* __restrict__ head, float* __restrict__ tail) {
  const int64_t p0 = (int64_t)blockIdx.x * SS_CH;
  const int64_t p1 = p0 + SS_CH < N ? p0 + SS_CH : N;
  if (p0 >= p1) return;
  // graph of row p0: last b with gptr[b] <= p0 (empty graphs share a start: take the one that owns the row)
  int lo = 0, hi = B;   // invariant: gptr[lo] <= p0 < gptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gptr[mid] <= p0) lo = mid; else hi = mid;
  }
  const int g0 = lo;
  float* hd = head + (int64_t)blockIdx.x * D;
  float* tl = tail + (int64_t)blockIdx.x * D;
  for (int64_t c = threadIdx.x; c < D; c += SS_T) {
    int g = g0;
    int64_t gend = gptr[g + 1];
    float acc = 0.f;
    auto flush = [&](int gg, float v) {
      const bool before = gptr[gg] < p0, after = (int64_t)gptr[gg + 1] > p1;
      if (before) hd[c] = v;
      else if (after) tl[c] = v;
      else {
        v += add ? ldf<T>(add + (int64_t)gg * D + c) : 0.f;
        if constexpr (MEAN) v /= (float)(gptr[gg + 1] - gptr[gg]);   // (a graph stored here owns a row of the chunk: n >= 1)
        stf<T>(out + (int64_t)gg * D + c, v);
      }
    };
    for (int64_t rb = p0; rb < p1; rb += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = rb + u < p1 ? ldf<T>(x + (rb + u) * D + c) : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t r = rb + u;
        if (r >= p1) break;
        if (r == gend) {            // row r opens the next non-empty graph
          flush(g, acc);
          acc = 0.f;
          do { ++g; gend = gptr[g + 1]; } while (gend <= r);
        }
        acc += v[u];
      }
    }
    flush(g, acc);
  }
}

template <typename T, bool MEAN = false>
__global__ void __launch_bounds__(SS_T) k_segsum_fixup(const T* __restrict__ add, const int32_t* __restrict__ gptr, int64_t D,
                                                       const float* __restrict__ head, const float* __restrict__ tail,
                                                       T* __restrict__ out) {
  const int b = blockIdx.x;
  const int64_t beg = gptr[b], end = gptr[b + 1];
  if (end > beg && beg / SS_CH == (end - 1) / SS_CH) return;   // inside one chunk: phase 1 stored it
  const int64_t c0 = beg / SS_CH, c1 = end > beg ? (end - 1) / SS_CH : 0;
  for (int64_t c = threadIdx.x; c < D; c += SS_T) {
    float acc = 0.f;
    if (end > beg) {
      acc = tail[c0 * D + c];
      int64_t j = c0 + 1;
      for (; j + 7 <= c1; j += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = head[(j + u) * D + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
      }
      for (; j <= c1; ++j) acc += head[j * D + c];
    }
    acc += add ? ldf<T>(add + (int64_t)b * D + c) : 0.f;
    if constexpr (MEAN) acc /= (float)(end - beg > 1 ? end - beg : 1);
    stf<T>(out + (int64_t)b * D + c, acc);
  }
}

}  // namespace
