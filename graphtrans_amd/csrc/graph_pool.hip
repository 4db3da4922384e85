// graph_pool.hip -- per-graph read-out of node rows: sum / mean / max with its backward (gt_graph_pool_fwd / gt_graph_pool_bwd).
//
// Reference semantics (paths under /root/reference):
//   global_add_pool / global_mean_pool / global_max_pool(h_node, batch)      models/gnn.py:64-69, :107   (PyG -> torch_scatter atomics,
//   the max's backward through torch_scatter's arg: the FIRST maximum in row order receives the gradient)
// `batch` is sorted (PyG collation), so every graph is a contiguous row range [ptr[b], ptr[b+1]): no atomics, fixed reduction order.
// Sum and mean are the two paths of gt_segment_sum / gt_segment_sum_ws (segment_sum.h); max has the same two paths with (value, row)
// partials.  NaN inputs are out of scope (a NaN never wins a max).
#include "gt_common.h"
#include "segment_sum.h"

namespace {

// ---- per-graph max with the winning row (gt_graph_pool_fwd, GT_POOL_MAX) ----------------------------------------------------
// (value, row) pairs; a later candidate replaces the held one only when it is strictly greater, or on equal values when its row is
// lower: whatever the order the partials meet in, the winner is the FIRST maximum in row order (torch_scatter's arg).  row < 0: none yet.
__device__ __forceinline__ void pmax_take(float& v, int& r, float nv, int nr) {
  if (nr >= 0 && (r < 0 || nv > v || (nv == v && nr < r))) { v = nv; r = nr; }
}
__device__ __forceinline__ void pmax_take4(float4& v, int4& r, float4 nv, int4 nr) {
  pmax_take(v.x, r.x, nv.x, nr.x); pmax_take(v.y, r.y, nv.y, nr.y); pmax_take(v.z, r.z, nv.z, nr.z); pmax_take(v.w, r.w, nv.w, nr.w);
}
// the row walk of one wave: rows ascend, so "strictly greater" alone keeps the first maximum
__device__ __forceinline__ void pmax_row4(float4& v, int4& r, float4 nv, int row) {
  if (r.x < 0 || nv.x > v.x) { v.x = nv.x; r.x = row; }
  if (r.y < 0 || nv.y > v.y) { v.y = nv.y; r.y = row; }
  if (r.z < 0 || nv.z > v.z) { v.z = nv.z; r.z = row; }
  if (r.w < 0 || nv.w > v.w) { v.w = nv.w; r.w = row; }
}

// grid (column tiles of 64 lanes x 4 columns, B) as k_segment_sum; the four waves stride the rows, their partials meet in LDS
template <typename T>
__global__ void __launch_bounds__(SEG_THREADS) k_pool_max(const T* __restrict__ x, const int32_t* __restrict__ gptr, int64_t D,
                                                          T* __restrict__ out, int32_t* __restrict__ arg) {
  __shared__ float4 smv[4][64];
  __shared__ int4 smr[4][64];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * 4;
  const bool act = c < D;
  const int beg = gptr[b], end = gptr[b + 1];
  float4 bv = gt_zero4();
  int4 br = make_int4(-1, -1, -1, -1);
  if (act) {
    int r = beg + wid;
    for (; r + 28 < end; r += 32) {   // 8 independent row loads in flight per wave
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = gt_load4<T>(x + (int64_t)(r + 4 * u) * D + c);
#pragma unroll
      for (int u = 0; u < 8; ++u) pmax_row4(bv, br, v[u], r + 4 * u);
    }
    for (; r < end; r += 4) pmax_row4(bv, br, gt_load4<T>(x + (int64_t)r * D + c), r);
  }
  smv[wid][lane] = bv;
  smr[wid][lane] = br;
  __syncthreads();
  if (wid == 0 && act) {
#pragma unroll
    for (int w = 1; w < 4; ++w) pmax_take4(bv, br, smv[w][lane], smr[w][lane]);
    // (an empty graph: no wave took a row, bv is still 0 and br -1)
    gt_store4<T>(out + (int64_t)b * D + c, bv);
    *reinterpret_cast<int4*>(arg + (int64_t)b * D + c) = br;
  }
}

// the two load-balanced phases of k_segsum_chunks / k_segsum_fixup with (value, row) instead of a sum; head / tail partials carry both
template <typename T>
__global__ void __launch_bounds__(SS_T) k_poolmax_chunks(const T* __restrict__ x, const int32_t* __restrict__ gptr, int B, int64_t N, int64_t D,
                                                         T* __restrict__ out, int32_t* __restrict__ arg, float* __restrict__ head,
                                                         float* __restrict__ tail, int32_t* __restrict__ head_r, int32_t* __restrict__ tail_r) {
  const int64_t p0 = (int64_t)blockIdx.x * SS_CH;
  const int64_t p1 = p0 + SS_CH < N ? p0 + SS_CH : N;
  if (p0 >= p1) return;
  int lo = 0, hi = B;   // invariant: gptr[lo] <= p0 < gptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gptr[mid] <= p0) lo = mid; else hi = mid;
  }
  const int g0 = lo;
  const int64_t ws = (int64_t)blockIdx.x * D;
  for (int64_t c = threadIdx.x; c < D; c += SS_T) {
    int g = g0;
    int64_t gend = gptr[g + 1];
    float acc = 0.f;
    int arow = -1;
    auto flush = [&](int gg, float v, int r) {
      const bool before = gptr[gg] < p0, after = (int64_t)gptr[gg + 1] > p1;
      if (before) { head[ws + c] = v; head_r[ws + c] = r; }
      else if (after) { tail[ws + c] = v; tail_r[ws + c] = r; }
      else { stf<T>(out + (int64_t)gg * D + c, v); arg[(int64_t)gg * D + c] = r; }
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
          flush(g, acc, arow);
          acc = 0.f; arow = -1;
          do { ++g; gend = gptr[g + 1]; } while (gend <= r);
        }
        if (arow < 0 || v[u] > acc) { acc = v[u]; arow = (int)r; }
      }
    }
    flush(g, acc, arow);
  }
}

template <typename T>
__global__ void __launch_bounds__(SS_T) k_poolmax_fixup(const int32_t* __restrict__ gptr, int64_t D, const float* __restrict__ head,
                                                        const float* __restrict__ tail, const int32_t* __restrict__ head_r,
                                                        const int32_t* __restrict__ tail_r, T* __restrict__ out, int32_t* __restrict__ arg) {
  const int b = blockIdx.x;
  const int64_t beg = gptr[b], end = gptr[b + 1];
  if (end > beg && beg / SS_CH == (end - 1) / SS_CH) return;   // inside one chunk: phase 1 stored it
  const int64_t c0 = beg / SS_CH, c1 = end > beg ? (end - 1) / SS_CH : 0;
  for (int64_t c = threadIdx.x; c < D; c += SS_T) {
    float acc = 0.f;
    int arow = -1;
    if (end > beg) {
      acc = tail[c0 * D + c];
      arow = tail_r[c0 * D + c];
      int64_t j = c0 + 1;
      for (; j + 7 <= c1; j += 8) {   // chunks ascend in row order: strictly greater keeps the first maximum
        float v[8];
        int rr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { v[u] = head[(j + u) * D + c]; rr[u] = head_r[(j + u) * D + c]; }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (v[u] > acc) { acc = v[u]; arow = rr[u]; }
      }
      for (; j <= c1; ++j) {
        const float v = head[j * D + c];
        if (v > acc) { acc = v; arow = head_r[j * D + c]; }
      }
    }
    stf<T>(out + (int64_t)b * D + c, acc);
    arg[(int64_t)b * D + c] = arow;
  }
}

// backward of the three read-outs: flat over node rows, every element of dx written once.  KIND: gt_pool_kind
template <typename T, int KIND>
__global__ void __launch_bounds__(SEG_THREADS) k_pool_bwd(const T* __restrict__ d_out, const int32_t* __restrict__ arg,
                                                          const int32_t* __restrict__ gptr, const int32_t* __restrict__ node_graph,
                                                          int64_t N, int64_t D, T* __restrict__ dx) {
  const int64_t C = D / 4;
  const int64_t total = N * C;
  for (int64_t i = (int64_t)blockIdx.x * SEG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * SEG_THREADS) {
    const int64_t r = i / C, c = (i % C) * 4;
    const int g = node_graph[r];
    float4 d = gt_load4<T>(d_out + (int64_t)g * D + c);
    if constexpr (KIND == GT_POOL_MEAN) {
      const int n = gptr[g + 1] - gptr[g];
      d = gt_scale4(d, 1.0f / (float)(n > 1 ? n : 1));
    } else if constexpr (KIND == GT_POOL_MAX) {
      const int4 a = *reinterpret_cast<const int4*>(arg + (int64_t)g * D + c);
      const int ri = (int)r;
      d = make_float4(a.x == ri ? d.x : 0.f, a.y == ri ? d.y : 0.f, a.z == ri ? d.z : 0.f, a.w == ri ? d.w : 0.f);
    }
    gt_store4<T>(dx + r * D + c, d);
  }
}

int check(const char* fn, int dtype, int64_t D) {   // the rule of segment.hip
  if (dtype != GT_F32 && dtype != GT_BF16) { gt_set_error("%s: bad dtype", fn); return GT_ERR_INVALID_ARG; }
  if (D <= 0 || D % 4 != 0) { gt_set_error("%s: dim %lld must be a positive multiple of 4", fn, (long long)D); return GT_ERR_UNSUPPORTED; }
  return GT_OK;
}

int flat_grid(int64_t items) {
  int64_t g = gt_cdiv(items, SEG_THREADS * 4);
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace

// ---- entry points.  One size rule for all three kinds (pool_chunked)
static bool pool_kind_ok(int kind) { return kind == GT_POOL_SUM || kind == GT_POOL_MEAN || kind == GT_POOL_MAX; }

extern "C" size_t gt_graph_pool_workspace_bytes(int kind, int64_t N, int64_t D) {
  if (kind != GT_POOL_MAX) return gt_segment_sum_workspace_bytes(N, D);
  return (size_t)4 * gt_cdiv(N > 0 ? N : 1, SS_CH) * D * sizeof(float) + 256;   // head / tail values + head / tail rows
}
static bool pool_chunked(int kind, int64_t N, int64_t D, const void* workspace, size_t workspace_bytes) {
  return N >= 4096 && workspace && workspace_bytes >= gt_graph_pool_workspace_bytes(kind, N, D);   // the rule of gt_segment_sum_ws
}

template <typename T>
static void pool_fwd_launch(int kind, bool chunked, const void* x_, const int32_t* gptr, int64_t N, int64_t B, int64_t D, void* out_,
                            int32_t* arg, void* workspace, hipStream_t stream) {
  const T* x = (const T*)x_;
  T* out = (T*)out_;
  const int64_t nch = gt_cdiv(N > 0 ? N : 1, SS_CH);
  float* head = static_cast<float*>(workspace);
  float* tail = head + nch * D;
  if (!chunked) {
    const dim3 grid((unsigned)gt_cdiv(D / 4, 64), (unsigned)B);
    if (kind == GT_POOL_SUM) hipLaunchKernelGGL((k_segment_sum<T, false>), grid, dim3(SEG_THREADS), 0, stream, x, (const T*)nullptr, gptr, D, out);
    else if (kind == GT_POOL_MEAN) hipLaunchKernelGGL((k_segment_sum<T, true>), grid, dim3(SEG_THREADS), 0, stream, x, (const T*)nullptr, gptr, D, out);
    else hipLaunchKernelGGL(k_pool_max<T>, grid, dim3(SEG_THREADS), 0, stream, x, gptr, D, out, arg);
  } else if (kind == GT_POOL_SUM) {
    hipLaunchKernelGGL((k_segsum_chunks<T, false>), dim3((unsigned)nch), dim3(SS_T), 0, stream, x, (const T*)nullptr, gptr, (int)B, N, D, out, head, tail);
    hipLaunchKernelGGL((k_segsum_fixup<T, false>), dim3((unsigned)B), dim3(SS_T), 0, stream, (const T*)nullptr, gptr, D, (const float*)head, (const float*)tail, out);
  } else if (kind == GT_POOL_MEAN) {
    hipLaunchKernelGGL((k_segsum_chunks<T, true>), dim3((unsigned)nch), dim3(SS_T), 0, stream, x, (const T*)nullptr, gptr, (int)B, N, D, out, head, tail);
    hipLaunchKernelGGL((k_segsum_fixup<T, true>), dim3((unsigned)B), dim3(SS_T), 0, stream, (const T*)nullptr, gptr, D, (const float*)head, (const float*)tail, out);
  } else {
    int32_t* head_r = reinterpret_cast<int32_t*>(tail + nch * D);
    int32_t* tail_r = head_r + nch * D;
    hipLaunchKernelGGL(k_poolmax_chunks<T>, dim3((unsigned)nch), dim3(SS_T), 0, stream, x, gptr, (int)B, N, D, out, arg, head, tail, head_r, tail_r);
    hipLaunchKernelGGL(k_poolmax_fixup<T>, dim3((unsigned)B), dim3(SS_T), 0, stream, gptr, D, (const float*)head, (const float*)tail,
                       (const int32_t*)head_r, (const int32_t*)tail_r, out, arg);
  }
}

extern "C" int gt_graph_pool_fwd(int kind, int dtype, const void* x, const int32_t* graph_ptr, int64_t N, int64_t B, int64_t D, void* out,
                                 int32_t* arg, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  int rc = check("gt_graph_pool_fwd", dtype, D);
  if (rc) return rc;
  GT_CHECK_ARG(pool_kind_ok(kind), "bad pooling kind");
  GT_CHECK_ARG(graph_ptr && out && (x || N == 0) && (kind != GT_POOL_MAX || arg), "null buffer");
  GT_CHECK_ARG(N >= 0 && B >= 0 && N <= 0x7fffffff, "sizes beyond int32");
  if (B == 0) return GT_OK;
  const bool chunked = pool_chunked(kind, N, D, workspace, workspace_bytes);
  GT_CHECK_ARG(chunked ? B <= 0x7fffffff : B <= 65535, "more than 65535 graphs per batch");
  hipStream_t stream = (hipStream_t)stream_;
  if (dtype == GT_F32) pool_fwd_launch<float>(kind, chunked, x, graph_ptr, N, B, D, out, arg, workspace, stream);
  else pool_fwd_launch<gt_bf16>(kind, chunked, x, graph_ptr, N, B, D, out, arg, workspace, stream);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

template <typename T>
static void pool_bwd_launch(int kind, const void* d_out, const int32_t* arg, const int32_t* gptr, const int32_t* node_graph, int64_t N, int64_t D,
                            void* dx, hipStream_t stream) {
  const dim3 grid(flat_grid(N * (D / 4)));
  if (kind == GT_POOL_SUM)
    hipLaunchKernelGGL((k_pool_bwd<T, GT_POOL_SUM>), grid, dim3(SEG_THREADS), 0, stream, (const T*)d_out, arg, gptr, node_graph, N, D, (T*)dx);
  else if (kind == GT_POOL_MEAN)
    hipLaunchKernelGGL((k_pool_bwd<T, GT_POOL_MEAN>), grid, dim3(SEG_THREADS), 0, stream, (const T*)d_out, arg, gptr, node_graph, N, D, (T*)dx);
  else
    hipLaunchKernelGGL((k_pool_bwd<T, GT_POOL_MAX>), grid, dim3(SEG_THREADS), 0, stream, (const T*)d_out, arg, gptr, node_graph, N, D, (T*)dx);
}

extern "C" int gt_graph_pool_bwd(int kind, int dtype, const void* d_out, const int32_t* arg, const int32_t* graph_ptr, const int32_t* node_graph,
                                 int64_t N, int64_t B, int64_t D, void* dx, gt_stream_t stream_) {
  (void)B;
  int rc = check("gt_graph_pool_bwd", dtype, D);
  if (rc) return rc;
  GT_CHECK_ARG(pool_kind_ok(kind), "bad pooling kind");
  GT_CHECK_ARG(N >= 0 && N <= 0x7fffffff, "sizes beyond int32");
  if (N == 0) return GT_OK;
  GT_CHECK_ARG(d_out && graph_ptr && node_graph && dx && (kind != GT_POOL_MAX || arg), "null buffer");
  hipStream_t stream = (hipStream_t)stream_;
  if (dtype == GT_F32) pool_bwd_launch<float>(kind, d_out, arg, graph_ptr, node_graph, N, D, dx, stream);
  else pool_bwd_launch<gt_bf16>(kind, d_out, arg, graph_ptr, node_graph, N, D, dx, stream);
  GT_CHECK_LAUNCH();
  return GT_OK;
}
