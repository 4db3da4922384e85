// collate.hip — mini-batch assembly on the device: a list of graph ids of an HBM-resident graph store
// becomes the concatenated batch the message-passing path consumes, including the Code2 edge
// augmentation the reference runs on every sample.
//
// Reference (paths under /root/reference):
//   * `augment_edge` (dataset/utils.py:89-141), installed as the per-sample transform
//     (dataset/code.py:97-101): edges of a graph become [ast, ast^-1, next-token, next-token^-1],
//     edge_attr (E,2) float32 = (is next-token, is inverse); the next-token chain links consecutive nodes
//     with node_is_attributed == 1 in node order.
//   * PyG 1.6.3 `Batch.from_data_list` behind `DataLoader` (main.py:149-152): attributes concatenated
//     along dim 0, edge_index along dim 1 and shifted by the node offset of its graph, `batch[v] = i`.
// The reference does this in Python per sample on DataLoader workers; here the whole dataset sits in HBM
// (ogbg-code2 is ~1.3 GB of int64) and a batch costs two launches.  All integer work, bit-exact.
//
// Layout: the store holds per-graph slices of concatenated arrays (node_ptr/edge_ptr, local node ids in the
// edges).  `attr_rank` = exclusive prefix sum of (node_is_attributed == 1) over ALL store nodes, built once
// by gt_attr_rank: rank differences give a node's position in its graph's next-token chain without a
// per-batch compaction.  One block row per selected graph; nodes and edges are strided by the block.
//
// Float features (TU datasets: x (N,37) f32, dataset/tud.py; ER-shaped stores: x (N,256) f32 + edge_attr (E,2) f32): a graph's
// rows are contiguous in the store and in the batch, so they move as ONE flat run per graph (16-byte vectors where both ends
// are 16-byte aligned, coalesced dwords otherwise) instead of the per-node column loop of the int64 path.  The fill kernel is
// instantiated twice; the all-int64 instance is the kernel as it was before float features existed.
//
// PNA in-degree histogram (dataset/code.py:119-132, dataset/mol.py:70-81: `degree(edge_index[1])` + `bincount` per training
// graph, on Code2 over the AUGMENTED edges): gt_store_in_degree counts every store node's in-degree over the edges gt_collate
// would emit, gt_degree_histogram bins the nodes of a selection of graphs.  Integer atomics only: exact, order-independent.
#include "gt_common.h"

namespace {

constexpr int CT = 256;
constexpr int SCAN_T = 1024;

// ---- exclusive prefix sum of (flag == 1), single block, chunked (one-off per dataset) -----------------
__global__ void __launch_bounds__(SCAN_T) k_attr_rank(const int64_t* __restrict__ flag, int64_t n, int64_t* __restrict__ rank) {
  __shared__ int64_t wsum[SCAN_T / GT_WAVE];
  __shared__ int64_t carry_s;
  const int tid = threadIdx.x, lane = tid & (GT_WAVE - 1), w = tid / GT_WAVE;
  constexpr int PER = 8;  // consecutive elements per thread
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += (int64_t)SCAN_T * PER) {
    const int64_t i0 = base + (int64_t)tid * PER;
    int v[PER];
    int tsum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      v[k] = (i0 + k < n && flag[i0 + k] == 1) ? 1 : 0;
      tsum += v[k];
    }
    int incl = tsum;  // wave inclusive scan
#pragma unroll
    for (int o = 1; o < GT_WAVE; o <<= 1) {
      const int t = __shfl_up(incl, o, GT_WAVE);
      if (lane >= o) incl += t;
    }
    if (lane == GT_WAVE - 1) wsum[w] = incl;
    __syncthreads();
    int64_t pre = carry_s;
    for (int k = 0; k < w; ++k) pre += wsum[k];
    int64_t run = pre + (incl - tsum);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (i0 + k < n) rank[i0 + k] = run;
      run += v[k];
    }
    __syncthreads();
    if (tid == SCAN_T - 1) carry_s = run;
    __syncthreads();
  }
  if (tid == 0) rank[n] = carry_s;
}

struct CollateArgs {
  gt_graph_store s;
  gt_collate_out o;
  const int64_t* ids;
  int64_t B, N, E;
  int64_t* node_off;  // (B+1) workspace
  int64_t* edge_off;  // (B+1) workspace
};

__device__ __forceinline__ int64_t out_edges(const gt_graph_store& s, int64_t g) {
  const int64_t e = s.edge_ptr[g + 1] - s.edge_ptr[g];
  if (!s.attr_rank) return e;
  const int64_t a = s.attr_rank[s.node_ptr[g + 1]] - s.attr_rank[s.node_ptr[g]];
  return 2 * e + 2 * (a > 1 ? a - 1 : 0);
}

// ---- per-batch offsets: exclusive scans of node and output-edge counts over the selected graphs -------
__global__ void __launch_bounds__(SCAN_T) k_collate_offsets(CollateArgs a) {
  __shared__ int64_t wn[SCAN_T / GT_WAVE], we[SCAN_T / GT_WAVE];
  __shared__ int64_t cn, ce;
  const int tid = threadIdx.x, lane = tid & (GT_WAVE - 1), w = tid / GT_WAVE;
  if (tid == 0) cn = ce = 0;
  __syncthreads();
  for (int64_t base = 0; base < a.B; base += SCAN_T) {
    const int64_t i = base + tid;
    int64_t n = 0, e = 0;
    if (i < a.B) {
      const int64_t g = a.ids[i];
      n = a.s.node_ptr[g + 1] - a.s.node_ptr[g];
      e = out_edges(a.s, g);
    }
    int64_t in = n, ie = e;
#pragma unroll
    for (int o = 1; o < GT_WAVE; o <<= 1) {
      const int64_t tn = __shfl_up(in, o, GT_WAVE), te = __shfl_up(ie, o, GT_WAVE);
      if (lane >= o) { in += tn; ie += te; }
    }
    if (lane == GT_WAVE - 1) { wn[w] = in; we[w] = ie; }
    __syncthreads();
    int64_t pn = cn, pe = ce;
    for (int k = 0; k < w; ++k) { pn += wn[k]; pe += we[k]; }
    if (i < a.B) {
      a.node_off[i] = pn + in - n;
      a.edge_off[i] = pe + ie - e;
      if (a.o.ptr) a.o.ptr[i] = pn + in - n;
    }
    __syncthreads();
    if (tid == SCAN_T - 1) { cn = pn + in; ce = pe + ie; }
    __syncthreads();
  }
  if (tid == 0) {
    a.node_off[a.B] = cn;
    a.edge_off[a.B] = ce;
    if (a.o.ptr) a.o.ptr[a.B] = cn;
  }
}

// one graph's contiguous float rows: `cnt` floats from src to dst, strided by the blocks of the graph's row.  float4 when both
// ends are 16-byte aligned (always so when the column count is a multiple of 4 and the arrays are), dwords otherwise
__device__ __forceinline__ void copy_run_f32(const float* __restrict__ src, float* __restrict__ dst, int64_t cnt, int t0, int stride) {
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    const int64_t q = cnt >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int64_t k = t0; k < q; k += stride) d4[k] = s4[k];
    for (int64_t k = 4 * q + t0; k < cnt; k += stride) dst[k] = src[k];
  } else {
    for (int64_t k = t0; k < cnt; k += stride) dst[k] = src[k];
  }
}

// ---- fill: grid (B, Y); block (i, y) strides over graph i's nodes and stored edges --------------------
// FLT: the store holds a float array (x_f32 and / or edge_attr_f32); false = every feature is int64
template <bool FLT>
__global__ void __launch_bounds__(CT) k_collate_fill(CollateArgs a) {
  const int64_t i = blockIdx.x;
  const gt_graph_store& s = a.s;
  const gt_collate_out& o = a.o;
  const int64_t g = a.ids[i];
  const int64_t ns = s.node_ptr[g], n = s.node_ptr[g + 1] - ns;
  const int64_t es = s.edge_ptr[g], e = s.edge_ptr[g + 1] - es;
  const int64_t no = a.node_off[i], eo = a.edge_off[i];
  const bool aug = s.attr_rank != nullptr;
  int64_t r0 = 0, m = 0;
  if (aug) {
    r0 = s.attr_rank[ns];
    const int64_t cnt = s.attr_rank[ns + n] - r0;
    m = cnt > 1 ? cnt - 1 : 0;
  }
  const int64_t eout = aug ? 2 * e + 2 * m : e;
  // a caller-supplied N / E smaller than the true totals must not turn into out-of-bounds writes
  if (no + n > a.N || eo + eout > a.E) return;
  int64_t* ei0 = o.edge_index;
  int64_t* ei1 = o.edge_index + a.E;
  const int stride = CT * gridDim.y;
  const int t0 = blockIdx.y * CT + threadIdx.x;

  for (int64_t v = t0; v < n; v += stride) {
    const int64_t sv = ns + v, dv = no + v;
    if (!FLT || s.x)
      for (int c = 0; c < s.x_cols; ++c) o.x[dv * s.x_cols + c] = s.x[sv * s.x_cols + c];
    if (o.node_depth) o.node_depth[dv] = s.node_depth[sv];
    o.batch[dv] = i;
    if (aug) {
      const int64_t r = s.attr_rank[sv] - r0;
      if (s.attr_rank[sv + 1] - s.attr_rank[sv] == 1) {
        if (r < m) {  // source of next-token edge r (and destination of its inverse)
          ei0[eo + 2 * e + r] = dv;
          ei1[eo + 2 * e + m + r] = dv;
          *reinterpret_cast<float2*>(o.edge_attr_f32 + (eo + 2 * e + r) * 2) = make_float2(1.f, 0.f);
          *reinterpret_cast<float2*>(o.edge_attr_f32 + (eo + 2 * e + m + r) * 2) = make_float2(1.f, 1.f);
        }
        if (r > 0) {  // destination of next-token edge r-1
          ei1[eo + 2 * e + r - 1] = dv;
          ei0[eo + 2 * e + m + r - 1] = dv;
        }
      }
    }
  }
  for (int64_t k = t0; k < e; k += stride) {
    const int64_t u = s.edge_src[es + k] + no, v = s.edge_dst[es + k] + no;
    ei0[eo + k] = u;
    ei1[eo + k] = v;
    if (aug) {
      ei0[eo + e + k] = v;
      ei1[eo + e + k] = u;
      *reinterpret_cast<float2*>(o.edge_attr_f32 + (eo + k) * 2) = make_float2(0.f, 0.f);
      *reinterpret_cast<float2*>(o.edge_attr_f32 + (eo + e + k) * 2) = make_float2(0.f, 1.f);
    } else if (o.edge_attr_i64) {
      for (int c = 0; c < s.ea_cols; ++c) o.edge_attr_i64[(eo + k) * s.ea_cols + c] = s.edge_attr[(es + k) * s.ea_cols + c];
    }
  }
  if (FLT) {
    if (s.x_f32) copy_run_f32(s.x_f32 + ns * s.x_cols, o.x_f32 + no * s.x_cols, n * s.x_cols, t0, stride);
    if (s.edge_attr_f32 && o.edge_attr_f32)
      copy_run_f32(s.edge_attr_f32 + es * s.ea_cols, o.edge_attr_f32 + eo * s.ea_cols, e * s.ea_cols, t0, stride);
  }
  if (o.y && blockIdx.y == 0) {
    const int64_t words = s.y_row_bytes / 4;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(static_cast<const char*>(s.y) + g * s.y_row_bytes);
    uint32_t* dst = reinterpret_cast<uint32_t*>(static_cast<char*>(o.y) + i * s.y_row_bytes);
    for (int64_t k = threadIdx.x; k < words; k += CT) dst[k] = src[k];
  }
}

// ---- in-degree of every store node over the edges gt_collate emits: one block per stored graph ---------
// A graph's edges name only its own nodes, so the block clears its slice of `deg`, then counts into it.
__global__ void __launch_bounds__(CT) k_store_in_degree(gt_graph_store s, int32_t* __restrict__ deg) {
  const int64_t g = blockIdx.x;
  const int64_t ns = s.node_ptr[g], n = s.node_ptr[g + 1] - ns;
  const int64_t es = s.edge_ptr[g], e = s.edge_ptr[g + 1] - es;
  const bool aug = s.attr_rank != nullptr;
  for (int64_t v = threadIdx.x; v < n; v += CT) deg[ns + v] = 0;
  __threadfence();
  __syncthreads();
  for (int64_t k = threadIdx.x; k < e; k += CT) {
    const int64_t u = s.edge_src[es + k], v = s.edge_dst[es + k];
    if ((uint64_t)v < (uint64_t)n) atomicAdd(&deg[ns + v], 1);          // stored edge u -> v
    if (aug && (uint64_t)u < (uint64_t)n) atomicAdd(&deg[ns + u], 1);   // its inverse v -> u
  }
  if (aug) {
    const int64_t r0 = s.attr_rank[ns];
    const int64_t cnt = s.attr_rank[ns + n] - r0;
    const int64_t m = cnt > 1 ? cnt - 1 : 0;
    for (int64_t v = threadIdx.x; v < n; v += CT) {
      const int64_t sv = ns + v;
      if (s.attr_rank[sv + 1] - s.attr_rank[sv] == 1) {
        const int64_t r = s.attr_rank[sv] - r0;
        const int add = (r > 0 ? 1 : 0) + (r < m ? 1 : 0);   // destination of next-token edge r-1, of the inverse of edge r
        if (add) atomicAdd(&deg[sv], add);
      }
    }
  }
}

// ---- histogram of `deg` over the nodes of the selected graphs: per-block bins in LDS, 64-bit flush ------
__global__ void __launch_bounds__(CT) k_degree_histogram(const int64_t* __restrict__ node_ptr, const int32_t* __restrict__ deg,
                                                         const int64_t* __restrict__ ids, int64_t B, int64_t G, int bins,
                                                         unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned long long lbin[];   // bins + 1 slots; slot `bins` = every degree >= bins
  for (int k = threadIdx.x; k <= bins; k += CT) lbin[k] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
    const int64_t g = ids ? ids[i] : i;
    if ((uint64_t)g >= (uint64_t)G) continue;   // (the caller checks its ids; never read outside the store)
    const int64_t ns = node_ptr[g], n = node_ptr[g + 1] - ns;
    for (int64_t v = threadIdx.x; v < n; v += CT) {
      const int32_t d = deg[ns + v];
      atomicAdd(&lbin[(d < 0 || d > bins) ? bins : d], 1ull);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= bins; k += CT)
    if (lbin[k]) atomicAdd(&hist[k], lbin[k]);
}

constexpr int HIST_MAX_BINS = 8191;   // (bins + 1) 64-bit counters in the 64 KiB of LDS a block gets by default

}  // namespace

extern "C" int gt_attr_rank(const int64_t* node_is_attributed, int64_t num_nodes, int64_t* rank, gt_stream_t stream) {
  GT_CHECK_ARG(num_nodes >= 0 && rank && (node_is_attributed || num_nodes == 0), "bad arguments");
  hipLaunchKernelGGL(k_attr_rank, dim3(1), dim3(SCAN_T), 0, (hipStream_t)stream, node_is_attributed, num_nodes, rank);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" size_t gt_collate_workspace_bytes(int64_t num_graphs) { return (size_t)(2 * (num_graphs + 1)) * sizeof(int64_t); }

extern "C" int gt_collate(const gt_graph_store* store, const int64_t* graph_ids, int64_t num_graphs, int64_t num_nodes,
                          int64_t num_edges, const gt_collate_out* out, void* workspace, size_t workspace_bytes,
                          gt_stream_t stream) {
  GT_CHECK_ARG(store && out, "null descriptor");
  GT_CHECK_ARG(num_graphs >= 0 && num_nodes >= 0 && num_edges >= 0, "negative size");
  if (num_graphs == 0) return GT_OK;
  GT_CHECK_ARG(store->node_ptr && store->edge_ptr && store->x_cols > 0, "store needs node_ptr, edge_ptr, x_cols");
  GT_CHECK_ARG((store->x != nullptr) != (store->x_f32 != nullptr), "store needs exactly one of x / x_f32");
  GT_CHECK_ARG(store->edge_src && store->edge_dst, "store needs edge_src / edge_dst");
  GT_CHECK_ARG(store->x ? (out->x && !out->x_f32) : (out->x_f32 && !out->x), "out->x / out->x_f32 must match the store's x type");
  GT_CHECK_ARG(out->batch && (out->edge_index || num_edges == 0), "out needs batch, edge_index");
  GT_CHECK_ARG(!(store->edge_attr && store->edge_attr_f32), "store holds at most one of edge_attr / edge_attr_f32");
  GT_CHECK_ARG(!(store->attr_rank && store->edge_attr_f32), "an augmenting store writes its own edge_attr_f32: none may be stored");
  GT_CHECK_ARG(store->attr_rank || !out->edge_attr_f32 || (store->edge_attr_f32 && store->ea_cols > 0), "edge_attr_f32 requested but not stored");
  GT_CHECK_ARG(!out->node_depth || store->node_depth, "node_depth requested but not stored");
  GT_CHECK_ARG(!store->attr_rank || out->edge_attr_f32 || num_edges == 0, "augmentation writes edge_attr_f32");
  GT_CHECK_ARG(store->attr_rank || !out->edge_attr_i64 || (store->edge_attr && store->ea_cols > 0), "edge_attr requested but not stored");
  GT_CHECK_ARG(!out->y || (store->y && store->y_row_bytes > 0 && store->y_row_bytes % 4 == 0), "y rows must be stored, multiple of 4 bytes");
  GT_CHECK_ARG(workspace_bytes >= gt_collate_workspace_bytes(num_graphs) && (workspace || num_graphs == 0), "workspace too small");
  GT_CHECK_ARG(graph_ids, "null graph_ids");
  CollateArgs a;
  a.s = *store;
  a.o = *out;
  a.ids = graph_ids;
  a.B = num_graphs;
  a.N = num_nodes;
  a.E = num_edges;
  a.node_off = static_cast<int64_t*>(workspace);
  a.edge_off = a.node_off + num_graphs + 1;
  hipLaunchKernelGGL(k_collate_offsets, dim3(1), dim3(SCAN_T), 0, (hipStream_t)stream, a);
  GT_CHECK_LAUNCH();
  // enough blocks to fill 256 CUs several times over when the batch is small
  int y = (int)(2048 / num_graphs);
  y = y < 1 ? 1 : (y > 8 ? 8 : y);
  if (store->x_f32 || store->edge_attr_f32)
    hipLaunchKernelGGL(k_collate_fill<true>, dim3((unsigned)num_graphs, y), dim3(CT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_collate_fill<false>, dim3((unsigned)num_graphs, y), dim3(CT), 0, (hipStream_t)stream, a);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_store_in_degree(const gt_graph_store* store, int32_t* deg, gt_stream_t stream) {
  GT_CHECK_ARG(store && store->num_graphs >= 0, "null descriptor");
  if (store->num_graphs == 0) return GT_OK;
  GT_CHECK_ARG(store->num_graphs <= INT32_MAX, "more than 2^31 - 1 graphs");
  GT_CHECK_ARG(store->node_ptr && store->edge_ptr && store->edge_src && store->edge_dst && deg, "store needs node_ptr, edge_ptr, edge_src / edge_dst; deg");
  hipLaunchKernelGGL(k_store_in_degree, dim3((unsigned)store->num_graphs), dim3(CT), 0, (hipStream_t)stream, *store, deg);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_degree_histogram(const gt_graph_store* store, const int32_t* deg, const int64_t* graph_ids, int64_t num_graphs,
                                   int64_t bins, int64_t* hist, gt_stream_t stream) {
  GT_CHECK_ARG(store && hist && num_graphs >= 0 && bins >= 1, "bad arguments");
  if (bins > HIST_MAX_BINS) {
    gt_set_error("%s: bins (%lld) above %d: the per-block counters must fit the block's LDS", __func__, (long long)bins, HIST_MAX_BINS);
    return GT_ERR_UNSUPPORTED;
  }
  GT_CHECK_ARG(graph_ids || num_graphs <= store->num_graphs, "without graph_ids the selection is graphs 0 .. num_graphs - 1 of the store");
  (void)hipMemsetAsync(hist, 0, (size_t)(bins + 1) * sizeof(int64_t), (hipStream_t)stream);
  if (num_graphs == 0) return GT_OK;
  GT_CHECK_ARG(store->node_ptr && deg, "store needs node_ptr; deg from gt_store_in_degree");
  const unsigned blocks = (unsigned)(num_graphs < 1024 ? num_graphs : 1024);
  hipLaunchKernelGGL(k_degree_histogram, dim3(blocks), dim3(CT), (size_t)(bins + 1) * sizeof(unsigned long long), (hipStream_t)stream,
                     store->node_ptr, deg, graph_ids, num_graphs, store->num_graphs, (int)bins, reinterpret_cast<unsigned long long*>(hist));
  GT_CHECK_LAUNCH();
  return GT_OK;
}
