// adj_mask.hip — the attention mask of the masked encoder as keep-bits, built on the device from the batch's edges.
//
// Reference semantics being replaced (paths inside the reference project):
//   data/adj_list.py                    make_adj_list: per graph a dense (n, n) array, adj[row, col] = 1 for every edge, + np.eye(n)
//   models/gnn_transformer.py:104-107   padded_adj_list[b, 0:n, 0:n] = adj (TOP-LEFT placement in a (B, T, T) fp32 tensor)
//   modules/masked_transformer_encoder.py:44-47   masked_fill(attn_mask == 0, -1e6), then masked_fill(valid_input_mask == 0, -1e6)
// Here the same predicate is ONE bit per (graph, query, key): bits[B][T][W] uint32, W = ceil(T / 32), key k = bit k & 31 of word
// k >> 5, 1 = keep.  bits[b][q][k] is set exactly when q < n_b, k < n_b, the batch has an edge (graph_ptr[b] + q) -> (graph_ptr[b] + k)
// (or self_loops and q == k) and key_valid[b][k] != 0 when that pointer is given.  Rows q >= n_b and bits k >= T are zero.
//
// A block owns the 64 query rows [tile * 64, tile * 64 + 64) of one graph.  It first packs what every row of the graph shares --
// "k < min(n_b, T) and key_valid[b][k] != 0" -- into LDS words by wave ballot, then every group of G lanes (G = the power of two
// >= W, between 4 and 64) owns whole rows: a lane walks out_dst[out_ptr[v] .. out_ptr[v+1]) of its row's node (the CSC by source of
// gt_graph_prep), ORs the keys of its word in a register and stores the word.  No atomics, no dependence on the order of the edges.
#include "gt_common.h"

namespace {

constexpr int ADJ_THREADS = 256;
constexpr int ADJ_ROWS = 64;         // query rows per block: 16 per wave
constexpr int ADJ_MAX_WORDS = 1024;  // W <= 1024 (T <= 32768): the shared key words of a graph stay in 4 KiB of LDS

__global__ void __launch_bounds__(ADJ_THREADS) k_adj_mask_bits(const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ out_ptr,
                                                              const int32_t* __restrict__ out_dst, int64_t N, int64_t E, int T, int W,
                                                              int tiles, int G, const float* __restrict__ key_valid, int self_loops,
                                                              uint32_t* __restrict__ bits) {
  __shared__ uint32_t sKey[ADJ_MAX_WORDS];
  const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t gp = graph_ptr[b];
  int64_t nb = (int64_t)graph_ptr[b + 1] - gp;
  if (gp < 0 || nb < 0 || gp + nb > N) nb = 0;   // (a graph_ptr that is no prefix sum of this batch: nothing is kept)
  const int lim = (int)(nb < T ? nb : T);        // keys and queries of the graph that have a position
  // ---- the words every row of the graph shares: bit k = (k < lim && key_valid[b][k] != 0), 64 keys per ballot
  for (int c = wid; c * 64 < W * 32; c += ADJ_THREADS / 64) {
    const int k = c * 64 + lane;
    bool keep = k < lim;
    if (keep && key_valid) keep = key_valid[(int64_t)b * T + k] != 0.f;
    const uint64_t m = __ballot(keep);
    if (lane == 0) {
      sKey[2 * c] = (uint32_t)m;
      if (2 * c + 1 < W) sKey[2 * c + 1] = (uint32_t)(m >> 32);
    }
  }
  __syncthreads();
  // ---- rows: 64 / G rows per wave and pass, the wave's 16 rows in 16 * G / 64 passes
  const int rows_per_pass = 64 / G;
  const int sub = lane / G, w0 = lane % G;
  for (int r = sub; r < ADJ_ROWS / 4; r += rows_per_pass) {
    const int q = tile * ADJ_ROWS + wid * (ADJ_ROWS / 4) + r;
    if (q >= T) break;
    int e0 = 0, e1 = 0;
    if (q < lim) {
      e0 = out_ptr[gp + q];
      e1 = out_ptr[gp + q + 1];
      if (e0 < 0) e0 = 0;
      if (e1 > E) e1 = (int)E;
    }
    uint32_t* row = bits + ((int64_t)b * T + q) * W;
    for (int w = w0; w < W; w += G) {   // (more than one word per lane only when W > 64)
      uint32_t word = 0;
      for (int e = e0; e < e1; ++e) {
        const int64_t k = (int64_t)out_dst[e] - gp;
        if (k >= 0 && k < lim && (int)(k >> 5) == w) word |= 1u << (k & 31);
      }
      if (self_loops && q < lim && (q >> 5) == w) word |= 1u << (q & 31);
      row[w] = word & sKey[w];
    }
  }
}

}  // namespace

extern "C" int gt_adj_mask_bits(const int32_t* graph_ptr, const int32_t* out_ptr, const int32_t* out_dst, int64_t N, int64_t E,
                                int64_t B, int64_t T, const float* key_valid, int self_loops, uint32_t* bits, gt_stream_t stream_) {
  GT_CHECK_ARG(N >= 0 && E >= 0 && B >= 0 && T >= 0, "negative size");
  GT_CHECK_ARG(N < (1ll << 31) && E < (1ll << 31), "N and E must fit int32");
  if (B == 0 || T == 0) return GT_OK;
  GT_CHECK_ARG(graph_ptr && out_ptr && bits, "null buffer");
  GT_CHECK_ARG(E == 0 || out_dst, "null edge buffer");
  const int64_t W = gt_cdiv(T, 32);
  if (W > ADJ_MAX_WORDS) {
    gt_set_error("gt_adj_mask_bits: T %lld unsupported (at most %d keys)", (long long)T, ADJ_MAX_WORDS * 32);
    return GT_ERR_UNSUPPORTED;
  }
  const int64_t tiles = gt_cdiv(T, ADJ_ROWS);
  GT_CHECK_ARG(B * tiles < (1ll << 31), "too many row tiles");
  int G = 4;
  while (G < W && G < 64) G <<= 1;
  hipLaunchKernelGGL(k_adj_mask_bits, dim3((unsigned)(B * tiles)), dim3(ADJ_THREADS), 0, (hipStream_t)stream_, graph_ptr, out_ptr,
                     out_dst, N, E, (int)T, (int)W, (int)tiles, G, key_valid, self_loops, bits);
  GT_CHECK_LAUNCH();
  return GT_OK;
}
