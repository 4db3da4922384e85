// model.hip — whole-model driver: ONE C call per direction (gt_model_forward / gt_model_backward).
//
// The reference's training step is `pred = model(batch); loss = calc_loss(pred, batch); loss.backward()`
// (trainers/base_trainer.py:29-36) over GNNTransformer.forward (models/gnn_transformer.py:90-128): node encoder ->
// L x {virtual-node add, conv, BatchNorm, ReLU, dropout, virtual-node update} (modules/gnn_module.py:60-107, :172-241) ->
// JK -> gnn2transformer -> pad + CLS + norm_input -> encoder layers -> final norm (modules/transformer_encoder.py:42-61) ->
// pooling -> heads.  Rounds 1-3 sequenced the composites of layers.hip from Python (~60 ctypes calls, descriptor refresh,
// arena book-keeping: 2.3 ms of interpreter time per Code2 step against ~1 ms of launches).  Here the same calls are issued
// from C in the same order on the same three streams; the caller supplies one arena per direction.
// Pure host code + nothing allocated or synchronised: every buffer is the caller's.
// Three modes share the code: the token path above, the read-out mode (gt_model::readout: message passing -> pooling -> heads, the GNN /
// PNA baselines) and the encoder-only mode (gt_model::enc_only: no message passing, the input encoder's rows are the token rows, the
// Transformer baseline of models/transformer.py:87-101) -- forward_enc_only_tokens + forward_encoder, Bwd::encoder / input_encoder.
//
// gt_model_prepare DECIDES: every question about which kernel or which stream a step takes is asked there, once, with the weight
// images bound, and the answers are stored in the context (Decisions); the arenas are sized beside them.  gt_model_forward and
// gt_model_backward REPLAY the stored answers and ask nothing again: an option or a threshold that changes between a forward and
// its backward cannot make the two halves of one step disagree about a buffer's shape.
#include <algorithm>
#include <cstring>

#include "host_seq.h"
#include "linear_call.h"
#include "seq_layout_host.h"

namespace {

constexpr int MAXL = GT_MODEL_MAX_LAYERS;
constexpr int MAXT = GT_MODEL_MAX_TABLES;
constexpr int64_t PREP_MIN_EDGES = 400000;   // gt_graph_prep beside the first kernels only for batches this large (see prepare_decisions)
constexpr uint64_t SEED_STEP = 0x9E3779B97F4A7C15ULL;   // graphtrans_amd/modules/gnn_module.py:layer_seed / vn_seed
inline uint64_t step_seed(uint64_t base, int k) { return base + SEED_STEP * (uint64_t)k; }
inline float train_p(const gt_model_batch* b, float p) { return b->training ? p : 0.f; }   // dropout only in training

struct Bump {
  size_t off = 0;
  size_t take(size_t bytes) {
    size_t o = off;
    off = (o + bytes + 255) / 256 * 256;
    return o;
  }
};
inline size_t c4(size_t n) { return (n + 3) / 4 * 4; }

// the graph structure of one batch: the caller's arrays, or what gt_graph_prep writes into the forward arena
struct Graph {
  const int32_t *graph_ptr, *node_graph, *in_ptr, *in_src, *in_eid, *out_ptr, *out_dst, *out_eid;
  const float *deg, *dis;
};

// the path decisions of one step: written by prepare_decisions, only read afterwards
struct Decisions {
  int use_prep;      // gt_graph_prep and the encoder's weight images on the prep stream
  int late_wait;     // GCN layer 0 waits for the structure between its GEMM and its aggregate (else: the main stream, before the layers)
  int cat2;          // JK = "cat" without its copy: gnn2transformer reads h_list[0] | h_list[-1] as two operands
  int fuse_rows;     // gnn2transformer's epilogue writes the token rows itself (row map)
  int fuse_nin;      // ... and norm_input in the same epilogue
  int want_wt;       // transposed weights for the backward's exact-fp32 dX GEMMs, written beside the forward
  int esort;         // node ids per table row for the embedding backward, sorted beside the forward
  int fuse_bn;       // BatchNorm-backward statistics summed in the dX epilogue of the layer above ...
  int bn_rows;       // ... as this many partial rows (the count travels with every call that writes or reads them)
  int bc[MAXL];      // layer l's dX epilogue adds the virtual-node update's gradient per graph (no N x D broadcast pass)
  int ov;            // the weight-gradient GEMMs run on the overlap stream
};

// ---- per-forward context (host memory of the caller, opaque to it) -----------------------------------------------------------
struct Ctx {
  uint32_t magic;
  int prepared, forwarded, stages_done;
  gt_model_batch in;
  int64_t rows, max_npos, num_work;
  int exact, lay_host;                 // lay_host: the layout was built into a staging slot by gt_model_prepare
  int compute, tdt;
  size_t tsz;
  int build_graph, build_layout_dev;
  Decisions k;
  // staging slot of the host-built layout
  void* stage_ptr;
  void* stage_event;
  SeqBlob lay;   // the layout blob's offsets (host-built and device-built alike)
  // batch descriptors (one conv kind per model: see the conv_* functions)
  union {
    gt_gcn_layer gcn[MAXL];
    gt_gin_layer gin[MAXL];
    gt_pna_layer pna[MAXL];
  };
  gt_vn_update vn[MAXL];
  gt_encoder_layer enc[MAXL];
  // forward arena
  size_t o_rowmap;   // int32 [N]: the token row of every node (gt_seq_token_rows), when gnn2transformer writes the token rows itself
  size_t o_pos;      // int32 [N]: the padded position of every node (gt_seq_positions), when the model has a positional encoding (gt_model::pe)
  int64_t S_host;    // min(max nodes per graph, max_input_len) where the host knows it (else read on the device: meta[3] of the layout)
  size_t o_h[MAXL + 1], o_x0, o_vn[MAXL], o_vn_saved[MAXL], o_conv_saved[MAXL], o_cat, o_hn, o_tok, o_xin, o_st0, o_xe[MAXL],
      o_enc_saved[MAXL], o_hgin, o_sto, o_eplan, o_esort_ws, o_ne_x, o_ne_w, o_hg, o_ws, o_ws2, o_wt[MAXL], o_g2t_wt;
  size_t o_scales, q_dimg;
  size_t o_hid, o_hid2;   // gt_model::head_kind: the saved hidden activations (1: a1 [B][h1], a2 [B][h2]; 2: the stacked hidden rows [B][pos * D])
  size_t o_arg, o_pool_ws, pool_ws_bytes;   // read-out mode: the max's winning rows [B][D] int32, gt_graph_pool_fwd's workspace (o_hg: the pooled rows [B][D])
  size_t o_graph_ptr, o_node_graph, o_in_ptr, o_out_ptr, o_idx, o_dd, o_status, o_prep_ws, o_lay, o_lay_meta;
  size_t ws_bytes, ws2_bytes, eplan_bytes, esort_ws_bytes, prep_ws_bytes, arena_bytes;
  int64_t Kc;
  char* base;
  // resolved pointers
  Graph g;
  const int32_t *seq_desc, *work_items;
  const int64_t* last_rows;
  const void *xptr[MAXL], *enc_in[MAXL], *pre_out, *first, *node_rep, *h_last;
  const float *g2t_wt, *ne_x, *ne_w;
  int T;
  const int64_t* e_idx[MAXT + 1];
  int64_t e_str[MAXT + 1], e_clamp[MAXT + 1], e_rows[MAXT + 1];
  // backward arena
  size_t q_d_hgin, q_dyp;
  size_t q_defer, defer_bytes, defer_small;   // defer_small: only partial buffers up to this size join the section (0 = all)   // the arena of the backward's deferred partial-sum reduces (gt_defer_begin)
  size_t q_d_hg, q_dtok[2], q_d_hn, q_d_cls, q_d_rep, q_dA, q_dB, q_dC, q_dJ, q_dvn[4], q_ne_dw, q_bnpart[MAXL], q_heads_ws,
      q_ws[2], q_ws2, q_ws3, q_d_hid;
  size_t bws_bytes, heads_ws_bytes, seg_ws_bytes, barena_bytes;
  // what one backward stage leaves for the next (the stages may come as separate calls)
  char* bb;
  int slot;
  void *dy, *d_h0;
};
constexpr uint32_t CTX_MAGIC = 0x67744d31u;

int model_check(const char* fn, const gt_model* m) {
  if (!m) { gt_set_error("%s: null model", fn); return GT_ERR_INVALID_ARG; }
  // (n_enc == 0 is legal in the reference's GNNTransformer -- it pools the token rows themselves -- but not built here: the callers route it
  // to the module path.  The read-out mode -- the GNN baseline, gt_model::readout -- has no encoder at all: there n_enc == 0 is required)
  if (m->enc_only) {   // the encoder-only mode (the Transformer baseline): checked here on its own, every other model exactly as below
    if (m->L != 0 || m->n_enc < 1 || m->n_enc > MAXL || !m->with_cls || m->readout || m->jk_cat || m->has_vn || m->pe || m->head_kind) {
      gt_set_error("%s: the encoder-only mode takes L == 0, 1..%d encoder layers, a CLS row, no read-out, JK = last, no virtual node, no "
                   "positional encoding and the linear heads", fn, MAXL);
      return GT_ERR_INVALID_ARG;
    }
    if (!m->enc || !m->cls || !m->head_w || !m->head_b) { gt_set_error("%s: null descriptor array", fn); return GT_ERR_INVALID_ARG; }
    if (m->d <= 0 || m->d % 8 || m->D != m->d) { gt_set_error("%s: bad widths (the encoder-only mode has D == d)", fn); return GT_ERR_INVALID_ARG; }
    const bool lin = m->embed_kind == 1;
    if (lin ? (!m->ne_w || !m->ne_b || m->ne_K < 1) : (m->n_tables < 1 || m->n_tables > MAXT || !m->embed_sorted)) {
      gt_set_error("%s: the encoder-only mode takes a Linear input encoder with its bias, or 1..%d tables the sorted backward covers", fn, MAXT);
      return GT_ERR_INVALID_ARG;
    }
    return GT_OK;
  }
  const bool ro = m->readout != 0;
  if (m->L < 1 || m->L > MAXL || (ro ? m->n_enc != 0 : (m->n_enc < 1 || m->n_enc > MAXL)) || m->n_tables < 0 || m->n_tables > MAXT) {
    gt_set_error("%s: layer / table counts out of range", fn);
    return GT_ERR_INVALID_ARG;
  }
  // (the read-out mode takes every conv kind: the PNA stack under its own conditions, checked below)
  if (ro && ((m->readout != GT_POOL_SUM && m->readout != GT_POOL_MEAN && m->readout != GT_POOL_MAX) || m->jk_cat || m->pe)) {
    gt_set_error("%s: the read-out mode takes a GT_POOL_* kind, JK = last and no positional encoding", fn);
    return GT_ERR_INVALID_ARG;
  }
  if (m->head_kind) {   // the PNA baseline's heads (csrc/mlp_heads.hip): their shape limits are asked here, once
    const bool mlp = m->head_kind == 1 && m->head_h1 >= 1 && m->head_h1 <= 64 && m->head_h2 >= 1 && m->head_h2 <= 64 && m->D <= 1024 &&
                     m->hid2_w && m->hid2_b && m->off_hid2_w >= 0 && m->off_hid2_b >= 0;
    const bool pos = m->head_kind == 2 && m->head_pos >= 1 && m->head_pos <= 16 && m->Nh % m->head_pos == 0 && m->D % 16 == 0 && m->D <= 512;
    if (!ro || !(mlp || pos) || !m->hid_w || !m->hid_b || m->off_hid_w < 0 || m->off_hid_b < 0) {
      gt_set_error("%s: head kind %d needs the read-out mode, its hidden layers and widths within the head kernels' limits", fn, m->head_kind);
      return GT_ERR_INVALID_ARG;
    }
  }
  if (!m->conv_layers || (m->n_enc && !m->enc) || (m->has_vn && m->L > 1 && !m->vn)) { gt_set_error("%s: null descriptor array", fn); return GT_ERR_INVALID_ARG; }
  if (m->D <= 0 || m->D % 4 || (!ro && (m->d <= 0 || m->d % 8))) { gt_set_error("%s: bad widths", fn); return GT_ERR_INVALID_ARG; }
  if (m->conv != GT_CONV_GCN && m->conv != GT_CONV_GIN && m->conv != GT_CONV_PNA) { gt_set_error("%s: bad conv kind", fn); return GT_ERR_INVALID_ARG; }
  // every position is < S <= max_input_len: a table of at least that many rows needs no clamp in the kernels
  if (m->pe && (m->pe_rows < m->max_input_len || ((uintptr_t)m->pe & 15))) {
    gt_set_error("%s: the positional-encoding table needs max_input_len rows and 16-byte alignment", fn);
    return GT_ERR_INVALID_ARG;
  }
  if (m->conv == GT_CONV_PNA && (m->has_vn || m->jk_cat || !m->residual || !m->pna_src || !m->pna_img || !m->pna_map || !m->pna_inv)) {
    gt_set_error("%s: the PNA stack runs without a virtual node, with JK = last, the residual connection and its weight images", fn);
    return GT_ERR_INVALID_ARG;
  }
  return GT_OK;
}

int bind_images(const gt_model* m, const Ctx* c) {
  if (c->in.use_w3) {
    const gt_image_set& s = c->in.use_w3 == 2 ? m->w3_enc : m->w3;
    if (s.n_bind > 0) GT_TRY(gt_w3_bind(s.n_bind, s.bind_w, s.bind_N, s.bind_K, s.bind_f, s.bind_t));
  }
  if (c->in.use_w1 && m->w1.n_bind > 0)
    GT_TRY(gt_w1_bind(m->w1.n_bind, m->w1.bind_w, m->w1.bind_N, m->w1.bind_K, m->w1.bind_f, m->w1.bind_t));
  return GT_OK;
}
struct BindGuard {   // the bind tables are per host thread: always undone on the way out
  bool dw = false;
  bool defer_abort = false;   // an error return must not leave the deferred-reduce section open on this thread (its arena dies with the step)
  ~BindGuard() {
    gt_w3_unbind();
    gt_w1_unbind();
    if (dw) gt_overlap_dw_end();
    if (defer_abort) (void)gt_defer_begin(nullptr, 0);
  }
};

// ---- the conv kind: the three-way choice between GCN, GIN and PNA lives in these functions (what ONLY the PNA stack has -- its image
// gather, degree scalers, image gradients -- is asked where it runs) ---------------------------------------------------------------
// layer l's descriptor = the model's static part + this batch's sizes, mode and seeds
void conv_init(const gt_model* m, const gt_model_batch* b, Ctx* c, int l) {
  const int training = b->training ? 1 : 0;
  const float p = train_p(b, b->gnn_p);
  const uint64_t seed = step_seed(b->gnn_seed, 2 * l + 1);
  auto with_vn = [&](auto& g) {   // what the GCN and the GIN descriptor share (the fields carry the same names)
    g.N = b->N; g.E = b->E; g.B = b->B;
    g.has_vn = m->has_vn; g.relu = l != m->L - 1; g.residual = m->residual;
    g.training = training; g.compute = c->compute;
    g.dropout_p = p; g.seed = seed;
    g.edge_attr = (g.edge_mode != GT_EDGE_NONE && b->E > 0) ? b->edge_attr : nullptr;
    g.ev_x_ready = nullptr;
    g.ev_dx_wait = (m->st_vn && m->has_vn && l < m->L - 1) ? m->ev_extra[l] : nullptr;
    g.x_has_vn = m->has_vn;
    g.vn_next = nullptr; g.ev_vn_next = nullptr;
  };
  if (m->conv == GT_CONV_GCN) {
    gt_gcn_layer& g = c->gcn[l];
    g = ((const gt_gcn_layer*)m->conv_layers)[l];
    with_vn(g);
    g.lin_wt = nullptr;
    g.prev_saved = nullptr; g.prev_bn_w = g.prev_bn_b = nullptr; g.prev_bn_part = nullptr; g.bn_part_in = nullptr;
    g.prev_relu = 0; g.bn_nparts_in = g.prev_bn_nparts = 0; g.ev_graph_ready = nullptr;
    g.dx_bcast = nullptr; g.dx_bcast_idx = nullptr;
  } else if (m->conv == GT_CONV_GIN) {
    gt_gin_layer& g = c->gin[l];
    g = ((const gt_gin_layer*)m->conv_layers)[l];
    with_vn(g);
    g.w1_t = g.w2_t = nullptr;
  } else {
    gt_pna_layer& g = c->pna[l];
    g = ((const gt_pna_layer*)m->conv_layers)[l];
    g.N = b->N; g.E = b->E;
    g.training = training; g.compute = c->compute;
    g.dropout_p = p; g.seed = seed;
  }
}
size_t conv_saved_bytes(const gt_model* m, const Ctx* c, int l) {
  if (m->conv == GT_CONV_PNA) return gt_pna_layer_saved_bytes(&c->pna[l]);
  return m->conv == GT_CONV_GIN ? gt_gin_layer_saved_bytes(&c->gin[l]) : gt_gcn_layer_saved_bytes(&c->gcn[l]);
}
size_t conv_ws_bytes(const gt_model* m, const Ctx* c, int l) {
  if (m->conv == GT_CONV_PNA) return gt_pna_layer_workspace_bytes(&c->pna[l]);
  return m->conv == GT_CONV_GIN ? gt_gin_layer_workspace_bytes(&c->gin[l]) : gt_gcn_layer_workspace_bytes(&c->gcn[l]);
}
// the D x D weight GEMMs of a layer whose transposes / deferred partials the driver makes room for (the PNA towers reduce on the spot)
int conv_gemms(const gt_model* m) { return m->conv == GT_CONV_GIN ? 2 : (m->conv == GT_CONV_GCN ? 1 : 0); }
// the structure's arrays (and, PNA, the degree scalers `scales`) into layer l's descriptor; ev_graph: see Decisions::late_wait
void conv_set_graph(const gt_model* m, Ctx* c, int l, const float* scales, void* ev_graph) {
  const Graph& s = c->g;
  auto csr = [&](auto& g) {   // every conv descriptor
    g.in_ptr = s.in_ptr; g.in_src = s.in_src; g.in_eid = s.in_eid; g.out_ptr = s.out_ptr; g.out_dst = s.out_dst; g.out_eid = s.out_eid;
  };
  if (m->conv == GT_CONV_GCN) {
    gt_gcn_layer& g = c->gcn[l];
    csr(g);
    g.graph_ptr = s.graph_ptr; g.node_graph = s.node_graph; g.deg = s.deg; g.dis = s.dis;
    g.ev_graph_ready = (l == 0 && c->k.late_wait) ? ev_graph : nullptr;
  } else if (m->conv == GT_CONV_GIN) {
    gt_gin_layer& g = c->gin[l];
    csr(g);
    g.graph_ptr = s.graph_ptr; g.node_graph = s.node_graph;
  } else {
    csr(c->pna[l]);
    c->pna[l].scales = scales;
  }
}
// layer l's weights transposed into wt (Decisions::want_wt: never PNA), for the backward's exact-fp32 dX GEMMs
int conv_transpose(const gt_model* m, Ctx* c, int l, float* wt, gt_stream_t st) {
  const int64_t D = m->D;
  if (m->conv == GT_CONV_GIN) {
    gt_gin_layer& g = c->gin[l];
    g.w1_t = wt; g.w2_t = wt + 2 * D * D;
    GT_TRY(gt_transpose(g.w1, wt, 2 * D, D, st));
    return gt_transpose(g.w2, wt + 2 * D * D, D, 2 * D, st);
  }
  c->gcn[l].lin_wt = wt;
  return gt_transpose(c->gcn[l].lin_w, wt, D, D, st);
}
void conv_set_vn_next(const gt_model* m, Ctx* c, int l, const void* vn_next, void* ev_next) {   // (a virtual node: never PNA)
  if (m->conv == GT_CONV_GIN) { c->gin[l].vn_next = vn_next; c->gin[l].ev_vn_next = ev_next; }
  else { c->gcn[l].vn_next = vn_next; c->gcn[l].ev_vn_next = ev_next; }
}
int conv_fwd(const gt_model* m, Ctx* c, int l, const void* h_in, const void* vn, void* y, gt_stream_t st) {
  void *saved = c->base + c->o_conv_saved[l], *ws = c->base + c->o_ws;
  if (m->conv == GT_CONV_PNA) return gt_pna_layer_fwd(&c->pna[l], h_in, y, saved, ws, c->ws_bytes, st);
  if (m->conv == GT_CONV_GIN) return gt_gin_layer_fwd(&c->gin[l], h_in, vn, nullptr, y, saved, ws, c->ws_bytes, st);
  return gt_gcn_layer_fwd(&c->gcn[l], h_in, vn, nullptr, y, saved, ws, c->ws_bytes, st);
}
// dt0: Decisions::bc (GCN only); dimg: the PNA towers' image gradients
int conv_bwd(const gt_model* m, Ctx* c, int l, const void* dy, const void* extra, const float* dt0, float* dimg, void* out, void* d_vn,
             float* grads, void* ws, gt_stream_t st) {
  const void* saved = c->base + c->o_conv_saved[l];
  if (m->conv == GT_CONV_PNA) {
    gt_pna_layer& g = c->pna[l];
    g.d_pre_w = dimg + m->pna_img_off[l][0]; g.d_pre_b = dimg + m->pna_img_off[l][1];
    g.d_post_w = dimg + m->pna_img_off[l][2]; g.d_post_b = dimg + m->pna_img_off[l][3];
    return gt_pna_layer_bwd(&g, c->xptr[l], dy, saved, out, grads, ws, c->bws_bytes, st);
  }
  if (m->conv == GT_CONV_GIN) return gt_gin_layer_bwd(&c->gin[l], c->xptr[l], dy, extra, saved, out, d_vn, grads, ws, c->bws_bytes, st);
  c->gcn[l].dx_bcast = dt0;   // (requested inside the layer, right in front of its one dX GEMM)
  c->gcn[l].dx_bcast_idx = dt0 ? c->g.node_graph : nullptr;
  return gt_gcn_layer_bwd(&c->gcn[l], c->xptr[l], dy, extra, saved, out, d_vn, grads, ws, c->bws_bytes, st);
}

// ---- gnn2transformer: the one place that writes its call records -----------------------------------------------------------------
// row operand: node_rep [N][Kc], or (Decisions::cat2) h_list[0] | h_list[-1] side by side, D columns each
LinFwd g2t_fwd(const gt_model* m, const Ctx* c, int y_dtype, void* y, const LinRowMap& map, gt_stream_t st) {
  const int64_t D = m->D, ldx = c->k.cat2 ? D : c->Kc;
  LinFwd f{GT_F32, y_dtype, c->compute, c->k.cat2 ? c->first : c->node_rep, m->g2t_w, m->g2t_b, y, c->in.N, m->d, c->Kc, ldx, m->d,
           1, 0, 0, 0, 0.f, 0, (hipStream_t)st};
  if (c->k.cat2) { f.x2 = c->h_last; f.x_split = D; f.ldx2 = D; }
  f.map = map;
  return f;
}
// frozen: weight / bias gradient only (the dW-only form of the same call: same row map, same operands), nothing reads a d node_rep;
// cat2: d h_list[0] -> dJ, d h_list[-1] -> dA straight from the GEMM; else d node_rep -> d_rep (W^T from the forward when it made one)
LinBwd g2t_bwd(const gt_model* m, const Ctx* c, bool frozen, const void* d_hn, const int32_t* rmap, float* G, void* ws, gt_stream_t st) {
  const int64_t D = m->D, ldx = c->k.cat2 ? D : c->Kc;
  char* bb = c->bb;
  void* dx = frozen ? nullptr : bb + (c->k.cat2 ? c->q_dJ : c->q_d_rep);
  LinBwd r{GT_F32, c->tdt, c->compute, c->k.cat2 ? c->first : c->node_rep, m->g2t_w, d_hn, nullptr, nullptr, nullptr, dx, G + m->off_g2t_w,
           G + m->off_g2t_b, c->in.N, m->d, c->Kc, ldx, m->d, 1, 0, 0, 0.f, ws, c->bws_bytes, (hipStream_t)st};
  if (c->k.cat2) { r.x2 = c->h_last; r.dx2 = frozen ? nullptr : bb + c->q_dA; r.x_split = D; r.ldx2 = D; }
  else if (!frozen) r.weight_t = c->g2t_wt;
  r.map.rows = rmap;
  return r;
}

// =================================================================================================================================
// gt_model_prepare, section by section
// ---- the token layout of one forward: the caller's, built on the host into a staging slot of the caller's ring (seq_layout_host.h), or
// built on the device by gt_model_forward (only upper bounds are known here)
int prepare_layout(const gt_model* m, const gt_model_batch* b, Ctx* c) {
  const int64_t N = b->N, B = b->B;
  const int cls = m->with_cls ? 1 : 0;
  if (b->seq_desc) {
    c->rows = b->rows; c->max_npos = b->max_npos; c->num_work = b->num_work; c->exact = b->lay_exact;
    c->S_host = b->lay_S;
    GT_CHECK_ARG(!m->pe || b->lay_meta || b->lay_S > 0, "a caller's token layout needs its S (lay_S or lay_meta) for the positional encoding");
  } else if (b->sizes_host) {
    const SeqHostLayout h = seq_layout_rank(GT_SEQ_PACKED, b->sizes_host, B, m->max_input_len, cls);
    c->rows = h.rows; c->max_npos = h.max_npos; c->num_work = h.num_work; c->exact = 1;
    c->lay_host = 1;
    c->S_host = h.S;
    c->lay = h.blob;
    GT_CHECK_ARG(b->ring, "host-built layout needs a staging ring");
    GT_TRY(gt_stage_ring_take(b->ring, h.blob.bytes, &c->stage_ptr, &c->stage_event));
    seq_layout_fill(h, (char*)c->stage_ptr);
  } else {   // sizes unknown on the host: gt_seq_layout_packed on the device, upper bounds here
    c->build_layout_dev = 1;
    c->rows = N + B * cls;
    c->max_npos = std::min<int64_t>(m->max_input_len, N) + cls;
    c->num_work = B + c->rows / 64;
    c->exact = 0;
    c->lay = seq_blob(B, std::max<int64_t>(c->num_work, 1));
  }
  return GT_OK;
}

// ---- batch descriptors: the model's static descriptors + this batch
void prepare_descriptors(const gt_model* m, const gt_model_batch* b, Ctx* c) {
  const int training = b->training ? 1 : 0;
  for (int l = 0; l < m->L; ++l) conv_init(m, b, c, l);
  for (int l = 0; l < (m->has_vn ? m->L - 1 : 0); ++l) {
    gt_vn_update& v = c->vn[l];
    v = m->vn[l];
    v.N = b->N; v.B = b->B;
    v.residual = m->residual; v.training = training; v.compute = c->compute;
    v.dropout_p = train_p(b, b->gnn_p);
    v.seed = step_seed(b->gnn_seed, 2 * l + 2);
    v.identity_graph = b->ident_B;
    v.ev_dx_done = (m->st_vn && m->vn_defer_dw) ? m->ev_extra[l] : nullptr;
  }
  for (int i = 0; i < m->n_enc; ++i) {
    gt_encoder_layer& e = c->enc[i];
    e = m->enc[i];
    e.rows = c->rows;
    e.dtype = c->tdt; e.compute = c->compute; e.training = training;
    e.num_seqs = b->B; e.row_stride = 1; e.max_npos = c->max_npos;
    e.num_work = c->num_work;
    e.dropout_p = train_p(b, b->enc_p);
    e.seed = step_seed(b->enc_seed, i + 1);
  }
  c->T = m->embed_kind != 1 ? m->n_tables : 0;
  for (int t = 0; t < c->T; ++t) c->e_rows[t] = m->table_rows[t];
  c->Kc = m->jk_cat ? 2 * m->D : m->D;
}

// ---- decisions: every question is asked here, once, with the weight images bound the way the forward and the backward bind them
int prepare_decisions(const gt_model* m, const gt_model_batch* b, Ctx* c) {
  const int64_t N = b->N, D = m->D, d = m->d;
  const int L = m->L;
  const bool frozen = b->gnn_frozen != 0, gcn = m->conv == GT_CONV_GCN;
  Decisions& k = c->k;
  if (m->enc_only) {
    // the encoder-only mode asks nothing of a GEMM: the table encoders always write the token rows through the row map
    // (gt_embed_tokens_fwd), the Linear encoder always goes through [N][d] rows and the gather -- its weight, re-pitched into the arena
    // at every forward (K % 4 != 0: the 37 TU features), can never have a bound image, which the row-map GEMM needs
    k.fuse_rows = m->embed_kind != 1 ? 1 : 0;
    k.esort = (b->will_bwd && m->embed_kind != 1) ? 1 : 0;   // the sort plan IS the table backward's input here (model_check: embed_sorted)
    k.ov = (m->st_dw && N * D >= m->dw_overlap_min_elems) ? 1 : 0;
    return GT_OK;
  }
  BindGuard guard;   // (thread-local bind tables: bound for the questions)
  GT_TRY(bind_images(m, c));
  // the prep stream pays for its stream switches and events (~0.4 ms of host time per step) only when the structure kernels are long:
  // measured r4, Code2 / Molpcba / PNA (E <= 1e5): same step time with and without, host 0.15-0.4 ms cheaper without; the
  // Erdos-Renyi stress (E = 1.05 M): 1 % faster with
  k.use_prep = (m->st_prep && b->sizes_host && c->build_graph && b->E >= PREP_MIN_EDGES) ? 1 : 0;
  // the structure may still be in the making on the prep stream: GCN layer 0 waits between its GEMM and its aggregate,
  // the virtual-node stream before its first segment sum; every other configuration before the layers
  k.late_wait = (k.use_prep && gcn && (!m->has_vn || m->vn0_in_embed)) ? 1 : 0;
  // JK = "cat" without its copy needs the bound image of gnn2transformer's weight
  k.cat2 = (m->jk_cat && b->use_w3 && gt_linear_cat2_ok(c->compute, m->g2t_w, N, d, D, D)) ? 1 : 0;
  // gnn2transformer's epilogue writes the token rows itself (row map; CLS rows by the map's kernel) when the layout is the packed one
  // built here and the bf16x6 kernel runs it: no pad pass over the node rows (modules/utils.py:5-29), no [N][d] intermediate
  k.fuse_rows = (!m->readout && !b->seq_desc && gt_linear_rows_ok(c->compute, GT_F32, c->tdt, m->g2t_w, N, d, c->Kc)) ? 1 : 0;
  // ... and norm_input (transformer_encoder.py:53-57) in the same epilogue when a token row fills one column block of the kernel
  k.fuse_nin = (k.fuse_rows && m->nin_w && gt_linear_rows_layernorm_ok(d)) ? 1 : 0;
  // (a frozen message-passing stack has no embedding backward, and no dX GEMM below gnn2transformer's weight gradient: neither the node ids
  // per table row nor the transposed weights are made)
  k.esort = (b->will_bwd && !frozen && m->embed_sorted && m->embed_kind != 1) ? 1 : 0;
  const bool have_imgs = b->use_w3 != 0;
  k.want_wt = (m->conv != GT_CONV_PNA && b->will_bwd && !frozen && gt_compute_base(c->compute) == GT_F32 && N >= 1024 && (!have_imgs || (!m->has_vn && gcn))) ? 1 : 0;
  // BatchNorm-backward statistics summed in the dX epilogue of the layer above (GCN, exact-fp32 GEMMs, no GNN dropout, no virtual node)
  // (not beyond 64 k rows: the statistics ride in the EXACT-fp32 dX kernel -- at the Erdos-Renyi stress' 131 k x 256 x 256 that GEMM is
  // 219 us against 116 us for the bf16x6 kernel + a 50-us partial pass: 17.6 k -> 17.9 k graphs/s without)
  if (L > 1 && !frozen && !b->sync_bn && gcn && b->training && c->gcn[0].dropout_p == 0.f && gt_linear_bwd_bnstats_ok(c->compute, GT_F32, GT_F32, N)) {
    // which kernel will run the layers' dX GEMMs: the register-row bf16x6 kernel (bound images, N >= 12288: one partial row per 128
    // rows, any N, with or without a virtual node -- its epilogue holds the complete d x_l, virtual-node rows included) or the
    // exact-fp32 one (64-row tiles; without a virtual node and up to 64 k rows only, see above)
    const int64_t exact_rows = gt_linear_bwd_bnstats_rows(N);
    const int64_t rows = b->use_w3 ? gt_linear_bwd_bnstats_rows_for(c->compute, GT_F32, GT_F32, c->gcn[1].lin_w, N, D, D) : exact_rows;
    // (the register-row kernel answers only with gt_option_set("bnstats_rows_kernel", 1) -- measured r5, Code2 b256: statistics in its epilogue 74.0 k graphs/s,
    // the separate partial pass 74.85 k; ER 19.07 k against 19.14 k: the epilogue's second row read + 320 lane shuffles per wave
    // cost more than the 23-us pass they replace)
    if (rows > 0 && (rows != exact_rows || (!m->has_vn && N <= 65536))) {
      k.fuse_bn = 1;
      k.bn_rows = (int)rows;
    }
  }
  // the virtual-node update's gradient per GRAPH, added per node in layer l's dX epilogue: only the register-row kernel does that
  for (int l = 0; l + 1 < L; ++l)
    k.bc[l] = (m->has_vn && !frozen && gcn && gt_linear_bwd_bcast_ok(c->compute, GT_F32, GT_F32, c->gcn[l].lin_w, N, D, D)) ? 1 : 0;
  // the overlap stream pays for itself only when the kernels are long enough to hide its extra stream operations
  k.ov = (m->st_dw && N * D >= m->dw_overlap_min_elems) ? 1 : 0;
  return GT_OK;
}

void prepare_forward_arena(const gt_model* m, const gt_model_batch* b, Ctx* c) {
  const int64_t N = b->N, E = b->E, B = b->B, D = m->D, d = m->d, rows = c->rows, Kc = c->Kc;
  const int L = m->L, nenc = m->n_enc, nvn = m->has_vn ? L - 1 : 0;
  const size_t tsz = c->tsz, ND4 = (size_t)N * D * 4;
  Bump a;
  const bool eo = m->enc_only != 0;   // no node-row matrices: the token rows are the input encoder's output
  for (int l = 0; l <= L; ++l) c->o_h[l] = a.take(eo ? 0 : ND4);
  if (m->has_vn) {
    c->o_x0 = a.take(m->vn0_in_embed ? 0 : ND4);
    for (int l = 0; l < L; ++l) c->o_vn[l] = a.take((size_t)B * D * 4);
    for (int l = 0; l < nvn; ++l) c->o_vn_saved[l] = a.take(gt_vn_update_saved_bytes(&c->vn[l]));
  }
  for (int l = 0; l < L; ++l) c->o_conv_saved[l] = a.take(conv_saved_bytes(m, c, l));
  c->o_cat = a.take((m->jk_cat && !c->k.cat2) ? (size_t)N * Kc * 4 : 0);
  const bool ro = m->readout != 0;   // no gnn2transformer, no token rows, no encoder: their slots are empty
  // (fp32 under a positional encoding: its add comes before the one rounding; encoder-only mode: the Linear encoder's rows, no table's)
  c->o_hn = a.take((ro || (eo && m->embed_kind != 1)) ? 0 : (size_t)N * d * (m->pe ? 4 : tsz));
  c->o_rowmap = a.take(ro ? 0 : (size_t)N * 4);
  c->o_pos = a.take(m->pe ? (size_t)N * 4 : 0);
  c->o_tok = a.take(ro ? 0 : (size_t)rows * d * tsz);
  if (m->nin_w) {
    c->o_xin = a.take((size_t)rows * d * tsz);
    c->o_st0 = a.take((size_t)2 * rows * 4);
  }
  // the LAST encoder layer is the pooled variant (gt_encoder_layer_pooled_*): cls / last pooling reads one row per sequence of it
  for (int i = 0; i < nenc; ++i) c->o_xe[i] = a.take((size_t)(i == nenc - 1 ? B : rows) * d * tsz);
  for (int i = 0; i < nenc; ++i)
    c->o_enc_saved[i] = a.take(i == nenc - 1 ? gt_encoder_layer_pooled_saved_bytes(&c->enc[i]) : gt_encoder_layer_saved_bytes(&c->enc[i]));
  if (m->nout_w) {   // the final norm runs on the POOLED rows only (cls / last pooling reads nothing else of it: gnn_transformer.py:113-114)
    c->o_hgin = a.take((size_t)B * d * 4);
    c->o_sto = a.take((size_t)2 * B * 4);
  }
  if (c->k.esort) {
    c->eplan_bytes = gt_embed_sort_plan_bytes(c->T, c->e_rows, N);
    c->esort_ws_bytes = gt_embed_sort_workspace_bytes(c->T, c->e_rows, N);
    c->o_eplan = a.take(c->eplan_bytes);
    c->o_esort_ws = a.take(c->esort_ws_bytes);
  }
  const int64_t Kp = (int64_t)c4((size_t)m->ne_K);
  if (m->embed_kind == 1 && Kp != m->ne_K) {
    c->o_ne_x = a.take((size_t)N * Kp * 4);
    c->o_ne_w = a.take((size_t)D * Kp * 4);
  }
  c->o_hg = a.take((size_t)B * (ro ? D : d) * 4);
  if (ro) {
    c->o_arg = a.take(m->readout == GT_POOL_MAX ? (size_t)B * D * 4 : 0);
    c->pool_ws_bytes = gt_graph_pool_workspace_bytes(m->readout, N, D);
    c->o_pool_ws = a.take(c->pool_ws_bytes);
    if (m->head_kind == 1) {
      c->o_hid = a.take((size_t)B * m->head_h1 * 4);
      c->o_hid2 = a.take((size_t)B * m->head_h2 * 4);
    } else if (m->head_kind == 2) {
      c->o_hid = a.take((size_t)B * m->head_pos * D * 4);
    }
  }
  if (m->conv == GT_CONV_PNA) c->o_scales = a.take((size_t)N * c->pna[0].S * 4);
  size_t ws = 256, ws2 = 256;
  for (int l = 0; l < L; ++l) ws = std::max(ws, conv_ws_bytes(m, c, l));
  for (int l = 0; l < nvn; ++l) ws2 = std::max(ws2, gt_vn_update_workspace_bytes(&c->vn[l]));
  ws = std::max(ws, ws2);
  c->ws_bytes = ws; c->ws2_bytes = ws2;
  c->o_ws = a.take(ws);
  c->o_ws2 = a.take(ws2);
  if (c->k.want_wt) {
    for (int l = 0; l < L; ++l) c->o_wt[l] = a.take((size_t)conv_gemms(m) * 2 * D * D * 4);
    c->o_g2t_wt = a.take(ro ? 0 : (size_t)d * Kc * 4);
  }
  if (c->build_graph) {
    c->o_graph_ptr = a.take((size_t)(B + 1) * 4);
    c->o_node_graph = a.take((size_t)N * 4);
    c->o_in_ptr = a.take((size_t)(N + 1) * 4);
    c->o_out_ptr = a.take((size_t)(N + 1) * 4);
    c->o_idx = a.take((size_t)4 * std::max<int64_t>(E, 1) * 4);
    c->o_dd = a.take((size_t)2 * N * 4);
    c->o_status = a.take(4);
    c->prep_ws_bytes = gt_graph_prep_workspace_bytes(N, E, B);
    c->o_prep_ws = a.take(c->prep_ws_bytes);
  }
  if (c->lay_host || c->build_layout_dev) c->o_lay = a.take(c->lay.bytes);
  if (c->build_layout_dev) c->o_lay_meta = a.take(16);
  c->arena_bytes = std::max(a.off, (size_t)256);
}

void prepare_backward_arena(const gt_model* m, const gt_model_batch* b, Ctx* c) {
  const int64_t N = b->N, B = b->B, D = m->D, d = m->d, rows = c->rows, Kc = c->Kc;
  const int L = m->L, nenc = m->n_enc;
  const size_t tsz = c->tsz, ND4 = (size_t)N * D * 4;
  const bool eo = m->enc_only != 0;
  const bool frozen = b->gnn_frozen != 0 || eo;   // (encoder-only mode: no message passing either, its slots are as empty as a frozen stack's)
  const bool ro = m->readout != 0;   // heads on the pooled rows [B][D]; the pooling's backward writes d h_list[-1] into q_d_rep
  const int64_t hk = ro ? D : d;     // the heads' input width
  Bump q;
  c->q_d_hg = q.take((size_t)B * hk * 4);
  c->q_d_hgin = q.take((m->nout_w && !ro) ? (size_t)B * d * 4 : 0);
  c->q_dyp = q.take(ro ? 0 : (size_t)B * d * tsz);
  c->q_dtok[0] = q.take(ro ? 0 : (size_t)rows * d * tsz);
  c->q_dtok[1] = q.take(ro ? 0 : (size_t)rows * d * tsz);
  c->q_d_hn = q.take((ro || (eo && m->embed_kind != 1)) ? 0 : (size_t)N * d * tsz);
  c->q_d_cls = q.take((ro || eo) ? 0 : (size_t)B * d * tsz);
  // (frozen message-passing stack: the node-row and virtual-node gradients are never made, their slots are empty)
  c->q_d_rep = q.take(frozen ? 0 : (size_t)N * Kc * 4);
  c->q_dA = q.take(frozen ? 0 : ND4); c->q_dB = q.take(frozen ? 0 : ND4); c->q_dC = q.take(frozen ? 0 : ND4);
  c->q_dJ = q.take((m->jk_cat && !frozen) ? ND4 : 0);
  for (int i = 0; i < 4; ++i) c->q_dvn[i] = q.take(frozen ? 0 : (size_t)B * D * 4);
  size_t enc_ws = 256;
  for (int i = 0; i < nenc; ++i)
    enc_ws = std::max(enc_ws, i == nenc - 1 ? gt_encoder_layer_pooled_workspace_bytes(&c->enc[i]) : gt_encoder_layer_workspace_bytes(&c->enc[i]));
  const size_t ln_ws = ro ? 0 : std::max(gt_layernorm_bwd_workspace_bytes(rows, d), gt_layernorm_bwd_workspace_bytes(B, d));
  size_t lin_ws = std::max(gt_linear_bwd_workspace_bytes(c->compute, B, m->Nh, hk), ro ? (size_t)0 : gt_linear_bwd_workspace_bytes(c->compute, N, d, Kc));
  if (m->head_kind == 2) lin_ws = std::max(lin_ws, gt_linear_bwd_workspace_bytes(c->compute, B, m->head_pos * D, D));   // the stacked hidden layers
  const int64_t Kp = (int64_t)c4((size_t)m->ne_K);
  size_t emb_ws;
  if (m->embed_kind == 1) {
    emb_ws = gt_linear_bwd_workspace_bytes(c->compute, N, D, Kp);
    c->q_ne_dw = q.take((Kp != m->ne_K && (!frozen || eo)) ? (size_t)D * Kp * 4 : 0);
  } else if (c->k.esort) {
    emb_ws = gt_embed_sum_bwd_sorted_workspace_bytes(c->T, N, D);
  } else {
    emb_ws = gt_embed_sum_bwd_workspace_bytes(c->T, c->e_rows, D);
  }
  c->bws_bytes = std::max(std::max(std::max(c->ws_bytes, enc_ws), std::max(ln_ws, lin_ws)), emb_ws);
  for (int l = 0; l + 1 < L; ++l) c->q_bnpart[l] = q.take(c->k.fuse_bn ? (size_t)c->k.bn_rows * 2 * D * 4 : 0);
  c->heads_ws_bytes = m->head_kind == 1   ? gt_head_mlp_workspace_bytes(B, m->head_h1, m->head_h2)
                      : m->head_kind == 2 ? gt_head_group_workspace_bytes(B, m->head_pos, D, m->Nh / m->head_pos)
                                          : gt_linear_bwd_workspace_bytes(c->compute, B, m->Nh, hk);
  c->q_heads_ws = q.take(c->heads_ws_bytes);
  c->q_d_hid = q.take(m->head_kind == 2 ? (size_t)B * m->head_pos * D * 4 : 0);
  c->q_ws[0] = q.take(c->bws_bytes);
  c->q_ws[1] = q.take(c->bws_bytes);
  c->q_ws2 = q.take(c->ws2_bytes);
  c->seg_ws_bytes = (m->has_vn && !frozen) ? gt_segment_sum_workspace_bytes(N, D) : 0;
  c->q_ws3 = q.take(c->seg_ws_bytes);
  c->q_dimg = q.take((m->conv == GT_CONV_PNA && !frozen) ? (size_t)m->pna_n_img * 4 : 0);
  // the sums over weight-gradient / LayerNorm partials of a stage are queued by their producers and run as ONE launch at the end of
  // the stage: room for every weight-gradient GEMM's partials and every LayerNorm's block partials of one backward (an upper bound: a
  // producer that finds the arena full reduces on the spot)
  size_t need = lin_ws + emb_ws + (size_t)(2 * nenc + 2) * ln_ws;
  for (int l = 0; l < L; ++l) need += conv_gemms(m) * conv_ws_bytes(m, c, l);
  for (int i = 0; i < nenc; ++i) {
    const gt_encoder_layer& e = c->enc[i];
    const int ec = e.dtype == GT_BF16 ? GT_BF16 : e.compute;
    need += gt_linear_bwd_workspace_bytes(ec, e.rows, 3 * e.d_model, e.d_model) + gt_linear_bwd_workspace_bytes(ec, e.rows, e.d_model, e.d_model) +
            gt_linear_bwd_workspace_bytes(ec, e.rows, e.ffn, e.d_model) + gt_linear_bwd_workspace_bytes(ec, e.rows, e.d_model, e.ffn);
  }
  // (up to ~6 M node-row elements: where the step is made of launches it gains them -- Molpcba +1 %, NCI1 +2 %, PNA b128 +1.2 % --;
  // at Code2 b256 (9.5 M) the arena copies of the partials are cold memory where the reused workspaces stay in the Infinity Cache:
  // -0.9 %, so the big batches keep the GEMMs' immediate reduces and defer the LayerNorms' column sums only)
  constexpr int64_t defer_max = 6000000;
  c->defer_small = N * D > defer_max && nenc > 0 ? ln_ws : 0;
  c->defer_bytes = N * D <= defer_max ? need + 64 * 256 : (c->defer_small ? (size_t)(2 * nenc + 2) * (ln_ws + 256) + 64 * 256 : 0);
  c->q_defer = q.take(c->defer_bytes);
  c->barena_bytes = std::max(q.off, (size_t)256);
}

// =================================================================================================================================
// gt_model_forward's prologue: who builds the graph structure and the token layout, the weight images, and their pointers into the
// descriptors.  *ev_w1: set when the encoder's weight images are being built on the prep stream
int forward_prologue(const gt_model* m, Ctx* c, gt_stream_t st, void** ev_w1) {
  const gt_model_batch& b = c->in;
  const int64_t N = b.N, E = b.E, B = b.B;
  auto P = [&](size_t off) -> void* { return c->base + off; };
  // ---- graph structure (gt_graph_prep) beside the first kernels, on the prep stream
  gt_stream_t pst = c->k.use_prep ? m->st_prep : st;
  Graph& g = c->g;
  if (c->build_graph) {
    int32_t* idx = (int32_t*)P(c->o_idx);
    const int64_t Ep = std::max<int64_t>(E, 1);
    float* dd = (float*)P(c->o_dd);
    g = Graph{(int32_t*)P(c->o_graph_ptr), (int32_t*)P(c->o_node_graph), (int32_t*)P(c->o_in_ptr), idx, idx + Ep, (int32_t*)P(c->o_out_ptr),
              idx + 2 * Ep, idx + 3 * Ep, dd, dd + N};
    if (c->k.use_prep) {
      GT_TRY(gt_event_record(m->ev_prep_begin, st));
      GT_TRY(gt_stream_wait_event(pst, m->ev_prep_begin));
    }
    GT_TRY(gt_graph_prep(b.edge_index, b.batch, N, E, B, (int32_t*)g.graph_ptr, (int32_t*)g.node_graph, (int32_t*)g.in_ptr, (int32_t*)g.in_src,
                         (int32_t*)g.in_eid, (int32_t*)g.out_ptr, (int32_t*)g.out_dst, (int32_t*)g.out_eid, (float*)g.deg, (float*)g.dis,
                         (int32_t*)P(c->o_status), P(c->o_prep_ws), c->prep_ws_bytes, pst));
    if (c->k.use_prep) GT_TRY(gt_event_record(m->ev_graph, pst));
  } else {
    g = Graph{b.graph_ptr, b.node_graph, b.in_ptr, b.in_src, b.in_eid, b.out_ptr, b.out_dst, b.out_eid, b.deg, b.dis};
  }
  // ---- token layout (none in the read-out mode)
  if (m->readout) {
    c->seq_desc = nullptr; c->last_rows = nullptr; c->work_items = nullptr;
  } else if (b.seq_desc) {
    c->seq_desc = b.seq_desc; c->last_rows = b.last_rows; c->work_items = b.work_items;
  } else {
    char* lay = (char*)P(c->o_lay);
    c->seq_desc = (const int32_t*)lay;
    c->last_rows = (const int64_t*)(lay + c->lay.o_last);
    c->work_items = c->num_work ? (const int32_t*)(lay + c->lay.o_work) : nullptr;
    if (c->lay_host) {
      if (hipMemcpyAsync(lay, c->stage_ptr, c->lay.bytes, hipMemcpyHostToDevice, (hipStream_t)st) != hipSuccess) {
        gt_set_error("gt_model_forward: layout copy failed");
        return GT_ERR_LAUNCH;
      }
      if (c->stage_event) GT_TRY(gt_event_record(c->stage_event, st));
    } else {
      GT_TRY(gt_seq_layout_packed(g.graph_ptr, B, m->max_input_len, m->with_cls ? 1 : 0, (int32_t*)lay, (int64_t*)(lay + c->lay.o_last),
                                  (int32_t*)(lay + c->lay.o_work), c->num_work, (int32_t*)P(c->o_lay_meta), st));
    }
  }
  for (int i = 0; i < m->n_enc; ++i) { c->enc[i].seq_desc = c->seq_desc; c->enc[i].work_items = c->work_items; }
  if (m->conv == GT_CONV_PNA)   // the towers' re-stacked weights (the optimizer changed them: one launch for all layers); their
    GT_TRY(gt_gather_f32(m->pna_img, m->pna_src, m->pna_map, m->pna_n_img, st));   // bf16x3 images are built from these just below
  // ---- weight images (the weights changed since the last step: one launch each)
  if (b.use_w3) {
    const gt_image_set& s = b.use_w3 == 2 ? m->w3_enc : m->w3;
    if (s.n_jobs > 0) GT_TRY(gt_w3_images(s.n_jobs, s.job_w, s.job_N, s.job_K, s.job_T, s.job_img, st));
  }
  if (b.use_w1 && m->w1.n_jobs > 0) {
    GT_TRY(gt_w1_images(m->w1.n_jobs, m->w1.job_w, m->w1.job_N, m->w1.job_K, m->w1.job_T, m->w1.job_img, pst));
    if (c->k.use_prep) {
      GT_TRY(gt_event_record(m->ev_w1, pst));
      *ev_w1 = m->ev_w1;
    }
  }
  // ---- graph pointers into the descriptors
  for (int l = 0; l < m->L; ++l) conv_set_graph(m, c, l, (const float*)P(c->o_scales), m->ev_graph);
  for (int l = 0; l < (m->has_vn ? m->L - 1 : 0); ++l) { c->vn[l].graph_ptr = g.graph_ptr; c->vn[l].node_graph = g.node_graph; }
  return GT_OK;
}

}  // namespace

extern "C" size_t gt_model_ctx_bytes(void) { return sizeof(Ctx); }

extern "C" int gt_model_grad_ranges(const gt_model* m, int64_t* lo3, int64_t* hi3) {
  GT_TRY(model_check("gt_model_grad_ranges", m));
  GT_CHECK_ARG(lo3 && hi3, "null output");
  if (m->enc_only) {   // no message passing: the middle range is empty, the input encoder's block ends where the CLS embedding's begins
    const int64_t t = m->off_cls;
    GT_CHECK_ARG(t >= 0 && t <= m->grad_total, "the encoder-only mode's gradient layout: input encoder, cls_embedding, ...");
    lo3[0] = t; hi3[0] = m->grad_total;
    lo3[1] = t; hi3[1] = t;
    lo3[2] = 0; hi3[2] = t;
    return GT_OK;
  }
  const int64_t gnn_lo = m->has_vn ? m->off_vn_emb : m->off_conv[0];
  // (read-out mode: no gnn2transformer, the heads follow message passing; their hidden layers lead the head block)
  const int64_t tail = m->readout ? (m->head_kind ? m->off_hid_w : m->off_head_w) : m->off_g2t_w;
  lo3[0] = tail;   hi3[0] = m->grad_total;
  lo3[1] = gnn_lo; hi3[1] = tail;
  lo3[2] = 0;            hi3[2] = gnn_lo;
  return GT_OK;
}

// =================================================================================================================================
extern "C" int gt_model_prepare(const gt_model* m, const gt_model_batch* b, void* ctx_, gt_model_sizes* out) {
  GT_TRY(model_check("gt_model_prepare", m));
  GT_CHECK_ARG(b && ctx_ && out, "null argument");
  GT_CHECK_ARG(b->N > 0 && b->B > 0 && b->E >= 0, "empty batch");
  // (encoder-only mode: the batch's edges are not this model's input, `batch` alone builds the structure it reads)
  GT_CHECK_ARG(b->x && (((b->edge_index || m->enc_only) && b->batch) || b->graph_ptr), "null batch arrays");
  if (m->enc_only) {   // refused before anything is launched: these combinations stay on the module path
    GT_CHECK_ARG(!b->gnn_frozen, "the encoder-only mode has no message-passing stack to freeze");
    GT_CHECK_ARG(!(b->perturb && m->embed_kind == 1), "the encoder-only mode takes a perturbation with the table encoders only");
  }
  // the perturbation of forward(batched_data, perturb) and its gradient (gt_model_batch::perturb / d_perturb)
  GT_CHECK_ARG(!(b->perturb && b->gnn_frozen), "perturb with gnn_frozen: a frozen message-passing stack hands out no d perturb");
  GT_CHECK_ARG(!b->d_perturb || (b->perturb && b->will_bwd), "d_perturb without perturb (or without will_bwd)");
  GT_CHECK_ARG(!(((uintptr_t)b->perturb | (uintptr_t)b->d_perturb) & 15), "perturb / d_perturb must be 16-byte aligned");
  Ctx* c = (Ctx*)ctx_;
  memset(c, 0, sizeof(Ctx));
  c->magic = CTX_MAGIC;
  c->in = *b;
  c->compute = b->compute;
  c->tdt = b->tdt;
  c->tsz = gt_elt_bytes(b->tdt);
  c->build_graph = b->graph_ptr == nullptr;
  if (m->enc_only) c->in.E = 0;   // gt_graph_prep at E = 0: graph_ptr / node_graph (all this mode reads), no edge is touched or sorted
  if (m->readout) {   // no token layout (rows = num_work = 0, no staging-ring slot), no encoder weight images
    GT_CHECK_ARG(!b->gnn_frozen, "the read-out mode has no frozen message-passing stack (models/gnn.py has no freeze_gnn)");
    GT_CHECK_ARG(m->head_kind != 2 || b->B <= 4096, "the per-position heads take at most 4096 graphs per batch");
    c->in.use_w3 = b->use_w3 ? 1 : 0;
    c->in.use_w1 = 0;
    c->exact = 1;
  } else {
    GT_TRY(prepare_layout(m, b, c));
  }
  prepare_descriptors(m, &c->in, c);
  GT_TRY(prepare_decisions(m, &c->in, c));
  prepare_forward_arena(m, &c->in, c);
  prepare_backward_arena(m, &c->in, c);
  c->prepared = 1;
  out->rows = c->rows; out->max_npos = c->max_npos; out->num_work = c->num_work;
  out->arena_bytes = (int64_t)c->arena_bytes; out->barena_bytes = (int64_t)c->barena_bytes;
  out->exact = c->exact; out->pad_ = 0;
  return GT_OK;
}

// =================================================================================================================================
namespace {

// the index columns, clamps and tables of a table input encoder (embed_kind 0 / 2) for the embedding kernels
int embed_columns(const gt_model* m, Ctx* c, const float** tabs) {
  const gt_model_batch& b = c->in;
  const int T = c->T;
  const int64_t* x = (const int64_t*)b.x;
  if (m->embed_kind == 2) {   // ASTNodeEncoder: type, attribute, clamped depth
    GT_CHECK_ARG(T == 3 && b.node_depth, "ASTNodeEncoder has three tables and needs node_depth");
    c->e_idx[0] = x; c->e_str[0] = b.x_stride0;
    c->e_idx[1] = x + b.x_stride1; c->e_str[1] = b.x_stride0;
    c->e_idx[2] = b.node_depth; c->e_str[2] = b.depth_stride;
  } else {
    for (int t = 0; t < T; ++t) { c->e_idx[t] = x + (int64_t)t * b.x_stride1; c->e_str[t] = b.x_stride0; }
  }
  for (int t = 0; t < T; ++t) { c->e_clamp[t] = m->table_clamp[t]; tabs[t] = m->tables[t]; }
  return GT_OK;
}

// ---- behind the token rows (c->o_tok; with Decisions::fuse_nin c->o_xin holds norm_input's output already): norm_input, the encoder
// layers with the last one pooled, the final norm on the pooled rows, the heads, and the closing joins of the side streams.  Shared by
// the token path and the encoder-only mode   (modules/transformer_encoder.py:42-61, models/gnn_transformer.py:113-126)
int forward_encoder(const gt_model* m, Ctx* c, float* logits, gt_stream_t st) {
  const gt_model_batch& b = c->in;
  const Decisions& k = c->k;
  const int64_t B = b.B, d = m->d, rows = c->rows;
  const int nenc = m->n_enc, tdt = c->tdt, compute = c->compute;
  auto P = [&](size_t off) -> void* { return c->base + off; };
  const void* cur = P(c->o_tok);
  if (k.fuse_nin) {
    cur = P(c->o_xin);
  } else if (m->nin_w) {
    GT_TRY(gt_layernorm_fwd(tdt, cur, nullptr, m->nin_w, m->nin_b, m->nin_eps, 0.f, 0, rows, d, P(c->o_xin), (float*)P(c->o_st0),
                            (float*)P(c->o_st0) + rows, st));
    cur = P(c->o_xin);
  }
  for (int i = 0; i < nenc; ++i) {
    c->enc_in[i] = cur;
    if (i == nenc - 1) {   // only the pooled row of every sequence is read behind the last layer: y = [B][d]
      GT_TRY(gt_encoder_layer_pooled_fwd(&c->enc[i], cur, c->last_rows, P(c->o_xe[i]), P(c->o_enc_saved[i]), st));
    } else {
      GT_TRY(gt_encoder_layer_fwd(&c->enc[i], cur, P(c->o_xe[i]), P(c->o_enc_saved[i]), st));
    }
    cur = P(c->o_xe[i]);
  }
  c->pre_out = cur;   // [B][d]: the pooled rows
  if (m->nout_w) {
    // transformer.norm (transformer_encoder.py:28-32) is row-wise: on the pooled rows (fp32 copies), forward and backward
    GT_TRY(gt_rows_gather(tdt, cur, nullptr, B, d, (float*)P(c->o_hgin), st));
    GT_TRY(gt_layernorm_fwd(GT_F32, P(c->o_hgin), nullptr, m->nout_w, m->nout_b, m->nout_eps, 0.f, 0, B, d, P(c->o_hg), (float*)P(c->o_sto),
                            (float*)P(c->o_sto) + B, st));
  } else {
    GT_TRY(gt_rows_gather(tdt, cur, nullptr, B, d, (float*)P(c->o_hg), st));
  }
  // ---- prediction heads as one GEMM over the stacked weights   (gnn_transformer.py:120-126)
  GT_TRY(gt_linear_fwd_ld(GT_F32, GT_F32, compute, P(c->o_hg), m->head_w, m->head_b, logits, B, m->Nh, d, m->ldy, 0, 0.f, 0, st));
  // the side streams wrote into this arena: join them before anything can hand it back to the allocator
  if (k.esort && m->st_dw) GT_TRY(gt_stream_wait_event(st, m->ev_sort[1]));
  else if (k.want_wt && m->st_dw) GT_TRY(gt_stream_wait_event(st, m->ev_wt[1]));
  return GT_OK;
}

// ---- the encoder-only mode's token rows (models/transformer.py:87-101: node encoder -> + perturb -> pad + CLS): the table encoders write
// them straight from the tables through the row map, the Linear encoder goes through [N][d] rows of the token type and the gather
int forward_enc_only_tokens(const gt_model* m, Ctx* c, gt_stream_t st) {
  const gt_model_batch& b = c->in;
  const Graph& g = c->g;
  const int64_t N = b.N, B = b.B, d = m->d;
  const int tdt = c->tdt;
  auto P = [&](size_t off) -> void* { return c->base + off; };
  if (m->embed_kind == 1) {   // nn.Linear(F, d) (dataset/tud.py:65) in gnn2transformer's place: x W^T + b, rounded once to the token type
    const int64_t K = m->ne_K, Kp = (int64_t)c4((size_t)K);
    const float *nx = (const float*)b.x, *nw = m->ne_w;
    if (Kp != K) {
      GT_TRY(gt_repitch(P(c->o_ne_x), Kp, b.x, K, N, 4, st));
      GT_TRY(gt_repitch(P(c->o_ne_w), Kp, m->ne_w, K, d, 4, st));
      nx = (const float*)P(c->o_ne_x); nw = (const float*)P(c->o_ne_w);
    }
    c->ne_x = nx; c->ne_w = nw;
    GT_TRY(gt_linear_fwd(GT_F32, tdt, c->compute, nx, nw, m->ne_b, P(c->o_hn), N, d, Kp, 0, 0.f, 0, st));
    return gt_seq_gather_cls32(tdt, P(c->o_hn), m->cls, g.graph_ptr, c->seq_desc, B, 1, c->max_npos, 1, d, P(c->o_tok), st);
  }
  const int T = c->T;
  const float* tabs[MAXT + 1];
  GT_TRY(embed_columns(m, c, tabs));
  int32_t* rmap = (int32_t*)P(c->o_rowmap);
  GT_TRY(gt_seq_token_rows(tdt, m->cls, g.graph_ptr, g.node_graph, c->seq_desc, B, 1, 1, N, d, P(c->o_tok), rmap, st));
  GT_TRY(gt_embed_tokens_fwd(T, c->e_idx, c->e_str, c->e_clamp, tabs, b.perturb, rmap, N, d, tdt, P(c->o_tok), st));
  if (c->k.esort) {   // node ids per table row for the backward: beside the encoder on the overlap stream, only the index columns are read
    gt_stream_t sst = st;
    if (m->st_dw) {
      sst = m->st_dw;
      GT_TRY(gt_event_record(m->ev_sort[0], st));
      GT_TRY(gt_stream_wait_event(sst, m->ev_sort[0]));
    }
    GT_TRY(gt_embed_sort(T, c->e_idx, c->e_str, c->e_clamp, c->e_rows, N, P(c->o_eplan), c->eplan_bytes, P(c->o_esort_ws), c->esort_ws_bytes, sst));
    if (m->st_dw) GT_TRY(gt_event_record(m->ev_sort[1], sst));
  }
  return GT_OK;
}

}  // namespace

// =================================================================================================================================
extern "C" int gt_model_forward(const gt_model* m, void* ctx_, void* arena, float* logits, gt_stream_t st) {
  GT_TRY(model_check("gt_model_forward", m));
  Ctx* c = (Ctx*)ctx_;
  GT_CHECK_ARG(c && c->magic == CTX_MAGIC && c->prepared && !c->forwarded, "context not prepared (or used twice)");
  GT_CHECK_ARG(arena && logits, "null buffer");
  const gt_model_batch& b = c->in;
  const Decisions& k = c->k;
  const int64_t N = b.N, B = b.B, D = m->D, d = m->d, rows = c->rows;
  const int L = m->L, tdt = c->tdt, compute = c->compute, cls = m->with_cls ? 1 : 0;
  c->base = (char*)arena;
  c->forwarded = 1;
  auto P = [&](size_t off) -> void* { return c->base + off; };
  BindGuard guard;
  GT_TRY(bind_images(m, c));
  void* ev_w1 = nullptr;
  GT_TRY(forward_prologue(m, c, st, &ev_w1));
  const Graph& g = c->g;
  if (m->enc_only) {   // no message passing, no gnn2transformer: the input encoder's rows are the token rows
    if (ev_w1) GT_TRY(gt_stream_wait_event(st, ev_w1));
    GT_TRY(forward_enc_only_tokens(m, c, st));
    return forward_encoder(m, c, logits, st);
  }

  gt_stream_t side = m->has_vn ? m->st_vn : nullptr;
  // ---- transposed weights for the backward's exact-fp32 dX GEMMs, written beside the forward
  if (k.want_wt) {
    gt_stream_t tst = st;
    if (m->st_dw) {
      tst = m->st_dw;
      GT_TRY(gt_event_record(m->ev_wt[0], st));
      GT_TRY(gt_stream_wait_event(tst, m->ev_wt[0]));
    }
    for (int l = 0; l < L; ++l) GT_TRY(conv_transpose(m, c, l, (float*)P(c->o_wt[l]), tst));
    if (!m->readout) {
      c->g2t_wt = (float*)P(c->o_g2t_wt);
      GT_TRY(gt_transpose(m->g2t_w, (float*)P(c->o_g2t_wt), d, c->Kc, tst));
    }
    if (m->st_dw) GT_TRY(gt_event_record(m->ev_wt[1], tst));
  }
  // ---- input encoder   (dataset/utils.py:28-30 / ogb AtomEncoder / nn.Linear(F, D) dataset/tud.py:65)
  const int T = c->T;
  if (m->embed_kind == 1) {
    const int64_t K = m->ne_K, Kp = (int64_t)c4((size_t)K);
    const float *nx = (const float*)b.x, *nw = m->ne_w;
    if (Kp != K) {
      GT_TRY(gt_repitch(P(c->o_ne_x), Kp, b.x, K, N, 4, st));
      GT_TRY(gt_repitch(P(c->o_ne_w), Kp, m->ne_w, K, D, 4, st));
      nx = (const float*)P(c->o_ne_x); nw = (const float*)P(c->o_ne_w);
    }
    c->ne_x = nx; c->ne_w = nw;
    GT_TRY(gt_linear_fwd(GT_F32, GT_F32, compute, nx, nw, m->ne_b, P(c->o_h[0]), N, D, Kp, 0, 0.f, 0, st));
    if (b.perturb)   // encoded + perturb (gnn_module.py:158), in place behind the GEMM
      GT_TRY(gt_add3((const float*)P(c->o_h[0]), b.perturb, nullptr, N * D, (float*)P(c->o_h[0]), st));
  } else {
    const float* tabs[MAXT + 1];
    GT_TRY(embed_columns(m, c, tabs));
    int Tn = T;
    if (m->vn0_in_embed) {   // + virtualnode_embedding.weight[0] for every node (gnn_module.py:195,199): one more table, stride-0 index
      c->e_idx[T] = m->zero_i64; c->e_str[T] = 0; c->e_clamp[T] = -1; tabs[T] = m->vn_emb;
      Tn = T + 1;
    }
    // (perturb, when there is one, behind the T node tables and in front of the virtual-node row: the module path's order)
    GT_TRY(gt_embed_sum_fwd_add(Tn, c->e_idx, c->e_str, c->e_clamp, tabs, b.perturb, T, N, D, (float*)P(c->o_h[0]), st));
    if (k.esort) {   // node ids per table row for the backward: beside the forward, only the index columns are read
      gt_stream_t sst = st;
      if (m->st_dw) {
        sst = m->st_dw;
        GT_TRY(gt_event_record(m->ev_sort[0], st));
        GT_TRY(gt_stream_wait_event(sst, m->ev_sort[0]));
      }
      GT_TRY(gt_embed_sort(T, c->e_idx, c->e_str, c->e_clamp, c->e_rows, N, P(c->o_eplan), c->eplan_bytes, P(c->o_esort_ws),
                           c->esort_ws_bytes, sst));
      if (m->st_dw) GT_TRY(gt_event_record(m->ev_sort[1], sst));
    }
  }
  // ---- the structure may still be in the making on the prep stream (Decisions::late_wait)
  if (k.use_prep) {
    if (!k.late_wait) GT_TRY(gt_stream_wait_event(st, m->ev_graph));
    else if (side) GT_TRY(gt_stream_wait_event(side, m->ev_graph));
  }
  // ---- message passing   (modules/gnn_module.py:181-224)
  auto X = [&](int l) -> void* {
    if (!m->has_vn) return P(c->o_h[l]);
    return (l == 0 && !m->vn0_in_embed) ? P(c->o_x0) : P(c->o_h[l]);
  };
  if (m->conv == GT_CONV_PNA)   // per-node degree scalers of this batch (in-degrees: the structure is ready on this stream here)
    GT_TRY(gt_pna_scales(g.in_ptr, N, c->pna[0].S, m->pna_kinds, m->pna_avg_log, m->pna_avg_lin, (float*)P(c->o_scales), st));
  if (m->has_vn)
    GT_TRY(gt_segment_bcast_add(GT_F32, nullptr, m->vn_emb, b.zeros_B, B, 1, D, P(c->o_vn[0]), st));
  for (int l = 0; l < L; ++l) {
    if (m->has_vn) {
      const bool last = l == L - 1;
      conv_set_vn_next(m, c, l, last ? nullptr : P(c->o_vn[l + 1]), (!last && side) ? m->ev_vn[l] : nullptr);
      if (l == 0 && !m->vn0_in_embed)   // Linear node encoder: x_0 = h_0 + vn_0[batch] as its own pass
        GT_TRY(gt_segment_bcast_add(GT_F32, P(c->o_h[0]), P(c->o_vn[0]), g.node_graph, N, B, D, P(c->o_x0), st));
      if (!last && side) {
        // vn_{l+1} beside layer l's GEMM / aggregate on the second stream; layer l's apply pass waits for it (ev_vn_next)
        GT_TRY(gt_event_record(m->ev_x[l], st));
        GT_TRY(gt_stream_wait_event(side, m->ev_x[l]));
        GT_TRY(gt_vn_update_fwd(&c->vn[l], X(l), P(c->o_vn[l]), P(c->o_vn[l + 1]), P(c->o_vn_saved[l]), P(c->o_ws2), c->ws2_bytes, side));
        GT_TRY(gt_event_record(m->ev_vn[l], side));
      } else if (!last) {
        GT_TRY(gt_vn_update_fwd(&c->vn[l], X(l), P(c->o_vn[l]), P(c->o_vn[l + 1]), P(c->o_vn_saved[l]), P(c->o_ws), c->ws_bytes, st));
      }
    }
    GT_TRY(conv_fwd(m, c, l, X(l), m->has_vn ? P(c->o_vn[l]) : nullptr, P(c->o_h[l + 1]), st));
    c->xptr[l] = X(l);
  }
  c->first = X(0);   // h_list[0] after the in-place virtual-node add
  c->h_last = P(c->o_h[L]);
  if (m->readout) {
    // ---- read-out + prediction heads   (models/gnn.py:107-115): the pooled rows [B][D], then one GEMM over the stacked head weights
    GT_TRY(gt_graph_pool_fwd(m->readout, GT_F32, c->h_last, g.graph_ptr, N, B, D, P(c->o_hg), m->readout == GT_POOL_MAX ? (int32_t*)P(c->o_arg) : nullptr,
                             P(c->o_pool_ws), c->pool_ws_bytes, st));
    if (m->head_kind == 1) {   // models/pna.py:53-60, :100: one launch, the two hidden activations saved for the backward
      GT_TRY(gt_head_mlp_fwd(compute, (const float*)P(c->o_hg), D, m->hid_w, m->hid_b, m->hid2_w, m->hid2_b, m->head_w, m->head_b,
                             (float*)P(c->o_hid), (float*)P(c->o_hid2), logits, m->ldy, B, D, m->head_h1, m->head_h2, m->Nh, st));
    } else if (m->head_kind == 2) {   // models/pna.py:62-71, :101-104: the stacked hidden layers with the ReLU epilogue, then the grouped output layer
      const int64_t Lp = m->head_pos;
      GT_TRY(gt_linear_fwd(GT_F32, GT_F32, compute, P(c->o_hg), m->hid_w, m->hid_b, P(c->o_hid), B, Lp * D, D, 1, 0.f, 0, st));
      GT_TRY(gt_head_group_fwd(compute, (const float*)P(c->o_hid), Lp * D, m->head_w, m->head_b, logits, m->ldy, B, Lp, D, m->Nh / Lp, st));
    } else {
      GT_TRY(gt_linear_fwd_ld(GT_F32, GT_F32, compute, P(c->o_hg), m->head_w, m->head_b, logits, B, m->Nh, D, m->ldy, 0, 0.f, 0, st));
    }
    if (k.esort && m->st_dw) GT_TRY(gt_stream_wait_event(st, m->ev_sort[1]));   // the closing join of the side streams, as below
    else if (k.want_wt && m->st_dw) GT_TRY(gt_stream_wait_event(st, m->ev_wt[1]));
    return GT_OK;
  }
  if (ev_w1) GT_TRY(gt_stream_wait_event(st, ev_w1));   // the encoder's weight images were built on the prep stream
  // ---- gnn2transformer + token rows + encoder   (models/gnn_transformer.py:92-114)
  void* g2t_out = P(c->o_hn);
  LinRowMap map{};   // rides, like the second operand, in the GEMM call's record
  // PositionalEncoding (models/gnn_transformer.py:98-100, :149-168: x + pe[:S] on the padded rows, before CLS and norm_input): the
  // row pe[padded position of the node] joins the node's token row where that row is written -- the GEMM's epilogue or the gather
  const int32_t* pos = nullptr;
  if (m->pe) {
    const int32_t* S_dev = c->build_layout_dev ? (const int32_t*)P(c->o_lay_meta) + 3 : ((b.seq_desc && b.lay_meta) ? b.lay_meta + 3 : nullptr);
    GT_TRY(gt_seq_positions(g.graph_ptr, g.node_graph, c->seq_desc, cls, N, c->S_host, S_dev, (int32_t*)P(c->o_pos), st));
    pos = (const int32_t*)P(c->o_pos);
  }
  const int g2t_dt = (m->pe && !k.fuse_rows) ? GT_F32 : tdt;   // (the gather adds in fp32 and rounds once)
  if (k.fuse_rows) {
    int32_t* rmap = (int32_t*)P(c->o_rowmap);
    if (k.fuse_nin) {
      float* st0 = (float*)P(c->o_st0);
      GT_TRY(gt_seq_token_rows_layernorm(tdt, m->cls, g.graph_ptr, g.node_graph, c->seq_desc, B, 1, cls, N, d, P(c->o_tok), rmap, m->nin_w,
                                         m->nin_b, m->nin_eps, P(c->o_xin), st0, st0 + rows, st));
      map = LinRowMap{rmap, m->nin_w, m->nin_b, P(c->o_xin), st0, st0 + rows, m->nin_eps};
    } else {
      GT_TRY(gt_seq_token_rows(tdt, m->cls, g.graph_ptr, g.node_graph, c->seq_desc, B, 1, cls, N, d, P(c->o_tok), rmap, st));
      map.rows = rmap;
    }
    if (m->pe) { map.add_table = m->pe; map.add_idx = pos; map.add_ld = d; }
    g2t_out = P(c->o_tok);
  }
  c->node_rep = k.cat2 ? nullptr : c->h_last;
  if (m->jk_cat && !k.cat2) {   // torch.cat([h_list[0], h_list[-1]], 1)   (gnn_module.py:104-105)
    GT_TRY(gt_copy2d(P(c->o_cat), c->Kc * 4, c->first, D * 4, D * 4, N, st));
    GT_TRY(gt_copy2d((char*)P(c->o_cat) + D * 4, c->Kc * 4, c->h_last, D * 4, D * 4, N, st));
    c->node_rep = P(c->o_cat);
  }
  GT_TRY(lin_fwd(g2t_fwd(m, c, g2t_dt, g2t_out, map, st)));
  if (!k.fuse_rows) {
    if (m->pe)
      GT_TRY(gt_seq_gather_add(tdt, GT_F32, P(c->o_hn), nullptr, m->cls, m->pe, d, pos, g.graph_ptr, c->seq_desc, B, 1, c->max_npos, cls, d,
                               P(c->o_tok), nullptr, st));
    else
      GT_TRY(gt_seq_gather_cls32(tdt, P(c->o_hn), m->cls, g.graph_ptr, c->seq_desc, B, 1, c->max_npos, cls, d, P(c->o_tok), st));
  }
  return forward_encoder(m, c, logits, st);
}

// =================================================================================================================================
namespace {

// what the three stages of one backward share
struct Bwd {
  const gt_model* m;
  Ctx* c;
  float* G;
  gt_stream_t st, side;
  void* P(size_t off) const { return c->base + off; }
  void* Q(size_t off) const { return c->bb + off; }
  // the next call's workspace: the two slots alternate, so the weight-gradient GEMMs a call forks onto the third stream (their
  // partials and the dy they read live in the call's slot) run beside the NEXT one; the main stream waits only for the
  // GEMMs that used this slot two calls ago
  void* W() const {
    c->slot ^= 1;
    void* p = Q(c->q_ws[c->slot]);
    if (c->k.ov) gt_overlap_dw_release(p, c->bws_bytes);
    return p;
  }
  // the sums a stage's producers queued (gt_defer_*), ONE launch.  `behind`: an event of a stream OTHER than the main one whose
  // producers queued partials too (the virtual-node update's weight gradients run on the second stream and the main stream joins
  // that stream only in stage 4)
  int flush(void* behind = nullptr) const {
    gt_stream_t fs = c->k.ov ? gt_overlap_dw_fork(st, 0) : st;   // behind everything queued on the main stream, on the overlap stream
    if (behind) GT_TRY(gt_stream_wait_event(fs, behind));
    GT_TRY(gt_defer_flush(fs));
    if (fs != st) gt_overlap_dw_booked(Q(c->q_defer), c->defer_bytes);
    return GT_OK;
  }
  int encoder(const float* dlogits, bool frozen) const;
  int message_passing() const;
  int input_encoder() const;
};

// ---- stage 1: heads, final norm, encoder layers, token rows -> node rows, gnn2transformer.  Leaves c->dy = d h_list[-1] (null:
// the JK slab is split in stage 2's prologue; frozen: nothing follows)
int Bwd::encoder(const float* dlogits, bool frozen) const {
  const int64_t N = c->in.N, B = c->in.B, d = m->d, rows = c->rows;
  const int nenc = m->n_enc, tdt = c->tdt, compute = c->compute;
  const size_t ws_bytes = c->bws_bytes;
  if (m->readout) {   // heads (dW forked, dX) on the pooled rows [B][D], then the pooling's backward: d h_list[-1] for stage 2
    const int64_t D = m->D;
    if (m->head_kind == 1) {
      GT_TRY(gt_head_mlp_bwd(compute, (const float*)P(c->o_hg), D, m->hid_w, m->hid2_w, m->head_w, (const float*)P(c->o_hid),
                             (const float*)P(c->o_hid2), dlogits, m->ldy, (float*)Q(c->q_d_hg), D, G + m->off_hid_w, G + m->off_hid_b,
                             G + m->off_hid2_w, G + m->off_hid2_b, G + m->off_head_w, G + m->off_head_b, B, D, m->head_h1, m->head_h2, m->Nh,
                             Q(c->q_heads_ws), c->heads_ws_bytes, st));
    } else if (m->head_kind == 2) {   // the output layers gate the hidden rows' gradient themselves (relu_mask): the hidden GEMM gets none
      const int64_t Lp = m->head_pos;
      GT_TRY(gt_head_group_bwd(compute, (const float*)P(c->o_hid), Lp * D, m->head_w, dlogits, m->ldy, 1, (float*)Q(c->q_d_hid), Lp * D,
                               G + m->off_head_w, G + m->off_head_b, B, Lp, D, m->Nh / Lp, Q(c->q_heads_ws), c->heads_ws_bytes, st));
      GT_TRY(gt_linear_bwd(GT_F32, GT_F32, compute, P(c->o_hg), m->hid_w, Q(c->q_d_hid), nullptr, nullptr, nullptr, Q(c->q_d_hg),
                           G + m->off_hid_w, G + m->off_hid_b, B, Lp * D, D, 0.f, W(), ws_bytes, st));
    } else {
      GT_TRY(gt_linear_bwd_dw_forked(GT_F32, GT_F32, compute, P(c->o_hg), m->head_w, dlogits, nullptr, G + m->off_head_w, G + m->off_head_b, B,
                                     m->Nh, D, D, m->ldy, 0.f, Q(c->q_heads_ws), c->heads_ws_bytes, st));
      GT_TRY(gt_linear_bwd_ld(GT_F32, GT_F32, compute, P(c->o_hg), m->head_w, dlogits, nullptr, nullptr, nullptr, Q(c->q_d_hg), nullptr, nullptr,
                              B, m->Nh, D, m->ldy, 0.f, W(), ws_bytes, st));
    }
    GT_TRY(gt_graph_pool_bwd(m->readout, GT_F32, Q(c->q_d_hg), m->readout == GT_POOL_MAX ? (const int32_t*)P(c->o_arg) : nullptr, c->g.graph_ptr,
                             c->g.node_graph, N, B, D, Q(c->q_d_rep), st));
    c->dy = Q(c->q_d_rep);
    return flush();
  }
  // ---- heads: the weight gradient first, forked onto the overlap stream beside the heads' own dX GEMM
  GT_TRY(gt_linear_bwd_dw_forked(GT_F32, GT_F32, compute, P(c->o_hg), m->head_w, dlogits, nullptr, G + m->off_head_w, G + m->off_head_b, B,
                                 m->Nh, d, d, m->ldy, 0.f, Q(c->q_heads_ws), c->heads_ws_bytes, st));
  GT_TRY(gt_linear_bwd_ld(GT_F32, GT_F32, compute, P(c->o_hg), m->head_w, dlogits, nullptr, nullptr, nullptr, Q(c->q_d_hg), nullptr, nullptr,
                          B, m->Nh, d, m->ldy, 0.f, W(), ws_bytes, st));
  // ---- pooled rows -> token rows
  void *dcur = Q(c->q_dtok[0]), *dnext = Q(c->q_dtok[1]);
  const float* d_pool = (const float*)Q(c->q_d_hg);
  if (m->nout_w) {   // the final norm on the pooled rows
    GT_TRY(gt_layernorm_bwd(GT_F32, P(c->o_hgin), nullptr, Q(c->q_d_hg), m->nout_w, (float*)P(c->o_sto), (float*)P(c->o_sto) + B, 0.f, 0, B, d,
                            Q(c->q_d_hgin), nullptr, G + m->off_nout_w, G + m->off_nout_b, W(), ws_bytes, st));
    d_pool = (const float*)Q(c->q_d_hgin);
  }
  GT_TRY(gt_rows_scatter(tdt, d_pool, nullptr, B, B, d, Q(c->q_dyp), st));   // the pooled rows' gradient in the token dtype
  for (int i = nenc - 1; i >= 0; --i) {
    if (i == nenc - 1)
      GT_TRY(gt_encoder_layer_pooled_bwd(&c->enc[i], c->enc_in[i], c->last_rows, Q(c->q_dyp), P(c->o_enc_saved[i]), dnext, G + m->off_enc[i],
                                         W(), ws_bytes, st));
    else
      GT_TRY(gt_encoder_layer_bwd(&c->enc[i], c->enc_in[i], dcur, P(c->o_enc_saved[i]), dnext, G + m->off_enc[i], W(), ws_bytes, st));
    std::swap(dcur, dnext);
  }
  if (m->nin_w) {
    GT_TRY(gt_layernorm_bwd(tdt, P(c->o_tok), nullptr, dcur, m->nin_w, (float*)P(c->o_st0), (float*)P(c->o_st0) + rows, 0.f, 0, rows, d,
                            dnext, nullptr, G + m->off_nin_w, G + m->off_nin_b, W(), ws_bytes, st));
    std::swap(dcur, dnext);
  }
  if (m->enc_only) {   // the cls gradient = column sums of the CLS rows; the token-row gradient stays where it is for stage 4
    GT_TRY(gt_colsum_rows_f32(tdt, dcur, c->last_rows, B, d, G + m->off_cls, st));
    c->dy = dcur;
    return flush();
  }
  // ---- token rows -> node rows (+ the CLS gradient)
  const void* d_hn = Q(c->q_d_hn);
  const int32_t* rmap = nullptr;
  if (c->k.fuse_rows) {   // the GEMMs read the token-row gradient through the row map; the cls gradient = column sums of the CLS rows
    if (m->cls) GT_TRY(gt_colsum_rows_f32(tdt, dcur, c->last_rows, B, d, G + m->off_cls, st));
    rmap = (const int32_t*)P(c->o_rowmap);
    d_hn = dcur;
  } else {
    GT_TRY(gt_seq_scatter(tdt, dcur, nullptr, c->g.graph_ptr, c->g.node_graph, c->seq_desc, B, 1, m->with_cls ? 1 : 0, N, d, Q(c->q_d_hn),
                          m->cls ? Q(c->q_d_cls) : nullptr, st));
    if (m->cls) GT_TRY(gt_colsum_f32(tdt, Q(c->q_d_cls), B, d, G + m->off_cls, st));
  }
  if (c->g2t_wt && m->st_dw) GT_TRY(gt_stream_wait_event(st, m->ev_wt[1]));   // W^T was written on the overlap stream beside the forward
  GT_TRY(lin_bwd(g2t_bwd(m, c, frozen, d_hn, rmap, G, W(), st)));
  c->dy = (frozen || (m->jk_cat && !c->k.cat2)) ? nullptr : Q(c->k.cat2 ? c->q_dA : c->q_d_rep);
  return flush();
}

// ---- stage 2: message passing, last layer first.  Leaves c->d_h0 = d h_list[0]
int Bwd::message_passing() const {
  const gt_model_batch& b = c->in;
  const Decisions& k = c->k;
  const int64_t N = b.N, B = b.B, D = m->D, Kc = c->Kc;
  const int L = m->L;
  const size_t ws_bytes = c->bws_bytes;
  // dy = d h_list[l+1]; "extra" = gradient reaching x_l from its consumers other than conv_l: the JK slab (l = 0) and the
  // virtual-node update's pooling (l < L-1)
  void* dy = c->dy;
  if (!k.cat2 && m->jk_cat) {
    GT_TRY(gt_copy2d(Q(c->q_dA), D * 4, (char*)Q(c->q_d_rep) + D * 4, Kc * 4, D * 4, N, st));   // d h_list[-1]
    GT_TRY(gt_copy2d(Q(c->q_dJ), D * 4, Q(c->q_d_rep), Kc * 4, D * 4, N, st));                   // d h_list[0]
    dy = Q(c->q_dA);
  }
  if (k.fuse_bn) {   // (GCN only) layer l's dX epilogue writes bn_rows partial rows, layer l-1's BatchNorm backward reads as many
    for (int l = 1; l < L; ++l) {
      gt_gcn_layer &up = c->gcn[l], &dn = c->gcn[l - 1];
      up.prev_saved = P(c->o_conv_saved[l - 1]);
      up.prev_bn_w = dn.bn_w; up.prev_bn_b = dn.bn_b; up.prev_relu = dn.relu;
      up.prev_bn_part = (float*)Q(c->q_bnpart[l - 1]);
      dn.bn_part_in = (const float*)Q(c->q_bnpart[l - 1]);
      up.prev_bn_nparts = dn.bn_nparts_in = k.bn_rows;
    }
  }
  void* d_vn_next = nullptr;
  for (int l = L - 1; l >= 0; --l) {
    const void* extra = (l == 0 && m->jk_cat) ? Q(c->q_dJ) : nullptr;
    const bool upd = m->has_vn && l < L - 1;
    void* d_vn_upd = Q(c->q_dvn[2]);   // d vn_l through update l (its pooled + residual inputs)
    const float* dt0 = nullptr;   // the update's gradient per GRAPH, added per node in the dX GEMM's epilogue (no N x D broadcast pass)
    if (upd) {   // vn_{l+1} = update(x_l, vn_l): d x_l = pooled gradient (+ the JK slab at l = 0)
      const bool bc = k.bc[l] != 0;
      void* dxl = bc ? nullptr : Q(c->q_dC);
      if (side) {   // beside layer l's BatchNorm / aggregate backward; joined before its dX GEMM (ev_dx_wait)
        GT_TRY(gt_event_record(m->ev_dvn[l], st));
        GT_TRY(gt_stream_wait_event(side, m->ev_dvn[l]));
        // without a residual branch d vn_l IS d_t0: read where the update's last GEMM wrote it (no copy launch)
        d_vn_upd = m->residual ? Q(c->q_dvn[2]) : (void*)gt_vn_update_bwd_dt0(&c->vn[l], Q(c->q_ws2));
        GT_TRY(gt_vn_update_bwd(&c->vn[l], d_vn_next, P(c->o_vn_saved[l]), extra, dxl, d_vn_upd, G + m->off_vn[l], Q(c->q_ws2),
                                c->ws2_bytes, side));
        if (!m->vn_defer_dw) GT_TRY(gt_event_record(m->ev_extra[l], side));
        if (bc) dt0 = gt_vn_update_bwd_dt0(&c->vn[l], Q(c->q_ws2));
      } else {
        void* vws = W();
        GT_TRY(gt_vn_update_bwd(&c->vn[l], d_vn_next, P(c->o_vn_saved[l]), extra, dxl, Q(c->q_dvn[2]), G + m->off_vn[l], vws, ws_bytes, st));
        if (bc) dt0 = gt_vn_update_bwd_dt0(&c->vn[l], vws);
      }
      if (!bc) extra = Q(c->q_dC);
    }
    void* out = dy == Q(c->q_dA) ? Q(c->q_dB) : Q(c->q_dA);
    // d h_list[0] IS d loss / d perturb: layer 0's input gradient goes straight into the caller's buffer, whichever kernel writes it;
    // the pooling just below and stage 4 (through c->d_h0) read it from there
    if (l == 0 && b.d_perturb) out = b.d_perturb;
    if (l == 0 && k.ov) gt_overlap_dw_urgent(1);   // layer 0's weight gradients are the last: nothing left to overlap them with
    const bool pool_on_side = m->has_vn && side;
    void* d_vn = (m->has_vn && !pool_on_side) ? Q(c->q_dvn[3]) : nullptr;
    GT_TRY(conv_bwd(m, c, l, dy, extra, dt0, (float*)Q(c->q_dimg), out, d_vn, G + m->off_conv[l], W(), st));
    if (m->has_vn) {   // d vn_l = per-graph sum of d x_l (+ update l's pooled + residual inputs): off the main chain
      gt_stream_t vst = pool_on_side ? side : st;
      void* tgt = Q(c->q_dvn[l % 2]);
      if (pool_on_side) {   // the pooled gradient + update l's share in ONE pass (the sum's `add` rows): no bcast_add / copy launch
        GT_TRY(gt_event_record(m->ev_pool[l], st));
        GT_TRY(gt_stream_wait_event(side, m->ev_pool[l]));
        GT_TRY(gt_segment_sum_ws(GT_F32, out, upd ? d_vn_upd : nullptr, c->g.graph_ptr, N, B, D, tgt, Q(c->q_ws3), c->seg_ws_bytes, side));
      } else if (upd) {
        GT_TRY(gt_segment_bcast_add(GT_F32, Q(c->q_dvn[3]), d_vn_upd, b.ident_B, B, B, D, tgt, vst));
      } else {
        GT_TRY(gt_copy2d(tgt, D * 4, Q(c->q_dvn[3]), D * 4, D * 4, B, vst));
      }
      d_vn_next = tgt;
    }
    dy = out;
  }
  c->d_h0 = dy;
  if (m->conv == GT_CONV_PNA) {   // image gradients -> the tower parameters' gradients (every source element sits in the images at most once)
    if (k.ov) gt_overlap_dw_sync();
    GT_TRY(gt_gather_f32(G + m->off_pna_src, (const float*)Q(c->q_dimg), m->pna_inv, m->pna_n_src, st));
  }
  if (m->has_vn) {
    gt_stream_t vst = side ? side : st;
    GT_TRY(gt_segment_sum(GT_F32, d_vn_next, nullptr, b.ptr01, B, 1, D, G + m->off_vn_emb, vst));
    if (side) GT_TRY(gt_event_record(m->ev_vnemb, side));
  }
  // the virtual-node updates' weight-gradient GEMMs queued their partials from the second stream: the sum runs behind its tail
  return flush((m->has_vn && side) ? m->ev_vnemb : nullptr);
}

// ---- stage 4: the input encoder's gradients from c->d_h0, and the closing joins
int Bwd::input_encoder() const {
  const int64_t N = c->in.N, D = m->D;
  const size_t ws_bytes = c->bws_bytes;
  void* d_h0 = c->d_h0;
  int dy_dt = GT_F32;
  if (m->enc_only && m->embed_kind == 1) {
    // encoder-only mode, Linear encoder: the node rows' gradient = the token-row gradient stage 1 left (c->dy), scattered back to the
    // nodes in the token type (zero rows for the nodes a truncated graph drops; the CLS rows were summed in stage 1)
    GT_TRY(gt_seq_scatter(c->tdt, c->dy, nullptr, c->g.graph_ptr, c->g.node_graph, c->seq_desc, c->in.B, 1, 1, N, D, Q(c->q_d_hn), nullptr, st));
    d_h0 = Q(c->q_d_hn);
    dy_dt = c->tdt;
  } else if (m->enc_only) {
    // ... table encoders: every table row sums its nodes' token-row gradients through the forward's row map and sort plan; d perturb =
    // the node's token-row gradient (zero rows for dropped nodes), written by the same call into the caller's buffer
    GT_CHECK_ARG(c->k.esort, "backward of a forward prepared without will_bwd");
    float* d_tabs[MAXT];
    for (int t = 0; t < c->T; ++t) d_tabs[t] = G + m->off_tables[t];
    GT_TRY(gt_embed_tokens_bwd(c->T, c->e_rows, c->tdt, c->dy, (const int32_t*)P(c->o_rowmap), N, D, P(c->o_eplan), d_tabs, c->in.d_perturb,
                               W(), ws_bytes, st));
    return flush();
  }
  if (m->embed_kind == 1) {   // dW = d_h0^T x, db = colsum(d_h0); the features need no gradient
    const int64_t K = m->ne_K, Kp = (int64_t)c4((size_t)K);
    float* dw = Kp == K ? G + m->off_ne_w : (float*)Q(c->q_ne_dw);
    GT_TRY(gt_linear_bwd(GT_F32, dy_dt, c->compute, c->ne_x, c->ne_w, d_h0, nullptr, nullptr, nullptr, nullptr, dw, G + m->off_ne_b, N, D, Kp,
                         0.f, W(), ws_bytes, st));
    if (Kp != K) GT_TRY(flush());   // the re-pitch below reads the summed gradient
    if (c->k.ov) gt_overlap_dw_sync();
    if (Kp != K) GT_TRY(gt_repitch(G + m->off_ne_w, K, dw, Kp, D, 4, st));
  } else {
    float* d_tabs[MAXT];
    for (int t = 0; t < c->T; ++t) d_tabs[t] = G + m->off_tables[t];
    if (c->k.esort)
      GT_TRY(gt_embed_sum_bwd_sorted(c->T, c->e_rows, (const float*)d_h0, N, D, P(c->o_eplan), d_tabs, W(), ws_bytes, st));
    else
      GT_TRY(gt_embed_sum_bwd(c->T, c->e_idx, c->e_str, c->e_clamp, c->e_rows, (const float*)d_h0, N, D, d_tabs, W(), ws_bytes, st));
  }
  // the virtual-node chain's tail (d vn_0 reduced on the second stream) joins here; the overlap section closes in the guard
  if (m->has_vn && side) GT_TRY(gt_stream_wait_event(st, m->ev_vnemb));
  return flush();
}

}  // namespace

extern "C" int gt_model_backward(const gt_model* m, void* ctx_, const float* dlogits, float* grads, void* barena, int stages,
                                 gt_stream_t st) {
  GT_TRY(model_check("gt_model_backward", m));
  Ctx* c = (Ctx*)ctx_;
  GT_CHECK_ARG(c && c->magic == CTX_MAGIC && c->forwarded, "context without a forward");
  GT_CHECK_ARG(dlogits && grads && barena, "null buffer");
  GT_CHECK_ARG(stages > 0 && stages < 8, "bad stage mask");
  // frozen message-passing stack (gt_model_batch::gnn_frozen): stage 1 is the whole backward and closes it; bits 1 and 2 do nothing,
  // in the same call or in later ones
  const bool frozen = c->in.gnn_frozen != 0;
  if (frozen) {
    if (!(stages & 1)) {
      GT_CHECK_ARG(c->stages_done & 1, "stage order");
      return GT_OK;
    }
    stages = 7;
  }
  GT_CHECK_ARG(!(stages & c->stages_done), "bad stage mask");
  GT_CHECK_ARG(!(stages & 2) || ((stages | c->stages_done) & 1), "stage order");
  GT_CHECK_ARG(!(stages & 4) || ((stages | c->stages_done) & 2), "stage order");
  GT_CHECK_ARG(!c->stages_done || (char*)barena == c->bb, "the stages of one backward share one arena");
  c->bb = (char*)barena;
  const Bwd s{m, c, grads, st, m->has_vn ? m->st_vn : nullptr};

  BindGuard guard;
  GT_TRY(bind_images(m, c));
  if (c->k.ov) {   // (Decisions::ov)
    if (!c->stages_done) GT_TRY(gt_overlap_dw_begin(st, m->st_dw));
    guard.dw = (stages & 4) != 0;   // the section stays open between the stage calls of one backward (same host thread)
  }
  // the deferred-reduce section (sized by prepare_backward_arena) is open across the stage calls like the overlap section; the arena is
  // not reused inside one backward
  if (!c->stages_done) {
    GT_TRY(gt_defer_begin(c->defer_bytes ? s.Q(c->q_defer) : nullptr, c->defer_bytes));
    if (c->defer_bytes && c->defer_small) GT_TRY(gt_defer_limit(c->defer_small));
  }
  guard.defer_abort = true;   // cleared on the successful way out
  // (an error return in a middle stage leaves the section open on this thread: the next gt_overlap_dw_begin resets it)

  if (stages & 1) {
    GT_TRY(s.encoder(dlogits, frozen));
    c->stages_done |= 1;
    if (frozen) {   // the closing joins of stage 4: nothing is left to queue a sum, the overlap section closes in the guard
      GT_TRY(gt_defer_end());
      c->stages_done = 7;
    }
  }
  if ((stages & 2) && !frozen) {
    if (!m->enc_only) GT_TRY(s.message_passing());   // (encoder-only mode: the bit is accepted and does nothing)
    c->stages_done |= 2;
  }
  if ((stages & 4) && !frozen) {
    GT_TRY(s.input_encoder());
    GT_TRY(gt_defer_end());
    c->stages_done |= 4;
  }
  guard.defer_abort = false;   // (between the stage calls of one backward the section stays open, like the overlap section)
  return GT_OK;
}

// sizes of the caller-filled structs (a binding checks its mirror of the layouts against these)
extern "C" int gt_model_abi_sizes(int64_t* out4) {
  GT_CHECK_ARG(out4, "null output");
  out4[0] = (int64_t)sizeof(gt_model);
  out4[1] = (int64_t)sizeof(gt_model_batch);
  out4[2] = (int64_t)sizeof(gt_image_set);
  out4[3] = (int64_t)sizeof(gt_stage_ring);
  return GT_OK;
}

// The token layout on the host on its own (what gt_model_prepare writes into its staging slot): meta8 = {rows, max_npos, num_work,
// offset of last_rows, offset of the work list, total bytes, S, row_stride}; out_host == NULL only sizes it.
extern "C" int gt_seq_layout_host(int kind, const int64_t* sizes_host, int64_t B, int64_t max_input_len, int with_cls, void* out_host,
                                  size_t out_bytes, int64_t* meta8) {
  GT_CHECK_ARG(meta8 && B >= 0 && (sizes_host || !B), "null argument");
  GT_CHECK_ARG(kind == GT_SEQ_PACKED || kind == GT_SEQ_PADDED, "bad layout kind");
  const SeqHostLayout h = seq_layout_rank(kind, sizes_host, B, max_input_len, with_cls ? 1 : 0);
  meta8[0] = h.rows; meta8[1] = h.max_npos; meta8[2] = h.num_work;
  meta8[3] = (int64_t)h.blob.o_last; meta8[4] = (int64_t)h.blob.o_work; meta8[5] = (int64_t)h.blob.bytes;
  meta8[6] = h.S; meta8[7] = h.row_stride;
  if (!out_host) return GT_OK;
  if (out_bytes < h.blob.bytes) { gt_set_error("gt_seq_layout_host: buffer too small"); return GT_ERR_WORKSPACE; }
  seq_layout_fill(h, (char*)out_host);
  return GT_OK;
}

extern "C" int gt_seq_layout_packed_host(const int64_t* sizes_host, int64_t B, int64_t max_input_len, int with_cls, void* out_host,
                                         size_t out_bytes, int64_t* meta6) {
  GT_CHECK_ARG(meta6, "null argument");
  int64_t meta8[8] = {};
  const int rc = gt_seq_layout_host(GT_SEQ_PACKED, sizes_host, B, max_input_len, with_cls, out_host, out_bytes, meta8);
  std::copy(meta8, meta8 + 6, meta6);
  return rc;
}

extern "C" int gt_stage_ring_take(gt_stage_ring* ring, size_t bytes, void** slot, void** event) {
  GT_CHECK_ARG(ring && ring->base && ring->slots > 0 && ring->slots <= 64 && slot && event, "bad staging ring");
  if ((int64_t)bytes > ring->slot_bytes) { gt_set_error("gt_stage_ring_take: %zu bytes exceed the staging slot", bytes); return GT_ERR_WORKSPACE; }
  const int i = ring->next;
  ring->next = (i + 1) % ring->slots;
  if (ring->events[i]) (void)hipEventSynchronize((hipEvent_t)ring->events[i]);   // the copy that last read this slot has completed
  *slot = (char*)ring->base + (size_t)i * (size_t)ring->slot_bytes;
  *event = ring->events[i];
  return GT_OK;
}
