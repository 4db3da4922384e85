"""The host-only description of a model for the whole-model driver (csrc/model.hip): pure Python over the module tree.

A fused model is built in three steps, and this module is the first:
  1. `ModelLayout(model)` (here) reads the module tree and lays out the flat gradient buffer -- family and shape, the ordered
     (parameter, offset) list, every `off_*` value of `gt_model`, the storage groups whose parameters must share one matrix, the
     descriptor arrays with their non-pointer fields, and the list of (struct, pointer field, tensor) the binding has to write.
     It calls neither the library nor the device, does not touch the model, and works on a model whose parameters are on the CPU.
  2. `engine.bind_storage` re-homes the storage groups, then writes every parameter and buffer pointer (device-agnostic).
  3. `engine._Plan` adds the device resources: streams, events, the PNA images, the weight images, the flat buffer.
`structural_ok` is the part of `engine.eligible` that asks the same module tree, through the same helpers (`input_encoder`,
`edge_encoder`, `emb_dim`, `vn_mlp`): where the parameters live and what the library says about the head dim stay in engine.py.
The gradient block orders are the contract with gt_model_forward / gt_model_backward / gt_model_grad_ranges.
"""
import numpy as np
import torch

from . import layers

MAXL, MAXT = 16, 16   # GT_MODEL_MAX_LAYERS, GT_MODEL_MAX_TABLES
W_MAX_BOUND = 64      # W3_MAX_BOUND / W1_MAX_BOUND of the library's bind tables
SCALER_KIND = {None: 0, "identity": 0, "amplification": 1, "attenuation": 2, "linear": 3, "inverse_linear": 4}


def _c4(n):
    return (n + 3) // 4 * 4


# ---- the model families -------------------------------------------------------------------------------------------------------
def readout_kind(model):
    """GT_POOL_* of a `models.gnn.GNN` or a `models.pna.PNANet` (the driver's read-out mode: message passing -> per-graph pooling ->
    heads), 0 for the token-path models"""
    from .models.gnn import GNN
    from .models.pna import PNANet
    from .ops import POOL_KINDS
    return POOL_KINDS[model.graph_pooling] if isinstance(model, (GNN, PNANet)) else 0


def model_parts(model):
    """(message-passing stack, token encoder, input encoder) of a model -- THE place that knows where each model family keeps them:
    `gnn_node` / `transformer_encoder` / `gnn_node.node_encoder` for the four families with message passing (no token encoder in the
    read-out mode), None / `transformer` / `node_encoder` for `models.transformer.Transformer`, which has no message passing (the
    driver's encoder-only mode, gt_model::enc_only)."""
    from .models.transformer import Transformer
    if isinstance(model, Transformer):
        return None, model.transformer, model.node_encoder
    gnn = model.gnn_node
    return gnn, (None if readout_kind(model) else model.transformer_encoder), gnn.node_encoder


def head_kind(model):
    """gt_model::head_kind: 0 the linear heads, 1 the narrow MLP of `PNANet` (max_seq_len None), 2 its per-position two-layer heads"""
    from .models.pna import PNANet
    if not isinstance(model, PNANet):
        return 0
    return 1 if model.max_seq_len is None else 2


def emb_dim(model):
    """gnn_emb_dim (d_model for a model without message passing): the width of the node rows, and of a perturbation"""
    gnn, enc, _ = model_parts(model)
    if gnn is None:
        return int(enc.d_model)
    return int(gnn.layers[0].in_channels if hasattr(gnn, "layers") else gnn.convs[0].emb_dim)


def conv_kind(gnn):
    """"pna" (PNANodeEmbedding), "gin" or "gcn" -- "gcn" also without message passing, where gt_model::conv is not read"""
    from .modules.conv import GINConv
    if gnn is None:
        return "gcn"
    if hasattr(gnn, "layers"):
        return "pna"
    return "gin" if isinstance(gnn.convs[0], GINConv) else "gcn"


def input_encoder(ne):
    """(kind, tables, clamps) of an input encoder: "ast" (ASTNodeEncoder: type, attribute and depth tables, the depth clamped),
    "linear" (nn.Linear over dense float features, dataset/tud.py:65), "atom" (AtomEncoder-style list of tables) or None"""
    if hasattr(ne, "type_encoder"):
        return "ast", [ne.type_encoder.weight, ne.attribute_encoder.weight, ne.depth_encoder.weight], [-1, -1, int(ne.max_depth)]
    if type(ne) is torch.nn.Linear:
        return "linear", [], []
    if hasattr(ne, "atom_embedding_list"):
        tabs = [e.weight for e in ne.atom_embedding_list]
        return "atom", tabs, [-1] * len(tabs)
    return None, [], []


def edge_encoder(conv):
    """(kind, parameters) of a GCN / GIN conv's edge encoder: "tables" (BondEncoder-style: one table per edge_attr column), "linear"
    (a module: its weight and bias) or None (a plain callable: the "zero" encoder)"""
    ee = conv.edge_encoder
    tabs = getattr(ee, "bond_embedding_list", None)
    if tabs is not None:
        return "tables", [t.weight for t in tabs]
    if isinstance(ee, torch.nn.Module):
        return "linear", [ee.weight, ee.bias]
    return None, []


def vn_mlp(seq):
    """(Linear, BatchNorm, Linear, BatchNorm) of a virtual-node MLP: Linear -> BN -> ReLU -> Linear -> BN -> ReLU (gnn_module.py:170-176)"""
    lin1, bn1, _, lin2, bn2, _ = list(seq)   # (any other length: ValueError)
    return lin1, bn1, lin2, bn2


def gin_mlp(conv):
    """(Linear, BatchNorm, Linear) of a GINConv's MLP: Linear -> BN -> ReLU -> Linear (conv.py:21-22)"""
    lin1, bn1, _, lin2 = list(conv.mlp)   # (any other length: ValueError)
    return lin1, bn1, lin2


def _wb(*mods):
    return [p for m in mods for p in (m.weight, m.bias)]


def frozen_pattern(model):
    """Which parameters of `model` are frozen (requires_grad == False): "none", "gnn" -- exactly the parameters of model.gnn_node,
    what epoch_callback's freeze_gnn leaves behind -- or "other" (a single conv, gnn2transformer, gnn_node plus a head, ...).
    Pure: flags only, no device, no library call."""
    frozen = {id(p) for p in model.parameters() if not p.requires_grad}
    if not frozen:
        return "none"
    gnn = model_parts(model)[0]   # (a model without message passing has no "gnn" pattern)
    return "gnn" if gnn is not None and frozen == {id(p) for p in gnn.parameters()} else "other"


def _frozen_ok(model):
    """every parameter trainable, or -- only with `model.fused_freeze`, never in the read-out or the encoder-only mode -- exactly
    gnn_node frozen"""
    pat = frozen_pattern(model)
    if readout_kind(model) or model_parts(model)[0] is None:
        return pat == "none"
    return pat == "none" or (pat == "gnn" and bool(getattr(model, "fused_freeze", False)))


# ---- the PNA tower images -------------------------------------------------------------------------------------------------------
def pna_maps(L, T, F, aggregators, blocks, scalers, K):
    """The gather map of the PNA tower images and its inverse, as int64 arrays, and the image offsets [L][4].
    Source (the flat tower storage), per layer: [pre_w (T,F,2F) | pre_b (T,F) | post_w (T,F,cols) | post_b (T,F)].
    Image, per layer: [pre_stack (T,2F,F) | pre_b2 (T,2F) | Wst (T,S*F,(1+K)F) | bst (T,S*F)]; map[i] is the source index of image
    entry i, or -1 for an entry that stays zero; inv[j] is the image entry of source element j (every one sits there exactly once).
    The post-net block restates PNAConv._post_maps (modules/pna/pna_module.py) with the layer's source base added."""
    from .modules.pna.pna_module import _AGG_SLOT
    A, S = len(aggregators), len(blocks)
    first = S - len(scalers)
    cols = (A * len(scalers) + 1) * F
    KF = (1 + K) * F          # the post-Linear's operand [x | K aggregates] per tower
    per_layer = T * F * 2 * F + T * F + T * F * cols + T * F
    img_per_layer = T * 2 * F * F + T * 2 * F + T * S * F * KF + T * S * F
    n_src, n_img = L * per_layer, L * img_per_layer
    mp = np.full(n_img, -1, dtype=np.int64)
    img_off = []
    t_ = np.arange(T).reshape(T, 1, 1)
    for l in range(L):
        sb = l * per_layer                      # source bases of this layer
        s_pre_w, s_pre_b = sb, sb + T * F * 2 * F
        s_post_w, s_post_b = s_pre_b + T * F, s_pre_b + T * F + T * F * cols
        ib = l * img_per_layer
        i_pre_w, i_pre_b = ib, ib + T * 2 * F * F
        i_post_w, i_post_b = i_pre_b + T * 2 * F, i_pre_b + T * 2 * F + T * S * F * KF
        r = np.arange(2 * F).reshape(1, 2 * F, 1)
        k = np.arange(F).reshape(1, 1, F)
        src = s_pre_w + t_ * (F * 2 * F) + np.where(r < F, r, r - F) * (2 * F) + np.where(r < F, 0, F) + k
        mp[i_pre_w:i_pre_w + T * 2 * F * F] = src.reshape(-1)
        rb = np.arange(2 * F).reshape(1, 2 * F)
        srcb = np.where(rb < F, s_pre_b + np.arange(T).reshape(T, 1) * F + rb, -1)
        mp[i_pre_b:i_pre_b + T * 2 * F] = srcb.reshape(-1)
        # post: block s of tower t, output o, operand column c in [x | mean | max | min | std (| sum | var)]
        w = np.full((T, S * F, KF), -1, dtype=np.int64)
        o = np.arange(F).reshape(F, 1)
        f = np.arange(F).reshape(1, F)
        for t in range(T):
            tb = s_post_w + t * F * cols
            for s_ in range(S):
                rows = slice(s_ * F, (s_ + 1) * F)
                if s_ == 0:
                    w[t, rows, 0:F] = tb + o * cols + f
                if s_ < first:
                    continue
                for ai, a in enumerate(aggregators):
                    slot = _AGG_SLOT[a]
                    w[t, rows, F + slot * F:F + (slot + 1) * F] = tb + o * cols + F + (s_ - first) * A * F + ai * F + f
        mp[i_post_w:i_post_w + T * S * F * KF] = w.reshape(-1)
        bb = np.full((T, S * F), -1, dtype=np.int64)
        bb[:, :F] = s_post_b + np.arange(T).reshape(T, 1) * F + np.arange(F).reshape(1, F)
        mp[i_post_b:i_post_b + T * S * F] = bb.reshape(-1)
        img_off.append([i_pre_w, i_pre_b, i_post_w, i_post_b])
    inv = np.full(n_src, -1, dtype=np.int64)
    used = mp >= 0
    inv[mp[used]] = np.nonzero(used)[0]
    assert (inv >= 0).all(), "every tower weight sits in the images exactly once"
    return mp, inv, img_off


# ---- the flat gradient buffer -----------------------------------------------------------------------------------------------------
class _Alloc:
    """The flat gradient buffer's allocator: the ordered (parameter, offset) list and the running total, in floats"""
    def __init__(self):
        self.params, self.total = [], 0

    def seg(self, p, size=None):
        """`p` at the current end; it takes its numel rounded up to 4 floats, or `size` floats: its offset"""
        off = self.total
        self.params.append((p, off))
        self.total += _c4(p.numel()) if size is None else size
        return off

    def block(self, ps):
        """parameters one behind the other, each rounded up to 4 floats: the block's first offset"""
        return [self.seg(p) for p in ps][0]

    def stacked(self, ps):
        """a storage group's members one behind the other WITHOUT rounding (their gradients are ONE matrix): the first offset"""
        return [self.seg(p, p.numel()) for p in ps][0]

    def align(self):
        self.total = _c4(self.total)


class ModelLayout:
    """Step 1 of a plan (see the module docstring): everything derived from the modules alone; `engine._Plan` binds it"""
    def __init__(self, model):
        from .modules.gnn_module import GNN_node_Virtualnode
        self.readout = readout_kind(model)
        gnn, enc, ne = model_parts(model)   # (read-out mode: nothing behind gnn_node but the heads; encoder-only mode: no gnn_node)
        self.enc_only = gnn is None
        self.kind = conv_kind(gnn)
        self.L, self.has_vn = (0 if gnn is None else gnn.num_layer), isinstance(gnn, GNN_node_Virtualnode)
        self.D = emb_dim(model)
        self.jk_cat = self.kind != "pna" and gnn is not None and gnn.JK == "cat"
        self.d = self.D if self.readout else enc.d_model   # the heads' input width
        self.num_tasks = model.num_tasks
        L, D = self.L, self.D
        a = self._alloc = _Alloc()
        self.ptrs = []             # (descriptor struct, or None for gt_model itself; pointer field; the tensor it names)
        self.storage_groups = []   # parameter lists whose storage must become one matrix, in order (engine.bind_storage re-homes them)
        f = self.fields = {k: -1 for k in ("off_ne_w", "off_ne_b", "off_vn_emb", "off_g2t_w", "off_g2t_b", "off_cls", "off_nin_w", "off_nin_b",
                                           "off_nout_w", "off_nout_b", "off_hid_w", "off_hid_b", "off_hid2_w", "off_hid2_b")}
        # ---- the input encoder and the virtual-node embedding
        self.embed_kind, self.embed, self.embed_clamp = input_encoder(ne)
        f["embed_kind"] = {"atom": 0, "linear": 1, "ast": 2}[self.embed_kind]
        f["n_tables"] = len(self.embed)
        f["off_tables"] = [a.seg(w) for w in self.embed]
        f["table_rows"], f["table_clamp"] = [int(w.shape[0]) for w in self.embed], list(self.embed_clamp)
        self.ne_lin, self.ne_K = (ne, int(ne.in_features)) if self.embed_kind == "linear" else (None, 0)
        if self.ne_lin is not None:
            f["off_ne_w"], f["off_ne_b"], f["ne_K"] = a.seg(ne.weight), a.seg(ne.bias), self.ne_K
            self.ptrs += [(None, "ne_w", ne.weight), (None, "ne_b", ne.bias)]
        self.vn_emb = gnn.virtualnode_embedding.weight if self.has_vn else None
        if self.has_vn:
            f["off_vn_emb"] = a.seg(self.vn_emb)
            self.ptrs.append((None, "vn_emb", self.vn_emb))
        # x_0 = h_0 + vn_0[batch] with vn_0 = the ONE row of virtualnode_embedding for every graph (gnn_module.py:195):
        # the embedding-sum kernel takes it as one more table whose index column is a stride-0 zero
        self.vn0_in_embed = self.has_vn and self.embed_kind != "linear" and len(self.embed) < 16
        self.embed_sorted = bool(self.embed) and max(int(t.shape[0]) for t in self.embed) <= 16384
        # ---- message passing
        self.w3_weights, self.w3_tail = [], []   # weights with bf16x3 images: the convs' (the binding appends the PNA tower views) | the rest
        self.conv_desc = None
        f["off_conv"], f["off_vn"] = [], []
        if self.kind == "pna":
            self._layout_pna(gnn)
        elif not self.enc_only:
            self._layout_convs(gnn)
        nvn = L - 1 if self.has_vn else 0
        self.vn_desc = (layers.VnUpdateDesc * max(nvn, 1))()
        for l in range(nvn):
            lin1, bn1, lin2, bn2 = vn_mlp(gnn.mlp_virtualnode_list[l])
            ps = _wb(lin1, bn1, lin2, bn2)
            f["off_vn"].append(a.block(ps))
            desc = self.vn_desc[l]
            desc.D = D
            self.ptrs += [(desc, n, p) for n, p in zip(("w1", "b1", "bn1_w", "bn1_b", "w2", "b2", "bn2_w", "bn2_b"), ps)]
            self._bn(desc, bn1, "bn1", hyper=True)
            self._bn(desc, bn2, "bn2")
        # ---- gnn2transformer, cls / norm_input, the encoder layers, the final norm (token path, encoder-only mode)
        self.cls = None
        self.enc_layers, self.w3_enc_weights = [], []   # (the encoder layers' GEMMs run in fp32 only in the fp32 mode: fp32 token rows)
        self.enc_desc = (layers.EncoderLayerDesc * 1)()
        if enc is not None:
            self._layout_encoder(model, enc)
        self._layout_heads(model)
        if self.ne_lin is not None and _c4(self.ne_K) == self.ne_K:
            self.w3_tail.append(ne.weight)
        pe = getattr(model, "pos_encoder", None)
        # PositionalEncoding (token_layout="packed" only, see GNNTransformer._use_packed): the module's buffer, read as [max_len][d]
        self.pe = pe.pe if pe is not None else None
        if pe is not None:
            f["pe_rows"] = int(self.pe.shape[0])
            self.ptrs.append((None, "pe", self.pe))
        self.params, self.total = a.params, a.total
        f.update(conv={"gcn": 0, "gin": 1, "pna": 2}[self.kind], L=L, n_enc=len(self.enc_layers), has_vn=int(self.has_vn),
                 jk_cat=int(self.jk_cat), residual=int(bool(gnn.residual)) if gnn is not None else 0, D=D, d=self.d, Nh=self.Nh, ldy=self.ldy,
                 readout=self.readout, pad_readout_=int(self.enc_only), max_input_len=int(enc.max_input_len) if enc is not None else 0,
                 with_cls=int(self.cls is not None), vn0_in_embed=int(self.vn0_in_embed), embed_sorted=int(self.embed_sorted),
                 head_kind=self.head_kind, grad_total=self.total)

    def fill(self, cm):
        """every non-pointer, non-stream, non-event field of a gt_model (engine.ModelDesc) but the two binding-time switches"""
        for k, v in self.fields.items():
            if isinstance(v, list):
                arr = getattr(cm, k)
                for i, x in enumerate(v):
                    arr[i] = type(arr[i])(*x) if isinstance(x, list) else x
            else:
                setattr(cm, k, v)

    def _bn(self, desc, bn, name="bn", hyper=False):
        """a descriptor's BatchNorm fields from the module: the running buffers `<name>_rm / _rv / _nbt`; hyper: this is the module
        whose momentum and eps the descriptor's ONE bn_momentum / bn_eps pair carries"""
        self.ptrs += [(desc, name + "_rm", bn.running_mean), (desc, name + "_rv", bn.running_var), (desc, name + "_nbt", bn.num_batches_tracked)]
        if hyper:
            desc.bn_momentum, desc.bn_eps = float(bn.momentum), float(bn.eps)

    def _layout_convs(self, gnn):
        """GCN / GIN layers.  Gradient block order of gt_gcn_layer_bwd: lin_w, lin_b, root, edge_w, edge_b, bn_w, bn_b;
        of gt_gin_layer_bwd: eps (20-float slot), edge tables | edge_w, edge_b, w1, b1, bn1_w, bn1_b, w2, b2, bn_w, bn_b"""
        a, f, D = self._alloc, self.fields, self.D
        self.convs = list(zip(gnn.convs, gnn.batch_norms))
        # BondEncoder-style tables: the aggregate kernels read ONE [rows][D] matrix per layer.  Instead of stacking a layer's tables
        # by a torch.cat per step, the parameters' storage IS the stacked matrix -- each table's weight becomes a view of it
        edges = [edge_encoder(conv) for conv, _ in self.convs]
        tabs_all = [ps for mode, ps in edges if mode == "tables"]
        if any(tabs_all):
            self.storage_groups.append([t for tl in tabs_all for t in tl])
        self.conv_desc = ((layers.GinLayerDesc if self.kind == "gin" else layers.GcnLayerDesc) * self.L)()
        for l, (conv, bn) in enumerate(self.convs):
            desc = self.conv_desc[l]
            mode, edge = edges[l]
            desc.D = D
            if self.kind == "gcn":
                f["off_conv"].append(a.block([*_wb(conv.linear), conv.root_emb.weight, *edge, *_wb(bn)]))
                self.w3_weights.append(conv.linear.weight)
                self.ptrs += [(desc, "lin_w", conv.linear.weight), (desc, "lin_b", conv.linear.bias), (desc, "root", conv.root_emb.weight)]
            else:
                lin1, bn1, lin2 = gin_mlp(conv)
                f["off_conv"].append(a.seg(conv.eps, 20))   # d_eps + the aggregate backward's scratch (GIN_EPS_SLOT in layers.hip)
                a.block([*edge, *_wb(lin1, bn1, lin2, bn)])
                self.w3_weights += [lin1.weight, lin2.weight]
                self.ptrs += [(desc, "eps", conv.eps)] + [(desc, n, p) for n, p in zip(("w1", "b1", "bn1_w", "bn1_b", "w2", "b2"), _wb(lin1, bn1, lin2))]
                self._bn(desc, bn1, "bn1")
            if mode == "linear":
                desc.edge_mode, desc.edge_cols = layers.GT_EDGE_LINEAR, edge[0].shape[1]
                self.ptrs += [(desc, "edge_w", edge[0]), (desc, "edge_b", edge[1])]
            elif mode == "tables":
                desc.edge_mode = layers.GT_EDGE_TABLES
                desc.edge_cols, desc.table_rows = len(edge), sum(int(t.shape[0]) for t in edge)
                acc = 0
                for i, t in enumerate(edge):
                    desc.tab_off[i] = acc
                    acc += int(t.shape[0])
                self.ptrs.append((desc, "edge_w", edge[0]))   # the layer's stacked [rows][D] block
            else:
                desc.edge_mode = layers.GT_EDGE_NONE
            self.ptrs += [(desc, "bn_w", bn.weight), (desc, "bn_b", bn.bias)]
            self._bn(desc, bn, hyper=True)

    def _layout_pna(self, gnn):
        """PNANodeEmbedding (modules/pna/pna_module.py:16-78): per layer lin / BatchNorm gradients in the layer block of the flat
        buffer; the tower weights of ALL layers are one storage group, from which the driver rebuilds the re-stacked images
        [A ; B], [b | 0], the per-scaler post-Linear blocks and their bias with ONE gather per step (`pna_maps`)."""
        a, f, L, D = self._alloc, self.fields, self.L, self.D
        convs = list(gnn.layers)
        self.convs = list(zip(convs, [b.module for b in gnn.batch_norms]))
        c0 = convs[0]
        T, F, S, K = c0.towers, c0.F_in, len(c0._blocks), c0.agg_slots   # K: the aggregate kernel's slot count: 4, or 6 with sum / var
        self.pna_T, self.pna_F, self.pna_S, self.pna_K = T, F, S, K
        cols = (len(c0.aggregators) * len(c0.scalers) + 1) * F
        # ---- the flat tower storage: per layer [pre_w (T,F,2F) | pre_b (T,F) | post_w (T,F,cols) | post_b (T,F)]
        towers = [p for conv in convs for nns in (conv.pre_nns, conv.post_nns)
                  for p in [nn[0].weight for nn in nns] + [nn[0].bias for nn in nns]]
        self.pna_map_np, self.pna_inv_np, img_off = pna_maps(L, T, F, c0.aggregators, c0._blocks, c0.scalers, K)
        assert sum(p.numel() for p in towers) == self.pna_inv_np.size and tuple(towers[0].shape) == (F, 2 * F) and tuple(towers[2 * T].shape) == (F, cols)
        self.storage_groups.append(towers)
        self.conv_desc = (layers.PnaLayerDesc * L)()
        # ---- gradient layout: per layer [lin_w, lin_b, bn_w, bn_b] (gt_pna_layer_bwd's order), then the flat tower storage
        for l, (conv, bn) in enumerate(self.convs):
            f["off_conv"].append(a.block(_wb(conv.lin, bn)))
            self.w3_weights.append(conv.lin.weight)
            desc = self.conv_desc[l]
            desc.D, desc.T, desc.S, desc.agg_slots = D, T, S, K
            self.ptrs += [(desc, n, p) for n, p in zip(("lin_w", "lin_b", "bn_w", "bn_b"), _wb(conv.lin, bn))]
            self._bn(desc, bn, hyper=True)
        f["off_pna_src"] = a.stacked(towers)
        self.ptrs.append((None, "pna_src", towers[0]))
        f.update(pna_img_off=img_off, pna_n_img=int(self.pna_map_np.size), pna_n_src=int(self.pna_inv_np.size),
                 pna_kinds=[SCALER_KIND[blk] for blk in c0._blocks], pna_avg_log=float(c0.avg_deg["log"]), pna_avg_lin=float(c0.avg_deg["lin"]))

    def _layout_encoder(self, model, enc):
        a, f, d = self._alloc, self.fields, self.d
        if not self.enc_only:
            g2t = model.gnn2transformer
            f["off_g2t_w"], f["off_g2t_b"] = a.seg(g2t.weight), a.seg(g2t.bias)
            self.ptrs += [(None, "g2t_w", g2t.weight), (None, "g2t_b", g2t.bias)]
            self.w3_tail.append(g2t.weight)
        self.cls = enc.cls_embedding
        if self.cls is not None:
            f["off_cls"] = a.seg(self.cls)
            self.ptrs.append((None, "cls", self.cls))
        def norm(which, mod):
            if mod is not None:
                f["off_%s_w" % which], f["off_%s_b" % which], f[which + "_eps"] = a.seg(mod.weight), a.seg(mod.bias), float(mod.eps)
                self.ptrs += [(None, which + "_w", mod.weight), (None, which + "_b", mod.bias)]
        norm("nin", enc.norm_input)
        self.enc_layers = list(enc.transformer.layers)
        self.enc_desc = (layers.EncoderLayerDesc * max(len(self.enc_layers), 1))()
        f["off_enc"] = []
        for i, mod in enumerate(self.enc_layers):
            ps = layers.encoder_layer_params(mod)
            f["off_enc"].append(a.block(ps))
            desc = self.enc_desc[i]
            desc.d_model, desc.ffn, desc.nhead = d, mod.linear1.weight.shape[0], enc.nhead
            desc.ln_eps, desc.act = float(mod.norm1.eps), layers.ENC_ACT[enc.activation]
            self.ptrs += [(desc, n, p) for n, p in zip(("in_w", "in_b", "out_w", "out_b", "l1_w", "l1_b", "l2_w", "l2_b", "n1_w", "n1_b",
                                                        "n2_w", "n2_b"), ps)]
            self.w3_enc_weights += [mod.self_attn.in_proj_weight, mod.self_attn.out_proj.weight, mod.linear1.weight, mod.linear2.weight]
        norm("nout", enc.transformer.norm)

    def _layout_heads(self, model):
        """the head block: hidden weights, hidden biases (PNANet only), output weights, output biases"""
        a, f = self._alloc, self.fields
        self.head_kind = head_kind(model)
        if self.head_kind == 1:     # mlp = Linear(D, 35) -> ReLU -> Linear(35, 17) -> ReLU -> Linear(17, T)  (models/pna.py:53-60)
            l1, l2, l3 = model.mlp[0], model.mlp[2], model.mlp[4]
            f["off_hid_w"], f["off_hid2_w"], f["off_hid_b"], f["off_hid2_b"] = a.seg(l1.weight), a.seg(l2.weight), a.seg(l1.bias), a.seg(l2.bias)
            f["head_h1"], f["head_h2"] = l1.out_features, l2.out_features
            self.ptrs += [(None, n, p) for n, p in zip(("hid_w", "hid_b", "hid2_w", "hid2_b"), _wb(l1, l2))]
            self.heads = [l3]
        elif self.head_kind == 2:   # per position Linear(D, D) -> ReLU -> Linear(D, T)  (models/pna.py:62-71): the hidden layers' storage
            hid = [seq[0] for seq in model.graph_pred_linear_list]   # becomes the stacked [L*D][D] matrix, as the output layers' below
            groups = [h.weight for h in hid], [h.bias for h in hid]
            f["head_pos"], f["off_hid_w"], f["off_hid_b"] = len(hid), a.stacked(groups[0]), a.stacked(groups[1])
            self.storage_groups += groups
            self.ptrs += [(None, "hid_w", hid[0].weight), (None, "hid_b", hid[0].bias)]
            self.heads = [seq[2] for seq in model.graph_pred_linear_list]
        elif model.max_seq_len is None:
            self.heads = [model.graph_pred_linear]
        else:
            self.heads = list(model.graph_pred_linear_list)
        self.Nh = sum(h.weight.shape[0] for h in self.heads)
        self.ldy = _c4(self.Nh)
        # head gradients: one [Nh][d] block and one [Nh] block, each rounded up to 4 floats; the per-head grads are slices of them.
        # The max_seq_len prediction heads (models/gnn_transformer.py:120-126) run as ONE GEMM over their stacked weights: the
        # parameters' storage IS the stacked matrix -- each head's weight / bias becomes a view of it
        for name, group in (("head_w", [h.weight for h in self.heads]), ("head_b", [h.bias for h in self.heads])):
            f["off_" + name] = a.stacked(group)
            a.align()
            if len(group) > 1:
                self.storage_groups.append(group)
            self.ptrs.append((None, name, group[0]))


# ---- the structural half of engine.eligible -----------------------------------------------------------------------------------------
def _bn_ok(bn):
    from .modules.norm import BatchNorm1d
    return isinstance(bn, BatchNorm1d) and bn.affine and bn.track_running_stats and bn.momentum is not None


def structural_ok(model):
    """What the fused step asks of the module tree alone (shapes, kinds, flags: answered for a CPU model as for one on the device).
    May raise on a model that is none of the families: engine._eligible_static holds the one `try` around it."""
    from .modules.norm import BatchNorm1d, any_sync
    gnn, enc, ne = model_parts(model)
    ro = readout_kind(model)
    if gnn is None:
        ok = _enc_only_ok(model, enc, ne)
    elif hasattr(gnn, "layers"):
        ok = _pna_ok(model, gnn, ro)
    else:
        ok = _convs_ok(model, gnn, ro)
    kind, tabs, _ = input_encoder(ne)
    if not ok or kind is None or (kind == "linear" and ne.bias is None) or (kind == "atom" and len(tabs) > 16):
        return False
    if enc is not None:   # what the encoder kernels ask of a TransformerNodeEncoder: layer count, activation, widths, FFN width
        if not (1 <= len(enc.transformer.layers) <= MAXL) or enc.activation not in layers.ENC_ACT or enc.d_model % 8:
            return False
        if enc.compute_dtype not in (torch.float32, torch.bfloat16) or any(mod.linear1.weight.shape[0] % 8 for mod in enc.transformer.layers):
            return False
    # (synchronised BatchNorm -- statistics over all data-parallel ranks -- runs on this path too: the library's BatchNorm calls
    # exchange their statistics through dist.BnSyncHook, installed around the pass; all of the model's BatchNorms or none)
    bns = [m for m in model.modules() if isinstance(m, BatchNorm1d)]
    if any_sync(*bns) and not (all(getattr(b, "sync", False) for b in bns) and len({id(getattr(b, "sync_group", None)) for b in bns}) == 1):
        return False
    return _frozen_ok(model)


def _convs_ok(model, gnn, ro):
    """GNN_node / GNN_node_Virtualnode with GCNConv or GINConv layers: the token path (packed layout, JK last / cat) or the read-out
    mode (models.gnn.GNN: JK = last only)"""
    from .modules.conv import GCNConv, GINConv, tables_fit_lds
    from .modules.norm import BatchNorm1d
    if ro:
        if gnn.JK != "last":
            return False
    elif not model._use_packed() or gnn.JK not in ("last", "cat") or model.gnn2transformer.weight.shape[1] % 4:
        return False
    D = emb_dim(model)
    kinds = {type(conv) for conv in gnn.convs}
    if gnn.num_layer > MAXL or D % 4 or len(kinds) != 1 or not (kinds <= {GCNConv, GINConv}):   # (MAXL: the driver's fixed-size tables)
        return False
    for conv, bn in zip(gnn.convs, gnn.batch_norms):
        if not _bn_ok(bn):
            return False
        if isinstance(conv, GINConv):
            lin1, bn1, lin2 = gin_mlp(conv)
            if not (isinstance(lin1, torch.nn.Linear) and isinstance(lin2, torch.nn.Linear) and _bn_ok(bn1)):
                return False
        mode, edge = edge_encoder(conv)
        ee = conv.edge_encoder
        if mode == "tables":
            if len(edge) > 4 or not tables_fit_lds(sum(int(t.shape[0]) for t in edge), D):
                return False
        elif mode == "linear":
            if not (isinstance(ee, torch.nn.Linear) and ee.in_features <= 4 and ee.bias is not None):
                return False
        else:
            e = ee(None)
            if not (isinstance(e, (int, float)) and e == 0):
                return False
    for seq in getattr(gnn, "mlp_virtualnode_list", ()):
        lin1, bn1, lin2, bn2 = vn_mlp(seq)
        if not (isinstance(lin1, torch.nn.Linear) and isinstance(bn1, BatchNorm1d) and isinstance(lin2, torch.nn.Linear) and isinstance(bn2, BatchNorm1d)):
            return False
    return True


def _enc_only_ok(model, enc, ne):
    """Transformer (models/transformer.py:20-115) on the driver's encoder-only mode: cls pooling and an input encoder whose rows can
    be the token rows -- ASTNodeEncoder / AtomEncoder with at most 16 tables of at most 16384 rows each (the sorted table backward,
    ops.EMBED_SORT_MAX_ROWS) and d_model columns, or nn.Linear(F, d_model).  (No frozen pattern in this mode: `_frozen_ok`.)"""
    from .ops import EMBED_SORT_MAX_ROWS
    if model.graph_pooling != "cls" or enc.cls_embedding is None:
        return False
    d = int(enc.d_model)
    kind, tabs, _ = input_encoder(ne)
    if kind == "linear":
        return ne.out_features == d
    return 1 <= len(tabs) <= MAXT and all(t.dim() == 2 and t.shape[1] == d and 1 <= t.shape[0] <= EMBED_SORT_MAX_ROWS for t in tabs)


def _pna_ok(model, gnn, ro):
    """PNATransformer (models/pna_transformer.py:16-118): PNANodeEmbedding with the residual connection, towers that divide the input,
    single-layer pre / post nets, packed token layout.  PNANet (models/pna.py:20-104): the same conv checks and the widths the head
    kernels take (csrc/mlp_heads.hip)."""
    if not _pna_convs_ok(gnn):
        return False
    D = emb_dim(model)
    if not ro:
        return model.pooling in ("cls", "last") and getattr(model, "layout", "auto") != "padded" and model.gnn2transformer.in_features == D
    if head_kind(model) == 1:
        l1, l2, l3 = model.mlp[0], model.mlp[2], model.mlp[4]
        return l1.in_features == D and max(l1.out_features, l2.out_features) <= 64 and all(m.bias is not None for m in (l1, l2, l3))
    heads = list(model.graph_pred_linear_list)
    if not (1 <= len(heads) <= 16 and D % 16 == 0 and D <= 512):
        return False
    return not any(seq[0].in_features != D or seq[0].out_features != D or seq[0].bias is None or seq[2].bias is None for seq in heads)


def _pna_convs_ok(gnn):
    """what the driver's PNA stack asks of a PNANodeEmbedding"""
    from .modules.pna.pna_module import PNAConv, _AGG_SLOT
    convs = list(gnn.layers)
    if not convs or len(convs) > MAXL or not gnn.residual:
        return False
    c0 = convs[0]
    for c in convs:
        if not (isinstance(c, PNAConv) and c.divide_input and c.in_channels == c.out_channels == c0.in_channels and c.towers == c0.towers
                and c.F_in == c.F_out and c.aggregators == c0.aggregators and c.scalers == c0.scalers and c.avg_deg == c0.avg_deg):
            return False
    if len(c0._blocks) > 8 or any(a not in _AGG_SLOT for a in c0.aggregators) or c0.in_channels > 1024:
        return False
    if any(b not in SCALER_KIND for b in c0._blocks) or not all(_bn_ok(getattr(bn, "module", None)) for bn in gnn.batch_norms):
        return False
    return not (c0.in_channels % 4 or c0.F_in % 4)
