"""Fused model path: the whole GNNTransformer forward (and its backward) as ONE autograd node and ONE C call per direction.

The module-by-module path (modules/, layers.py) costs ~3.5 ms of host time per Code2 step in Python autograd bookkeeping alone;
rounds 1-3 sequenced the library's layer composites from here (~60 ctypes calls, descriptor refresh, arena book-keeping: ~2.3 ms
of interpreter time per step).  Now the sequencing lives behind `gt_model_forward` / `gt_model_backward`
(csrc/model.hip, include/graphtrans_hip.h "Whole-model driver"): this module fills one `gt_model` struct per model (static
pointers, sizes, gradient offsets, streams, events) and one `gt_model_batch` per step, allocates the two arenas the driver asks for,
and hands the flat gradient buffer's slices to the parameters.  Autograd sees a single node.

A model's plan is built in three steps.  (1) model_layout.py, host only: `ModelLayout(model)` reads the module tree and lays out the
flat gradient buffer, the non-pointer fields of `gt_model` and of the layer descriptors, the storage groups and the list of pointers
to write; `structural_ok` is the half of `eligible` that asks the same tree.  (2) `bind_storage` here, device-agnostic: re-homes the
storage groups, then writes every pointer.  (3) `_Plan` here: streams, events, PNA and weight images, the flat buffer.

Covered configuration (everything else keeps using the module path, see `eligible`):
  GNN_node / GNN_node_Virtualnode with GCNConv or GINConv layers, Linear(<=4, D), BondEncoder-style
  embedding tables or "zero" edge encoders,
  any gnn_dropout, JK in {last, cat}, ASTNodeEncoder / AtomEncoder / nn.Linear inputs; a perturb (FLAG) only on request,
  `model.fused_flag` (--fused_flag): a contiguous fp32 [N, gnn_emb_dim] tensor, every parameter trainable, no active dist.GradSync
  -- the forward adds it inside the input encoder, the backward hands d h_list[0] out as its gradient (`_perturb_ok`);
  packed token layout (cls / last pooling, with or without the positional encoder, no masked layers), ReLU / GELU post-norm
  encoder layers; stacked max_seq_len heads or a single head;
  every parameter trainable, or -- on request, `model.fused_freeze` (--fused_freeze) -- exactly `gnn_node` frozen (freeze_gnn /
  epoch_callback): the same forward, and a backward that stops behind gnn2transformer's weight gradient (`frozen_pattern`).
  The GNN baseline (models/gnn.py: `GNN`) runs the driver's read-out mode (gt_model::readout): the same message-passing stack (GCN /
  GIN, JK = last), then sum / mean / max pooling per graph and the heads -- no gnn2transformer, token layout, staging ring or encoder
  weight images; every parameter trainable.
  The PNA baseline (models/pna.py: `PNANet`) runs the same mode over the PNA stack, with its own heads (gt_model::head_kind,
  csrc/mlp_heads.hip): the narrow MLP (max_seq_len None) or the per-position two-layer heads (gnn_emb_dim a multiple of 16 up to 512).
  The Transformer baseline (models/transformer.py: `Transformer`, opt-in `model.fused_step`, cls pooling) runs the driver's encoder-only
  mode (gt_model::enc_only): no message passing, the input encoder's rows are the token rows -- ASTNodeEncoder / AtomEncoder through
  gt_embed_tokens_*, nn.Linear in gnn2transformer's place -- then the token path's encoder, final norm and heads; every parameter
  trainable, a perturb only with `model.fused_flag` and a table encoder, no dist.GradSync.  `model_parts` tells the families apart.
Reference call path: trainers/base_trainer.py:29-36 -> models/gnn_transformer.py:88-127 -> modules/gnn_module.py:181-224 ->
modules/transformer_encoder.py:42-61.
"""
import ctypes as C
import os
import sys
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import GT_BF16, GT_EDGE_LINEAR, GT_EDGE_NONE, GT_EDGE_TABLES, GT_F32
from .graph import StageRingDesc, _stream, stage_ring
from .model_layout import (MAXL, MAXT, W_MAX_BOUND, ModelLayout, _frozen_ok, edge_encoder, emb_dim, frozen_pattern, head_kind,  # noqa: F401
                           input_encoder, model_parts, readout_kind, structural_ok)   # (callers and tests read them as engine.<name>)


OVERLAP_VN = os.environ.get("GT_OVERLAP_VN", "1") != "0"
OVERLAP_DW = os.environ.get("GT_OVERLAP_DW", "1") != "0"
# gt_graph_prep (8 short launches) and the encoder's weight images do not depend on anything the step computes: they run on a side
# stream beside the zero-fills, the bf16x3 images, the input embedding and layer 0's GEMM (csrc/model.hip)
PREP_OVERLAP = os.environ.get("GT_PREP_OVERLAP", "1") != "0"
# the overlap stream pays for itself only when the kernels are long enough to hide its extra stream operations
DW_OVERLAP_MIN_ELEMS = 1 << 20   # nodes x emb_dim of the batch
VN_DEFER_DW = os.environ.get("GT_VN_DEFER_DW", "1") != "0"

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


# ---- mirrors of the driver's structs (include/graphtrans_hip.h; sizes checked against gt_model_abi_sizes at first use) ----------
class ImageSet(C.Structure):   # gt_image_set
    _fields_ = [("n_jobs", _i32), ("n_bind", _i32)] + [(k, _vp) for k in ("job_w", "job_N", "job_K", "job_T", "job_img", "bind_w",
                                                                          "bind_N", "bind_K", "bind_f", "bind_t")]


class ModelDesc(C.Structure):   # gt_model
    _fields_ = [(k, _i32) for k in ("conv", "L", "n_enc", "has_vn", "jk_cat", "residual", "embed_kind", "n_tables", "vn0_in_embed",
                                    "embed_sorted", "with_cls", "vn_defer_dw")] + \
               [(k, _i64) for k in ("D", "d", "Nh", "ldy", "ne_K", "max_input_len", "dw_overlap_min_elems")] + \
               [("conv_layers", _vp), ("vn", _vp), ("enc", _vp), ("tables", _vp * MAXT), ("table_rows", _i64 * MAXT),
                ("table_clamp", _i64 * MAXT)] + \
               [(k, _vp) for k in ("vn_emb", "ne_w", "ne_b", "g2t_w", "g2t_b", "cls", "nin_w", "nin_b", "nout_w", "nout_b", "head_w",
                                   "head_b", "zero_i64")] + \
               [("nin_eps", _f32), ("nout_eps", _f32), ("off_tables", _i64 * MAXT), ("off_ne_w", _i64), ("off_ne_b", _i64),
                ("off_vn_emb", _i64), ("off_conv", _i64 * MAXL), ("off_vn", _i64 * MAXL), ("off_g2t_w", _i64), ("off_g2t_b", _i64),
                ("off_cls", _i64), ("off_nin_w", _i64), ("off_nin_b", _i64), ("off_enc", _i64 * MAXL), ("off_nout_w", _i64),
                ("off_nout_b", _i64), ("off_head_w", _i64), ("off_head_b", _i64), ("grad_total", _i64),
                ("st_vn", _vp), ("st_dw", _vp), ("st_prep", _vp), ("ev_x", _vp * MAXL), ("ev_vn", _vp * MAXL), ("ev_dvn", _vp * MAXL),
                ("ev_extra", _vp * MAXL), ("ev_pool", _vp * MAXL), ("ev_vnemb", _vp), ("ev_sort", _vp * 2), ("ev_wt", _vp * 2),
                ("ev_prep_begin", _vp), ("ev_graph", _vp), ("ev_w1", _vp), ("w3", ImageSet), ("w3_enc", ImageSet), ("w1", ImageSet),
                ("pna_src", _vp), ("pna_img", _vp), ("pna_map", _vp), ("pna_inv", _vp), ("pna_n_img", _i64), ("pna_n_src", _i64),
                ("off_pna_src", _i64), ("pna_img_off", (_i64 * 4) * MAXL), ("pna_kinds", _i32 * 8), ("pna_avg_log", _f32),
                ("pna_avg_lin", _f32)] + [(k, _i32) for k in ("head_kind", "head_h1", "head_h2", "head_pos")] + \
               [(k, _vp) for k in ("hid_w", "hid_b", "hid2_w", "hid2_b")] + \
               [(k, _i64) for k in ("off_hid_w", "off_hid_b", "off_hid2_w", "off_hid2_b")] + \
               [("readout", _i32), ("pad_readout_", _i32), ("pe", _vp), ("pe_rows", _i64)]
    # gt_model::enc_only took the place of the padding word beside `readout` (same size, same offsets; the mirror keeps the field's name)
    enc_only = property(lambda self: self.pad_readout_, lambda self, v: setattr(self, "pad_readout_", int(v)))


class BatchDesc(C.Structure):   # gt_model_batch
    _fields_ = [("N", _i64), ("E", _i64), ("B", _i64), ("edge_index", _vp), ("batch", _vp), ("sizes_host", _vp)] + \
               [(k, _vp) for k in ("graph_ptr", "node_graph", "in_ptr", "in_src", "in_eid", "out_ptr", "out_dst", "out_eid", "deg", "dis",
                                   "seq_desc", "last_rows", "work_items")] + \
               [("rows", _i64), ("max_npos", _i64), ("num_work", _i64), ("lay_exact", _i32), ("pad0_", _i32),
                ("x", _vp), ("x_stride0", _i64), ("x_stride1", _i64), ("node_depth", _vp), ("depth_stride", _i64), ("edge_attr", _vp),
                ("zeros_B", _vp), ("ident_B", _vp), ("ptr01", _vp)] + \
               [(k, _i32) for k in ("training", "compute", "tdt", "will_bwd", "use_w3", "use_w1", "sync_bn", "gnn_frozen")] + \
               [("gnn_p", _f32), ("enc_p", _f32), ("gnn_seed", C.c_uint64), ("enc_seed", C.c_uint64), ("ring", _vp),
                ("lay_S", _i64), ("lay_meta", _vp), ("perturb", _vp), ("d_perturb", _vp)]


class SizesDesc(C.Structure):   # gt_model_sizes
    _fields_ = [(k, _i64) for k in ("rows", "max_npos", "num_work", "arena_bytes", "barena_bytes")] + [("exact", _i32), ("pad_", _i32)]


_ABI_OK = []


def _check_abi():
    if not _ABI_OK:
        out = (_i64 * 4)()
        _lib.check(_lib.lib().gt_model_abi_sizes(out), "gt_model_abi_sizes")
        mine = (C.sizeof(ModelDesc), C.sizeof(BatchDesc), C.sizeof(ImageSet), C.sizeof(StageRingDesc))
        if tuple(out) != mine:
            raise RuntimeError("graphtrans_amd.engine: struct layouts differ from the library's (%r vs %r): rebuild the library" % (mine, tuple(out)))
        _ABI_OK.append(True)


# The overlap streams are created ONCE per device and shared by every plan: HIP maps streams onto a handful of hardware queues in
# creation order, and the streams of a second model's plan landed on the main stream's queue (measured: the second model built
# in a process ran 8 % slower, whichever precision mode it used).
_SIDE_STREAMS = {}
# priorities of the side streams: the virtual-node chain is short and latency-bound and sits on the critical path of the
# backward (highest); the weight-gradient GEMMs are long, chip-filling and nobody waits for them (lowest)
_SIDE_LEVEL = {"vn": int(os.environ.get("GT_PRIO_VN", "-1")), "dw": int(os.environ.get("GT_PRIO_DW", "1"))}


def _side_stream(device, which):
    """a HIP stream created by the library (gt_stream_create: carries a priority); lives as long as the process"""
    key = (torch.device(device).index or 0, which)
    st = _SIDE_STREAMS.get(key)
    if st is None:
        with torch.cuda.device(device):
            st = _lib.lib().gt_stream_create(_SIDE_LEVEL.get(which, 0))
        if not st:
            raise RuntimeError("gt_stream_create failed")
        _SIDE_STREAMS[key] = st
    return st


def _image_set(imgs):
    """gt_image_set view of a w3.W3Images / W1Images object (its ctypes arrays stay owned by `imgs`)"""
    s = ImageSet()
    if imgs is None:
        return s
    s.n_jobs, s.n_bind = imgs._n, len(imgs.weights)
    for k, a in (("job_w", imgs._w), ("job_N", imgs._N), ("job_K", imgs._K), ("job_T", imgs._T), ("job_img", imgs._img),
                 ("bind_w", imgs._bw), ("bind_N", imgs._bN), ("bind_K", imgs._bK), ("bind_f", imgs._bf), ("bind_t", imgs._bt)):
        setattr(s, k, C.cast(a, _vp))
    return s


def _rehome(params):
    """Make `params` views of ONE contiguous storage, in their order (same Parameter objects, same state_dict keys;
    optim.FusedAdamW notices the move and rebuilds its tables): returns the flat storage and every parameter's offset in it."""
    with torch.no_grad():
        flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
        offs, off = [], 0
        for p in params:
            p.data = flat[off:off + p.numel()].view(p.shape)
            offs.append(off)
            off += p.numel()
    return flat, offs


PNA_TOWER_IMAGES = os.environ.get("GT_PNA_TOWER_IMAGES", "1") != "0"   # bf16x3 images of the PNA tower weights (grouped k_lin3)


# ---------------------------------------------------------------------------------------------------
# plan: a model's layout (model_layout.ModelLayout, host only) bound to its storage and to a device, built once per model
# ---------------------------------------------------------------------------------------------------
def bind_storage(lay, cm):
    """Step 2 of a plan, device-agnostic (`_rehome` and `data_ptr()` work on CPU tensors): the parameters of every storage group of
    the layout become views of one matrix, then every parameter and buffer pointer goes into `cm` and the layout's descriptors.
    ORDER: re-homing gives a parameter new storage, so a pointer read before its group is re-homed points at freed memory.  Every
    group is re-homed HERE, in this one loop, and no code reads a data_ptr() before it has run."""
    for group in lay.storage_groups:
        _rehome(group)
    lay.fill(cm)
    for desc, name, t in lay.ptrs:
        setattr(cm if desc is None else desc, name, t.data_ptr())
    for t, w in enumerate(lay.embed):
        cm.tables[t] = w.data_ptr()
    cm.conv_layers = C.cast(lay.conv_desc, _vp) if lay.conv_desc is not None else None
    cm.vn = C.cast(lay.vn_desc, _vp) if (lay.has_vn and lay.L > 1) else None
    cm.enc = C.cast(lay.enc_desc, _vp) if lay.enc_layers else None


class _Plan(ModelLayout):
    """A layout IS the plan's base class: everything the per-step path reads stays a plain attribute of the plan object."""
    def __init__(self, model):
        from . import w3
        _check_abi()
        lib = _lib.lib()
        super().__init__(model)   # step 1: the layout (host only)
        cm = self.cm = ModelDesc()
        bind_storage(self, cm)    # step 2: storage
        # ---- step 3: device resources
        self.dev = next(model.parameters()).device
        self._cache = {}   # per batch size: small index arrays
        self.pe_ptr = self.pe.data_ptr() if self.pe is not None else 0
        cm.vn_defer_dw = int(VN_DEFER_DW)
        tower_views = self._bind_pna_images() if self.kind == "pna" else []
        # persistent flat gradient buffer and its per-parameter views
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=self.dev)
        self.views = [self.flat[o:o + p.numel()].view(p.shape) for p, o in self.params]
        self.flat2 = None   # flat_accum: made by the first accumulating backward of a `fused_flag` model
        self.plist = [p for p, _ in self.params]
        self.param_ptrs = tuple(p.data_ptr() for p in self.plist)
        self.frozen = None   # set_frozen: which parameters the backward hands gradients to
        self.zero_i64 = torch.zeros(1, dtype=torch.int64, device=self.dev)
        cm.zero_i64 = self.zero_i64.data_ptr()
        # streams: the virtual-node update of layer l only feeds layer l+1 (second stream beside layer l's conv / BatchNorm +
        # aggregate backward); the weight-gradient GEMMs run on a third stream beside the dX chain; the graph structure on a fourth
        self.side = _side_stream(self.dev, "vn") if (self.has_vn and OVERLAP_VN) else None
        self.side_dw = _side_stream(self.dev, "dw") if OVERLAP_DW else None
        self.side_prep = _side_stream(self.dev, "prep") if PREP_OVERLAP else None
        cm.st_vn, cm.st_dw, cm.st_prep = self.side, self.side_dw, self.side_prep
        self._events = []

        def ev():
            e = lib.gt_event_create()
            self._events.append(e)
            return e
        with torch.cuda.device(self.dev):
            for l in range(self.L):
                cm.ev_x[l], cm.ev_vn[l], cm.ev_dvn[l], cm.ev_extra[l], cm.ev_pool[l] = ev(), ev(), ev(), ev(), ev()
            cm.ev_vnemb, cm.ev_prep_begin, cm.ev_graph, cm.ev_w1 = ev(), ev(), ev(), ev()
            cm.ev_sort[0], cm.ev_sort[1], cm.ev_wt[0], cm.ev_wt[1] = ev(), ev(), ev(), ev()
        self._set_min_elems()
        # ---- weight images: bf16x3 (fp32-accurate big-M GEMMs on the bf16 pipe, csrc/linear3x.h) and fragment-order bf16 (encoder
        # layers, csrc/linear1.h); rebuilt by the driver at every forward (the optimizer changed the weights: one launch each), bound
        # per host thread inside the driver.  A weight list beyond the bind tables' 64 entries keeps the exact / tiled kernels.
        self.w3_weights = self.w3_weights + tower_views + self.w3_tail
        self.imgs3 = self.imgs3e = self.imgs1 = None
        if w3.ENABLED:
            if self.w3_weights and len(self.w3_weights) <= W_MAX_BOUND:   # (none: the encoder-only mode with a table or a re-pitched encoder)
                self.imgs3 = w3.W3Images(self.w3_weights)
            if self.w3_enc_weights and len(self.w3_weights) + len(self.w3_enc_weights) <= W_MAX_BOUND:
                self.imgs3e = w3.W3Images(self.w3_weights + self.w3_enc_weights)
        if w3.W1_ENABLED and self.w3_enc_weights and len(self.w3_enc_weights) <= W_MAX_BOUND:
            self.imgs1 = w3.W1Images(self.w3_enc_weights)
        cm.w3, cm.w3_enc, cm.w1 = _image_set(self.imgs3), _image_set(self.imgs3e), _image_set(self.imgs1)
        self.ctx_bytes = int(lib.gt_model_ctx_bytes())
        lo, hi = (_i64 * 3)(), (_i64 * 3)()
        _lib.check(lib.gt_model_grad_ranges(C.byref(cm), lo, hi), "gt_model_grad_ranges")
        self.ranges = list(zip(lo, hi))
        self.cm_ref = C.byref(cm)
        # range 0 -- what stage 1 of the backward completes -- holds every parameter outside gnn_node and nothing else
        # (encoder-only mode: what lies below the tail is the input encoder, and there is no frozen pattern)
        tail = self.ranges[0][0]
        gnn, _, ne = model_parts(model)
        gnn_ids = {id(p) for p in (gnn if gnn is not None else ne).parameters()}
        self.gnn_plist = [p for p, o in self.params if o < tail]
        self.tail_outside_gnn = {id(p) for p in self.gnn_plist} == gnn_ids
        self.set_frozen(gnn is not None and frozen_pattern(model) == "gnn")

    def _bind_pna_images(self):
        """the PNA tower images (model_layout.pna_maps) on the device, the descriptors' pointers into them, and -- where they fit
        the bind table -- the views of the image buffer that get bf16x3 images too (returned)"""
        cm, L, T, F, S, K = self.cm, self.L, self.pna_T, self.pna_F, self.pna_S, self.pna_K
        self.pna_map = torch.from_numpy(self.pna_map_np.astype(np.int32)).to(self.dev)
        self.pna_inv = torch.from_numpy(self.pna_inv_np.astype(np.int32)).to(self.dev)
        self.pna_img = torch.zeros(self.pna_map_np.size, dtype=torch.float32, device=self.dev)
        base = self.pna_img.data_ptr()
        cm.pna_img, cm.pna_map, cm.pna_inv = base, self.pna_map.data_ptr(), self.pna_inv.data_ptr()
        for l in range(L):
            desc = self.conv_desc[l]
            desc.pre_w, desc.pre_b, desc.post_w, desc.post_b = (base + 4 * o for o in cm.pna_img_off[l])
        # the towers' re-stacked matrices get bf16x3 images too (grouped k_lin3: the T GEMMs of a tower stack in one launch on the
        # bf16 matrix pipe at fp32 accuracy); views of pna_img, whose contents the driver gathers before it builds the images
        views = []
        if PNA_TOWER_IMAGES:
            for l in range(L):
                for j, (rows_, cols_) in ((0, (2 * F, F)), (2, (S * F, (1 + K) * F))):
                    o0 = int(cm.pna_img_off[l][j])
                    views += [self.pna_img[o0 + t * rows_ * cols_:o0 + (t + 1) * rows_ * cols_].view(rows_, cols_) for t in range(T)]
            # the bind table holds W_MAX_BOUND weights: when the tower views would overflow it they are the ones left out (the towers
            # then run the exact-fp32 tiled kernels) -- NOT every image of the model (the whole set silently fell back)
            if len(self.w3_weights) + len(views) + 2 > W_MAX_BOUND:   # (+ gnn2transformer, + a Linear node encoder)
                import warnings
                warnings.warn("graphtrans_amd: %d PNA tower matrices do not fit the library's %d-entry weight-image table beside the "
                              "model's other weights: the towers run on the exact-fp32 kernels" % (len(views), W_MAX_BOUND))
                views = []
        return views

    def set_frozen(self, frozen):
        """The part of the plan that follows `requires_grad`: with gnn_node frozen the backward is stage 1 alone (gt_model_batch::
        gnn_frozen) and only range 0 of the flat buffer -- the parameters outside gnn_node -- is handed out as `.grad`.  The flat
        layout, the offsets and the parameters' storage stay as they are."""
        if frozen and not self.tail_outside_gnn:
            raise RuntimeError("graphtrans_amd.engine: the gradient buffer's tail does not hold exactly the parameters outside gnn_node")
        self.frozen = bool(frozen)
        lo = self.ranges[0][0] if self.frozen else 0
        self.tparams = [(p, o) for p, o in self.params if o >= lo]
        self.tlist = [p for p, _ in self.tparams]
        self.tviews = [v for (_, o), v in zip(self.params, self.views) if o >= lo]
        self.trigger = self.tlist[0]   # what the autograd node hangs on: a parameter that requires grad (frozen: gnn2transformer.weight)

    def flat_accum(self):
        """The second persistent flat gradient buffer (`model.fused_flag`): a backward that accumulates writes it, one add folds it into
        `flat`.  Zero-filled once: the floats between the parameters' ranges, which no kernel writes, stay zero in both."""
        if self.flat2 is None:
            self.flat2 = torch.zeros_like(self.flat)
        return self.flat2

    def _set_min_elems(self):
        self.min_elems = DW_OVERLAP_MIN_ELEMS
        self.cm.dw_overlap_min_elems = DW_OVERLAP_MIN_ELEMS

    def __del__(self):
        try:
            lib = _lib.lib()
            for e in self._events:
                lib.gt_event_destroy(e)
        except Exception:
            pass

    def small(self, B):
        c = self._cache.get(B)
        if c is None:
            z = torch.zeros(B, dtype=torch.int32, device=self.dev)
            i = torch.arange(B, dtype=torch.int32, device=self.dev)
            p = torch.tensor([0, B], dtype=torch.int32, device=self.dev)
            c = self._cache[B] = (z, i, p, z.data_ptr(), i.data_ptr(), p.data_ptr())
        return c


# Per-model engine state (plan with its ctypes descriptors / HIP events / streams, eligibility cache, attached
# GradSync) lives OUTSIDE the module: nothing unpicklable ends up in `model.__dict__`, so copy.deepcopy(model),
# torch.save(model) and EMA snapshots keep working after the first fused forward, and a copy builds its own plan.
_STATE = weakref.WeakKeyDictionary()


def state(model):
    st = _STATE.get(model)
    if st is None:
        st = _STATE[model] = {}
    return st


def invalidate(model):
    """Forget the cached plan / eligibility of `model` (parameters were frozen, replaced or re-registered)."""
    st = _STATE.get(model)
    if st is not None:
        st.pop("plan", None)
        st.pop("eligible", None)
        st.pop("params", None)
        st.pop("bn_sync", None)
        st.pop("bn_hook", None)


def _bn_sync_hook(model, plan):
    """dist.BnSyncHook of a model whose BatchNorms are synchronised (modules/norm.py:convert_sync_batchnorm), else None"""
    from .modules.norm import BatchNorm1d, any_sync
    st = state(model)
    if "bn_sync" not in st:
        bns = [m for m in model.modules() if isinstance(m, BatchNorm1d)]
        st["bn_sync"] = bns[0].sync_group if (bns and any_sync(*bns)) else False
    grp = st["bn_sync"]
    if grp is False:
        return None
    hook = st.get("bn_hook")
    if hook is None:
        from .dist import BnSyncHook
        hook = st["bn_hook"] = BnSyncHook(grp)
    return hook


def _plan(model):
    st = state(model)
    plan = st.get("plan")
    pe = getattr(model, "pos_encoder", None)   # (a buffer moves with .to() like the parameters)
    if plan is None or plan.param_ptrs != tuple(p.data_ptr() for p in plan.plist) or plan.pe_ptr != (pe.pe.data_ptr() if pe is not None else 0):
        plan = st["plan"] = _Plan(model)
    # `eligible` lets through "all trainable" and "exactly gnn_node frozen": one flag tells them apart.  Looked at on every call: a
    # freeze (or an un-freeze) by hand after a warm-up forward reaches no callback
    frozen = not plan.gnn_plist[0].requires_grad
    if frozen != plan.frozen:
        plan.set_frozen(frozen)
    return plan


def eligible(model, batched_data, perturb):
    """True when the fused path covers this model / call (the static part is cached per model and mode)."""
    if not getattr(model, "fused", True):
        return False
    gnn, _, ne = model_parts(model)
    if gnn is None and not _enc_only_call_ok(model, ne, perturb):
        return False
    # a perturbation (FLAG: forward(batched_data, perturb)) sends the model to the module path, unless `model.fused_flag` asks for the
    # fused step with it (`_perturb_ok`): opt-in, like `fused_freeze`
    if perturb is not None and not _perturb_ok(model, batched_data, perturb):
        return False
    # the fused node differentiates EVERY parameter and assigns `.grad` itself: any frozen parameter (epoch_callback's freeze_gnn,
    # or a user's requires_grad_(False) on any submodule), any tensor hook on a parameter and a DistributedDataParallel wrapper send
    # the model through the module path.  The one exception is opt-in (`model.fused_freeze`): with exactly gnn_node frozen
    # (`frozen_pattern` == "gnn") the node differentiates the parameters outside it and leaves gnn_node's `.grad` alone.
    # All three are looked at on EVERY call (a model may be wrapped or hooked after its first
    # fused forward): flags and hooks by one pass over the parameters, the wrapper through a flag that torch's module-registration
    # hook sets at the moment a DistributedDataParallel takes the model as its `.module` (`_note_ddp_wrapper`).
    st = state(model)
    plist = st.get("params")
    if plist is None:
        plist = st["params"] = list(model.parameters())
    flags = _grad_flags(plist)
    if flags is None:
        return False
    w = st.get("ddp_wrapper")   # set by the module-registration hook below when a DistributedDataParallel adopts this model
    if w is not None:
        if w() is not None:
            return False
        st["ddp_wrapper"] = None   # the wrapper is gone
    if perturb is not None and not all(flags):   # (no frozen pattern with a perturbation: the driver rejects perturb + gnn_frozen)
        return False
    key = (model.training, torch.is_grad_enabled(), tuple(flags), bool(getattr(model, "fused_freeze", False)),
           bool(getattr(model, "fused_flag", False)))
    cache = st.setdefault("eligible", {})
    ok = cache.get(key)
    if ok is None:
        ok = cache[key] = _eligible_static(model)
    if not ok:
        return False
    pos = getattr(model, "pos_encoder", None)
    if pos is not None and not (pos.dropout.p == 0 and pos.pe.is_cuda and pos.pe.dtype == torch.float32 and pos.pe.is_contiguous()):
        return False   # (changed since the static answer was cached: the module path raises GNNTransformer._packed_pe's message)
    x = batched_data.x
    kind, tabs, _ = input_encoder(ne)
    if kind == "linear":
        # (features that require a gradient go through the module path: the fused node only differentiates parameters)
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == ne.in_features
                and not x.requires_grad and getattr(batched_data, "node_depth", None) is None):
            return False
    else:
        if not (x.is_cuda and x.dtype == torch.int64 and x.dim() == 2):
            return False
        if kind == "ast":   # ASTNodeEncoder reads columns 0, 1 of x and node_depth (dataset/utils.py:28-30)
            nd = getattr(batched_data, "node_depth", None)
            if x.shape[1] < 2 or nd is None or nd.numel() != x.shape[0]:
                return False
        elif x.shape[1] != len(tabs):
            # e.g. the reference's `--feature simple` (dataset/mol.py:65-69) slices x to 2 columns: the fused kernels
            # index one column per table, so a different column count goes through the module path
            return False
    if gnn is None or hasattr(gnn, "layers"):   # no message passing / PNANodeEmbedding: no edge features on the path (modules/pna/pna_module.py:73)
        return True
    # edge features: the aggregate kernels read `edge_cols` values per edge at that pitch
    mode, edge = edge_encoder(gnn.convs[0])
    ea = getattr(batched_data, "edge_attr", None)
    if mode == "tables":
        if ea is None or ea.dim() != 2 or ea.shape[1] != len(edge) or ea.dtype != torch.int64 or not ea.is_cuda:
            return False
    elif mode == "linear":
        if ea is None or ea.dim() != 2 or ea.shape[1] != edge[0].shape[1] or not ea.is_cuda or not ea.is_floating_point():
            return False
    return True


def _enc_only_call_ok(model, ne, perturb):
    """what `models.transformer.Transformer` asks of a call beside everything `eligible` asks of every model: the model opted in
    (`model.fused_step`, off by default), no attached active dist.GradSync (data parallelism stays on the module path for this model,
    DESIGN.md section 10), and a perturbation only with a table encoder (the driver refuses it with the Linear encoder)"""
    if not getattr(model, "fused_step", False):
        return False
    sync = state(model).get("sync")
    if sync is not None and sync.active:
        return False
    return perturb is None or input_encoder(ne)[0] != "linear"


def _perturb_ok(model, batched_data, perturb):
    """what the fused step asks of a call with a perturbation, beside everything it asks without one: the model opted in
    (`model.fused_flag`, --fused_flag), the perturbation is what the kernels read -- contiguous fp32 [N, gnn_emb_dim] on the device --
    and no dist.GradSync reduces this model's gradients (FLAG under data parallelism accumulates m backwards before one reduction:
    the module path)."""
    if not getattr(model, "fused_flag", False):
        return False
    if not (torch.is_tensor(perturb) and perturb.is_cuda and perturb.dtype == torch.float32 and perturb.dim() == 2
            and perturb.is_contiguous() and perturb.data_ptr() % 16 == 0):
        return False
    sync = state(model).get("sync")
    if sync is not None and sync.active:
        return False
    try:
        return tuple(perturb.shape) == (int(batched_data.batch.numel()), emb_dim(model))
    except Exception:
        return False


def _grad_flags(params):
    """requires_grad of every parameter in one pass -- or None when one of them carries a tensor hook (register_hook /
    register_post_accumulate_grad_hook): the fused node assigns `.grad` itself and would never fire it."""
    flags = []
    for p in params:
        if p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
            return None
        flags.append(p.requires_grad)
    return flags


def has_grad_hooks(model):
    """Tensor hooks on parameters: see `_grad_flags`."""
    return _grad_flags(model.parameters()) is None


def wrapped_in_ddp(model):
    """True when `model` is the `.module` of a live torch DistributedDataParallel instance.  DDP reduces gradients from hooks on the
    parameters' AccumulateGrad nodes (C++ side, invisible from here), which a node that assigns `.grad` directly never reaches:
    such a model runs the module-by-module path (autograd accumulates as usual), or -- the supported way -- uses
    graphtrans_amd.dist.GradSync, whose all-reduce the fused backward issues itself."""
    w = state(model).get("ddp_wrapper")
    return w is not None and w() is not None


def _note_ddp_wrapper(parent, name, child):
    """torch.nn module-registration hook (fires on `parent.<name> = child`, i.e. inside DistributedDataParallel.__init__): remember
    the wrapper -- weakly -- in the wrapped model's state.  Exact and free on the step (the previous detection compared
    sys.getrefcount(model) between calls, which any extra reference -- a list, a closure, a debugger -- triggered or hid)."""
    if name == "module" and isinstance(child, torch.nn.Module):
        from torch.nn.parallel import DistributedDataParallel
        if isinstance(parent, DistributedDataParallel):
            state(child)["ddp_wrapper"] = weakref.ref(parent)
    return None


torch.nn.modules.module.register_module_module_registration_hook(_note_ddp_wrapper)


def _eligible_static(model):
    """The static half of `eligible`: what the module tree says (model_layout.structural_ok: the same for a CPU model), then where the
    parameters live and the library's own question.  THE one blanket `except`: a model that is none of the families is not eligible."""
    try:
        return structural_ok(model) and _placement_ok(model)
    except Exception:
        return False


def _placement_ok(model):
    """every parameter a contiguous fp32 tensor on the device, and a head dim the library's attention kernels take"""
    enc = model_parts(model)[1]
    head_dim_ok = getattr(_lib.lib(), "gt_attn_head_dim_ok", None)   # (None: an A/B library of an earlier revision, GT_LIB_PATH)
    if enc is not None and head_dim_ok is not None and not head_dim_ok(GT_F32, enc.d_model, enc.nhead):
        return False   # (the module path raises the library's own message)
    return all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in model.parameters())


def _eligible_static_enc_only(model):
    """`_eligible_static` of a `models.transformer.Transformer` (the driver's encoder-only mode); False for every other model"""
    return _eligible_static(model) and model_parts(model)[0] is None


# ---------------------------------------------------------------------------------------------------
# the autograd node
# ---------------------------------------------------------------------------------------------------
def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def _num_graphs(batched_data, sizes):
    ng = getattr(batched_data, "_num_graphs", None)
    if ng is None and sizes is None and hasattr(type(batched_data), "num_graphs"):
        try:
            ng = batched_data.num_graphs
        except Exception:
            ng = None
    if ng is None:
        ng = len(sizes) if sizes is not None else int(batched_data.batch[-1].item()) + 1   # (device sync: the reference's own, gnn_module.py:195)
    return int(ng)


class _FusedModel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trigger, model, batched_data, plan, perturb=None):
        from . import ops
        lib = _lib.lib()
        cm = plan.cm
        if plan.min_elems != DW_OVERLAP_MIN_ELEMS:
            plan._set_min_elems()
        gnn, enc, _ = model_parts(model)
        training = bool(model.training)
        bt = BatchDesc()
        x, batch = batched_data.x, batched_data.batch
        N = int(batch.numel())
        keep = [x, batch]
        gs = getattr(batched_data, "_gt_structure", None)   # built earlier by the module path (modules/gnn_module.py:batch_structure): reused
        sizes = getattr(batched_data, "_sizes", None)
        if gs is not None:
            if gs.ready_event is not None:
                _call("gt_stream_wait_event", _stream(), gs.ready_event)
                gs.ready_event = None
            E, B = gs.E, gs.B
            for k in ("graph_ptr", "node_graph", "in_ptr", "in_src", "in_eid", "out_ptr", "out_dst", "out_eid", "deg", "dis"):
                setattr(bt, k, getattr(gs, k).data_ptr())
            keep.append(gs)
            if sizes is None:
                sizes = gs._sizes
            lay = None if plan.readout else gs._layouts.get(("packed", int(enc.max_input_len), enc.cls_embedding is not None))
            if lay is not None:
                bt.seq_desc, bt.last_rows = lay.desc.data_ptr(), lay.last_rows.data_ptr()
                work = getattr(lay, "work", None)
                bt.work_items = work.data_ptr() if work is not None else None
                bt.rows, bt.max_npos, bt.num_work, bt.lay_exact = lay.rows, lay.max_npos, getattr(lay, "num_work", 0), int(lay.exact)
                if lay.exact:   # S for the positional encoding: a host value, or meta[3] of the device-built layout
                    bt.lay_S = int(lay.S)
                else:
                    bt.lay_meta = lay.meta.data_ptr()
                keep.append(lay)
        elif plan.enc_only:   # the batch's edges are not this model's input: the driver builds graph_ptr / node_graph from `batch` alone
            if batch.dtype != torch.int64:
                raise TypeError("batch must be int64 (PyG collation dtype)")
            batch = batch.contiguous()
            E, B = 0, _num_graphs(batched_data, sizes)
            bt.batch = batch.data_ptr()
            keep.append(batch)
        else:
            ei = batched_data.edge_index
            if ei.dtype != torch.int64 or batch.dtype != torch.int64:
                raise TypeError("edge_index and batch must be int64 (PyG collation dtype)")
            ei, batch = ei.contiguous(), batch.contiguous()
            E, B = int(ei.shape[1]), _num_graphs(batched_data, sizes)
            bt.edge_index, bt.batch = ei.data_ptr(), batch.data_ptr()
            keep += [ei, batch]
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, dtype=np.int64)
            if sizes.size != B:
                raise ValueError("per-graph sizes do not match the number of graphs")
            bt.sizes_host = sizes.ctypes.data
        bt.N, bt.E, bt.B = N, E, B
        # ---- inputs
        if plan.embed_kind == "linear":
            x = x.contiguous()
            bt.x = x.data_ptr()
            keep.append(x)
        else:
            bt.x, bt.x_stride0, bt.x_stride1 = x.data_ptr(), x.stride(0), x.stride(1)
            if plan.embed_kind == "ast":
                depth = batched_data.node_depth.reshape(-1)
                bt.node_depth, bt.depth_stride = depth.data_ptr(), (depth.stride(0) if N > 1 else 1)
                keep.append(depth)
        ea = getattr(batched_data, "edge_attr", None)
        mode0 = plan.conv_desc[0].edge_mode if (plan.kind != "pna" and not plan.enc_only) else GT_EDGE_NONE
        if mode0 == GT_EDGE_LINEAR:
            ea = ea if (ea.dtype == torch.float32 and ea.is_contiguous()) else ea.float().contiguous()
        elif mode0 == GT_EDGE_TABLES:
            if ea.dtype != torch.int64:
                raise TypeError("embedding-table edge encoders need int64 edge_attr")
            ea = ea.contiguous()
        if mode0 != GT_EDGE_NONE:
            bt.edge_attr = ea.data_ptr()
            keep.append(ea)
        if plan.has_vn:
            sm = plan.small(B)
            bt.zeros_B, bt.ident_B, bt.ptr01 = sm[3], sm[4], sm[5]
        # compute type of the fp32-stored GEMMs (message passing, gnn2transformer, heads): exact-fp32 MFMA or bf16 MFMA
        # (ops.set_matmul_dtype); the encoder layers compute in bf16 whenever their token rows are stored in bf16
        # (layers.hip: dtype == bf16 ? bf16 : compute), i.e. (fp32, bf16 tokens) is the mixed mode of bench.py
        bf16_mm = ops.get_matmul_dtype() == torch.bfloat16
        tok_bf16 = enc is not None and enc.compute_dtype == torch.bfloat16   # (read-out mode: no token rows; everything is fp32-stored)
        # (ops.set_matmul_precision is read here, at every forward; the prepared context carries it to this forward's backward)
        bt.training, bt.compute, bt.tdt = int(training), ops.f32_compute_code(), (GT_BF16 if tok_bf16 else GT_F32)
        will_bwd = bool(ctx.needs_input_grad[0])
        bt.will_bwd = int(will_bwd)
        # exact-fp32 GEMM mode: the big-M linears run as bf16x6 on the bf16 matrix pipe on images of their weights; bf16 token rows:
        # the encoder layers' GEMMs run with the weight stationary in registers on fragment-order images
        if not bf16_mm and N >= 1024:
            if tok_bf16:
                bt.use_w3 = 1 if plan.imgs3 is not None else 0
            else:
                bt.use_w3 = 2 if plan.imgs3e is not None else (1 if plan.imgs3 is not None else 0)
        bt.use_w1 = int(tok_bf16 and plan.imgs1 is not None)
        # dropout seeds: drawn in the module path's order (GNN first, then the encoder)
        from .modules.gnn_module import _gnn_seed
        if gnn is not None:
            bt.gnn_seed = _gnn_seed(gnn) & 0xFFFFFFFFFFFFFFFF
            bt.gnn_p = float(gnn.drop_ratio) if training else 0.0
        enc_p = float(enc.dropout_p) if enc is not None else 0.0
        bt.enc_p = enc_p if training else 0.0
        bt.enc_seed = (int(torch.empty((), dtype=torch.int64).random_().item()) & 0xFFFFFFFFFFFFFFFF) if (training and enc_p > 0) else 0
        hook = _bn_sync_hook(model, plan) if training else None
        bt.sync_bn = int(hook is not None)
        bt.gnn_frozen = int(plan.frozen)
        # the perturbation (`eligible` checked it: contiguous fp32 [N, D] on the device).  Its gradient is d h_list[0], which the
        # backward writes straight into a buffer of ours when somebody will ask for it; otherwise the forward only adds
        d_perturb = None
        if perturb is not None:
            bt.perturb = perturb.data_ptr()
            keep.append(perturb)
            if will_bwd and ctx.needs_input_grad[4]:
                d_perturb = _d_perturb_buffer(N, int(plan.cm.D), plan.dev)
                bt.d_perturb = d_perturb.data_ptr()
        cbuf = C.create_string_buffer(plan.ctx_bytes)
        sz = SizesDesc()
        if plan.readout:   # no token layout: no staging ring
            _lib.check(lib.gt_model_prepare(plan.cm_ref, C.byref(bt), cbuf, C.byref(sz)), "gt_model_prepare")
        else:
            ring = stage_ring(plan.dev)   # (the driver takes a slot of it for a host-built token layout)
            bt.ring = C.addressof(ring.desc)
            with ring.lock:
                _lib.check(lib.gt_model_prepare(plan.cm_ref, C.byref(bt), cbuf, C.byref(sz)), "gt_model_prepare")
        arena = (torch.empty if sz.exact else torch.zeros)(sz.arena_bytes, dtype=torch.uint8, device=plan.dev)
        logits = torch.empty((B, plan.ldy), dtype=torch.float32, device=plan.dev)
        if hook is not None:
            hook.install()
        try:
            _lib.check(lib.gt_model_forward(plan.cm_ref, cbuf, arena.data_ptr(), logits.data_ptr(), _stream()), "gt_model_forward")
        finally:
            if hook is not None:
                hook.uninstall()
                if hook.error is not None:
                    e, hook.error = hook.error, None
                    raise e
        if will_bwd:
            ctx.state = (plan, cbuf, arena, int(sz.barena_bytes), bool(sz.exact), keep, state(model).get("sync"), hook, B,
                         (plan.frozen, plan.tparams, plan.tlist, plan.tviews), d_perturb, bool(getattr(model, "fused_flag", False)))
        else:
            ctx.state = None
        ctx.set_materialize_grads(False)
        return logits[:, :plan.Nh] if plan.ldy != plan.Nh else logits

    @staticmethod
    def backward(ctx, dlogits):
        s = ctx.state
        if s is None:
            raise RuntimeError("graphtrans_amd fused model: backward through the graph a second time "
                               "(the saved activations are freed after the first backward)")
        if dlogits is None:
            return None, None, None, None, None
        plan, cbuf, arena, barena_bytes, exact, _keep, model_sync, hook, B, (frozen, tparams, plist, tviews), d_perturb, flag = s
        from . import ops
        lib = _lib.lib()
        dl = dlogits.reshape(B, plan.Nh)
        if dl.dtype != torch.float32:
            dl = dl.to(torch.float32)
        dl = ops._padded_rows(dl, plan.ldy) if plan.ldy != plan.Nh else dl.contiguous()
        # gradients: straight into the persistent flat buffer when nothing has to be accumulated
        # (over the parameters this backward differentiates: all of them, or those outside a frozen gnn_node -- as the forward found
        # them: the prepared context carries the flag, a freeze between forward and backward changes nothing, as under autograd)
        direct = True
        for p in plist:
            if p.grad is not None:
                direct = False
                break
        # `model.fused_flag` only: a backward that finds every `.grad` still the plan's own view (FLAG's second and third backward of a
        # batch) writes a second persistent flat buffer and accumulates with ONE add onto the first; the `.grad` objects stay the views
        accum = flag and not direct and _grads_are_views(plist, tviews)
        if accum:
            flat = plan.flat_accum()
        else:
            flat = plan.flat if direct else torch.empty_like(plan.flat)
        barena = (torch.empty if exact else torch.zeros)(barena_bytes, dtype=torch.uint8, device=plan.dev)
        st = _stream()
        args = (plan.cm_ref, cbuf, dl.data_ptr(), flat.data_ptr(), barena.data_ptr())
        sync = model_sync if (direct and model_sync is not None and model_sync.active) else None
        if hook is not None:
            hook.install()
        try:
            if sync is None:
                _lib.check(lib.gt_model_backward(*args, 7, st), "gt_model_backward")
            else:
                # data parallel: each stage completes one range of the flat buffer, which goes on the wire (asynchronously, on RCCL's
                # stream) while the next stage runs: heads .. gnn2transformer | message passing | input encoder
                # (the C side keeps its overlap and deferred-reduce sections open between the stage calls on this host thread: a raise
                # from Python in between -- the collective, the BatchNorm hook -- must not leave them pointing at this step's arena)
                # (gnn_node frozen: stage 1 is the whole backward and its closing stage -- one range, one collective, no virtual-node stream)
                staged_open = False
                stages = (1,) if frozen else (1, 2, 4)
                try:
                    for i, stage in enumerate(stages):
                        staged_open = stage != stages[-1]
                        _lib.check(lib.gt_model_backward(*args, stage, st), "gt_model_backward")
                        if stage == 2 and plan.has_vn and plan.side is not None:
                            _call("gt_stream_wait_event", st, plan.cm.ev_vnemb)   # d virtualnode_embedding was reduced on the second stream
                        if stage != stages[-1]:
                            _call("gt_overlap_dw_sync")   # (the last stage joins the weight-gradient stream itself)
                        lo, hi = plan.ranges[i]
                        sync.reduce_flat(flat, lo, hi)
                    staged_open = False
                finally:
                    if staged_open:
                        lib.gt_defer_begin(None, 0)
                        lib.gt_overlap_dw_end()
        finally:
            if hook is not None:
                hook.uninstall()
                if hook.error is not None:
                    e, hook.error = hook.error, None
                    raise e
        # ---- hand the gradients to the parameters
        if direct:
            for p, v in zip(plist, tviews):
                p.grad = v
        elif accum:
            lo = plan.ranges[0][0] if frozen else 0   # (frozen: only range 0 was written, only its parameters carry a `.grad`)
            plan.flat[lo:].add_(flat[lo:])
        else:
            for p, o_ in tparams:
                v = flat[o_:o_ + p.numel()].view(p.shape)
                p.grad = v if p.grad is None else p.grad + v
        ctx.state = None
        return None, None, None, None, d_perturb


def _d_perturb_buffer(N, D, dev):
    """a fresh, uninitialised [N, D] buffer for d perturb: layer 0's input-gradient kernel overwrites every element (a function of its
    own so a test can hand out a NaN-filled one)"""
    return torch.empty((N, D), dtype=torch.float32, device=dev)


def _grads_are_views(plist, tviews):
    """every `.grad` is still the view of the plan's flat buffer that an earlier backward handed out (same storage offset, same shape)"""
    for p, v in zip(plist, tviews):
        g = p.grad
        if g is None or g.data_ptr() != v.data_ptr() or g.shape != v.shape or g.dtype != v.dtype or not g.is_contiguous():
            return False
    return True


def forward(model, batched_data, perturb=None):
    """logits (B, Nh) [row-padded storage] of the fused path; `model` must be `eligible` (with the same `perturb`)."""
    plan = _plan(model)
    if perturb is not None and not torch.is_grad_enabled():
        perturb = perturb.detach()   # (ctx.needs_input_grad follows requires_grad alone: under no_grad nobody will ask for d perturb)
    return _FusedModel.apply(plan.trigger, model, batched_data, plan, perturb)
