"""Transformer — the plain Transformer baseline of the GraphTrans tables (models/transformer.py:20-115): no message passing at all,

    node encoder -> (+ perturb) -> pad -> TransformerNodeEncoder -> cls | sum | mean | max read-out -> prediction heads

behind the reference's module surface: same ctor `(num_tasks, node_encoder, edge_encoder_cls, args)`, `forward(batched_data,
perturb=None)`, static `get_emb_dim / add_args / name`, and the same state_dict keys (`node_encoder.*`, `transformer.*`,
`graph_pred_linear.*` or `graph_pred_linear_list.<i>.*`), so reference checkpoints load.

Data paths.  The module path (the default):
  * cls: the packed token layout with CLS rows.  With `fused_embed` on and ops.embed_tokens_supported (a table encoder: ASTNodeEncoder,
    AtomEncoder) the token rows come from ops.embed_tokens, which writes them straight from the embedding tables; otherwise from
    the composition node_encoder -> + perturb -> ops.seq_gather (also the nn.Linear encoder of the TU datasets).  Then
    forward_tokens(pooled=True) and the heads.
  * sum | mean | max: the reference's semantics exactly (models/transformer.py:101-107): no CLS, and after the encoder unpad_batch
    with the UN-transformed encoder output as base -- the leading nodes a truncated graph drops keep their input rows -- then
    global_*_pool over all N rows (ops.seq_scatter, ops.graph_pool).  The packed layout: padding never influences a valid row.

The fused step (opt-in: `model.fused_step = True`, or `args.fused_step`; no parser flag, like `fused_embed`; off by default): with cls
pooling the whole forward and backward run as ONE C call per direction on the whole-model driver's encoder-only mode (engine.py,
csrc/model.hip: gt_model::enc_only) whenever `engine.eligible` says yes -- a table encoder with at most 16 tables of at most 16384 rows,
or nn.Linear with a bias; every parameter trainable fp32; no tensor hooks, DDP wrapper or active dist.GradSync.  A perturbation
stays on the fused step only with `model.fused_flag` (same kind of attribute) and a table encoder: flag.flag_step then keeps all m
passes there.  Everything else -- sum | mean | max pooling, larger tables, a perturbation with the Linear encoder, any frozen
parameter -- falls through to the module path below, exactly as it runs without the attribute.  `fused_embed` has no meaning on the
fused step: the driver always writes the token rows straight from the tables.

Deviations from the reference:
  * graph_pooling "attention" / "set2set" raise NotImplementedError (not built, as in GNN);
  * any other pooling, "last" included, raises ValueError("Invalid graph pooling type.") -- as the reference does;
  * the class is reached through BASELINE_MODELS / get_model_class, not MODELS.
"""
import torch

from .. import engine, ops
from ..modules.gnn_module import _encode_nodes, batch_structure
from ..modules.transformer_encoder import TransformerNodeEncoder
from .base_model import BaseModel, StackedHeads, stacked_heads

POOLINGS = ("cls", "sum", "mean", "max")
POOLINGS_NOT_BUILT = ("attention", "set2set")
FUSED_EMBED_DEFAULT = True   # measured not slower than the composition at the Code2 and Molpcba shapes (profiles/LOG.md)


class Transformer(BaseModel):
    @staticmethod
    def get_emb_dim(args):
        return args.d_model

    @staticmethod
    def add_args(parser):
        TransformerNodeEncoder.add_args(parser)

    @staticmethod
    def name(args):
        name = f"{args.model_type}-pooling={args.graph_pooling}"
        name += f"+{args.gnn_type}"
        name += "-virtual" if args.gnn_virtual_node else ""
        name += f"-d={args.d_model}"
        name += f"-tdp={args.transformer_dropout}"
        return name

    def __init__(self, num_tasks, node_encoder, edge_encoder_cls, args):
        super().__init__()
        self.graph_pooling = args.graph_pooling
        if self.graph_pooling in POOLINGS_NOT_BUILT:
            raise NotImplementedError(f"graph_pooling={self.graph_pooling!r} is not built here (cls, sum, mean and max are)")
        if self.graph_pooling not in POOLINGS:
            raise ValueError("Invalid graph pooling type.")
        self.transformer = TransformerNodeEncoder(args)
        self.node_encoder = node_encoder
        self.emb_dim = args.d_model
        self.num_tasks = num_tasks
        self.max_seq_len = args.max_seq_len
        # token rows straight from the embedding tables (ops.embed_tokens) where the encoder is a sum of tables; off: the composition
        self.fused_embed = bool(getattr(args, "fused_embed", FUSED_EMBED_DEFAULT))
        # the whole step on the driver's encoder-only mode where engine.eligible allows it (cls pooling); `fused_flag`: with a perturbation too
        self.fused_step = bool(getattr(args, "fused_step", False))
        self.fused_flag = bool(getattr(args, "fused_flag", False))
        if self.max_seq_len is None:
            self.graph_pred_linear = torch.nn.Linear(self.emb_dim, self.num_tasks)
        else:
            self.graph_pred_linear_list = torch.nn.ModuleList()
            for _ in range(self.max_seq_len):
                self.graph_pred_linear_list.append(torch.nn.Linear(self.emb_dim, self.num_tasks))

    def _embed_columns(self, batched_data):
        """(columns, tables, clamps) when the node encoder is a sum of embedding tables, else None"""
        fn = getattr(self.node_encoder, "embed_columns", None)
        if fn is None:
            return None
        node_depth = batched_data.node_depth if hasattr(batched_data, "node_depth") else None
        return fn(batched_data.x) if node_depth is None else fn(batched_data.x, node_depth.view(-1))

    def _encoded(self, batched_data, perturb):
        h = _encode_nodes(self.node_encoder, batched_data)
        return h + perturb if perturb is not None else h

    def forward(self, batched_data, perturb=None):
        if batched_data.batch.numel() == 0:
            raise ValueError("empty batch")
        if perturb is not None and perturb.shape[0] != batched_data.batch.numel():
            raise ValueError("perturb must have one row per node")
        if self.fused_step and engine.eligible(self, batched_data, perturb):   # whole model as one autograd node (engine.py)
            out = engine.forward(self, batched_data, perturb)
            if self.max_seq_len is None:
                return out
            return StackedHeads(out.view(out.shape[0], self.max_seq_len, self.num_tasks))
        enc = self.transformer
        gs = batch_structure(batched_data)
        max_len = int(enc.max_input_len)
        if self.graph_pooling == "cls":
            lay = gs.layout("packed", max_len, True)
            tokens = None
            if self.fused_embed:
                emb = self._embed_columns(batched_data)
                if emb is not None and ops.embed_tokens_supported(emb[0], emb[1], gs, lay, enc.compute_dtype):
                    tokens = ops.embed_tokens(emb[0], emb[1], emb[2], gs, lay, cls=enc.cls_embedding, perturb=perturb,
                                              out_dtype=enc.compute_dtype)
            if tokens is None:
                tokens, _ = ops.seq_gather(self._encoded(batched_data, perturb), enc.cls_embedding, gs, lay)
            h_graph = enc.forward_tokens(tokens, lay, pooled=True).float()
        else:
            lay = gs.layout("packed", max_len, False)
            tmp = self._encoded(batched_data, perturb)
            tokens, _ = ops.seq_gather(tmp, None, gs, lay)
            out = enc.forward_tokens(tokens, lay).float()
            h_node = ops.seq_scatter(out, tmp, gs, lay)   # unpad_batch: dropped nodes keep their rows of tmp
            h_graph = ops.graph_pool(h_node, gs, self.graph_pooling)
        if self.max_seq_len is None:
            return ops.linear_module(self.graph_pred_linear, h_graph)
        return stacked_heads(h_graph, self.graph_pred_linear_list, self.num_tasks)
