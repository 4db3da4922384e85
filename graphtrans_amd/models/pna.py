"""PNANet -- the PNA baseline of every GraphTrans table (models/pna.py:20-104) behind the reference's module surface: same ctor
`(num_tasks, node_encoder, edge_encoder_cls, args)`, `forward(batched_data, perturb=None)`, static `get_emb_dim / need_deg / add_args /
name`, and the same state_dict keys -- `node_encoder.*` and `pna_module.node_encoder.*` (one module, registered first as
`node_encoder`), `pna_module.layers.*`, `pna_module.batch_norms.<i>.module.*`, and `mlp.{0,2,4}.*` (max_seq_len None) or
`graph_pred_linear_list.<i>.{0,2}.*` -- so reference checkpoints load and `main.py --model_type pna` constructs it unchanged.

    pna_module -> per-graph read-out (sum | mean | max, ops.graph_pool) -> heads
      max_seq_len None : mlp = Linear(D, 35) -> ReLU -> Linear(35, 17) -> ReLU -> Linear(17, T)         ops.head_mlp   (one launch)
      max_seq_len = L  : per position Linear(D, D) -> ReLU -> Linear(D, T): the L hidden layers as ONE GEMM over their stacked weights
                         with the ReLU epilogue, the L output layers as one grouped launch into the one logits buffer  ops.head_group

forward() picks between two equivalent data paths:
  * fused  (engine.eligible: the residual connection, tower widths that are multiples of 4, every parameter trainable, no hooks / DDP
            wrapper; a perturb only with `fused_flag`; position heads: gnn_emb_dim a multiple of 16 up to 512): the whole model as one
            autograd node on the whole-model driver's read-out mode (csrc/model.hip, gt_model::readout + gt_model::head_kind);
  * module path, always available: pna_module(batched_data, perturb) -> ops.graph_pool -> heads.

One deliberate deviation from the reference, the same as `GNN`: graph_pooling "attention" / "set2set" raise
NotImplementedError (a gate MLP with a segment softmax, an LSTM: not built).
"""
import torch
import torch.nn as nn

from .. import engine, ops
from ..modules.gnn_module import batch_structure
from ..modules.pna.pna_module import PNANodeEmbedding
from .base_model import BaseModel, StackedHeads
from .gnn import POOLINGS, POOLINGS_NOT_BUILT


class PNANet(BaseModel):
    @staticmethod
    def get_emb_dim(args):
        return args.gnn_emb_dim

    @staticmethod
    def need_deg():
        return True

    @staticmethod
    def add_args(parser):
        PNANodeEmbedding.add_args(parser)

    @staticmethod
    def name(args):
        return f"{args.model_type}"

    def __init__(self, num_tasks, node_encoder, edge_encoder_cls, args):
        super().__init__()
        self.num_layer = args.gnn_num_layer
        self.num_tasks = num_tasks
        self.max_seq_len = args.max_seq_len
        self.aggregators = args.aggregators
        self.scalers = args.scalers
        self.residual = args.gnn_residual
        self.drop_ratio = args.gnn_dropout
        self.graph_pooling = args.graph_pooling
        self.emb_dim = args.gnn_emb_dim
        self.fused_flag = bool(getattr(args, "fused_flag", False))   # (engine.eligible: a perturbation on the fused step; no parser flag here)

        if self.graph_pooling in POOLINGS_NOT_BUILT:
            raise NotImplementedError(f"graph_pooling={self.graph_pooling!r} is not built here (sum, mean and max are)")
        if self.graph_pooling not in POOLINGS:
            raise ValueError("Invalid graph pooling type.")

        self.node_encoder = node_encoder
        self.pna_module = PNANodeEmbedding(node_encoder, args)

        if self.max_seq_len is None:
            self.mlp = nn.Sequential(
                nn.Linear(self.emb_dim, 35, bias=True),
                nn.ReLU(),
                nn.Linear(35, 17, bias=True),
                nn.ReLU(),
                nn.Linear(17, self.num_tasks, bias=True),
            )
        else:
            self.graph_pred_linear_list = nn.ModuleList()
            for _ in range(self.max_seq_len):
                self.graph_pred_linear_list.append(
                    nn.Sequential(nn.Linear(self.emb_dim, self.emb_dim), nn.ReLU(), nn.Linear(self.emb_dim, self.num_tasks)))

    @property
    def gnn_node(self):
        """the message-passing stack under the name the engine reads on every model"""
        return self.pna_module

    def forward(self, batched_data, perturb=None):
        if batched_data.batch.numel() == 0:
            raise ValueError("empty batch")
        if perturb is not None and perturb.shape[0] != batched_data.batch.numel():
            raise ValueError("perturb must have one row per node")
        if engine.eligible(self, batched_data, perturb):   # whole model as one autograd node (engine.py)
            out = engine.forward(self, batched_data, perturb)
            if self.max_seq_len is None:
                return out
            return StackedHeads(out.view(out.shape[0], self.max_seq_len, self.num_tasks))
        x = self.pna_module(batched_data, perturb)
        h_graph = ops.graph_pool(x.float(), batch_structure(batched_data), self.graph_pooling)
        if self.max_seq_len is None:
            return ops.head_mlp(h_graph, self.mlp[0], self.mlp[2], self.mlp[4])
        heads = list(self.graph_pred_linear_list)
        D = self.emb_dim
        if D % 16 or D > 512:   # widths the grouped kernel does not take: position by position on the tiled GEMMs, the reference's list
            return [ops.linear_module(seq[2], ops.linear_module(seq[0], h_graph, act="relu")) for seq in heads]
        hidden = ops.linear(h_graph, torch.cat([seq[0].weight for seq in heads], dim=0), torch.cat([seq[0].bias for seq in heads], dim=0),
                            act="relu")
        return ops.head_group(hidden, [seq[2] for seq in heads])
