"""GNN — the message-passing baseline of every GraphTrans table (models/gnn.py:16-115) behind the reference's module surface:
same ctor `(num_tasks, node_encoder, edge_encoder_cls, args)`, `forward(batched_data, perturb=None)`, static
`get_emb_dim / add_args / name`, and the same state_dict keys (`gnn_node.*`, `graph_pred_linear.*` or
`graph_pred_linear_list.<i>.*`), so reference checkpoints load and `main.py --model_type gnn` constructs it unchanged.

    gnn_node -> per-graph read-out (sum | mean | max, ops.graph_pool) -> prediction heads (one GEMM over the stacked weights)

forward() picks between two equivalent data paths:
  * fused  (engine.eligible: JK = last, every parameter trainable, no hooks / DDP wrapper; a perturb only with `fused_flag`): the whole model as one
            autograd node on the whole-model driver's read-out mode (csrc/model.hip, gt_model::readout);
  * module path, always available: gnn_node(batched_data, perturb) -> ops.graph_pool -> heads.

Two deliberate deviations from the reference:
  * graph_pooling "attention" / "set2set" raise NotImplementedError (a gate MLP with a segment softmax, an LSTM: not built);
  * gnn_JK = "cat" raises ValueError in the constructor: the reference builds Linear(emb_dim, ...) heads over 2 * emb_dim wide
    node rows and fails with a shape error on its first forward.
"""
import torch

from .. import engine, ops
from ..modules.gnn_module import GNNNodeEmbedding, batch_structure
from .base_model import BaseModel, StackedHeads, stacked_heads

POOLINGS = ("sum", "mean", "max")
POOLINGS_NOT_BUILT = ("attention", "set2set")


class GNN(BaseModel):
    @staticmethod
    def get_emb_dim(args):
        return args.gnn_emb_dim

    @staticmethod
    def add_args(parser):
        return

    @staticmethod
    def name(args):
        name = f"{args.model_type}+{args.gnn_type}"
        name += "-virtual" if args.gnn_virtual_node else ""
        return name

    def __init__(self, num_tasks, node_encoder, edge_encoder_cls, args):
        super().__init__()
        self.num_layer = args.gnn_num_layer
        self.drop_ratio = args.gnn_dropout
        self.JK = args.gnn_JK
        self.emb_dim = args.gnn_emb_dim
        self.num_tasks = num_tasks
        self.max_seq_len = args.max_seq_len
        self.graph_pooling = args.graph_pooling
        self.fused_flag = bool(getattr(args, "fused_flag", False))   # (engine.eligible: a perturbation on the fused step; no parser flag here)

        if self.num_layer < 2:
            raise ValueError("Number of GNN layers must be greater than 1.")
        if self.graph_pooling in POOLINGS_NOT_BUILT:
            raise NotImplementedError(f"graph_pooling={self.graph_pooling!r} is not built here (sum, mean and max are)")
        if self.graph_pooling not in POOLINGS:
            raise ValueError("Invalid graph pooling type.")
        if self.JK == "cat":
            raise ValueError("gnn_JK='cat' does not fit the GNN model: its heads are Linear(gnn_emb_dim, num_tasks) while the "
                             "concatenated node rows are 2 * gnn_emb_dim wide")

        self.gnn_node = GNNNodeEmbedding(args.gnn_virtual_node, self.num_layer, self.emb_dim, node_encoder, edge_encoder_cls,
                                         JK=self.JK, drop_ratio=self.drop_ratio, residual=args.gnn_residual,
                                         gnn_type=args.gnn_type)
        if self.max_seq_len is None:
            self.graph_pred_linear = torch.nn.Linear(self.emb_dim, self.num_tasks)
        else:
            self.graph_pred_linear_list = torch.nn.ModuleList()
            for _ in range(self.max_seq_len):
                self.graph_pred_linear_list.append(torch.nn.Linear(self.emb_dim, self.num_tasks))

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
        h_node = self.gnn_node(batched_data, perturb)
        h_graph = ops.graph_pool(h_node.float(), batch_structure(batched_data), self.graph_pooling)
        if self.max_seq_len is None:
            return ops.linear_module(self.graph_pred_linear, h_graph)
        return stacked_heads(h_graph, self.graph_pred_linear_list, self.num_tasks)
