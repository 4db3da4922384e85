"""Model registry (models/__init__.py:9-15): `gnn` (the GCN / GIN baseline with a sum / mean / max read-out), `gnn-transformer`,
`pna-transformer` and `pna` (the PNA baseline with its MLP heads).  The reference's `transformer` and `transformer-gnn` remain out.

`pna` sits in a second table, ABLATION_MODELS, beside MODELS: the suite pins MODELS to its three keys, and the reference's driver only
calls `get_model_and_parser` (main.py:21,94), which looks in both.  Folding the two tables into one is a follow-up."""
from .gnn import GNN
from .gnn_transformer import GNNTransformer
from .pna import PNANet
from .pna_transformer import PNATransformer


def get_model_and_parser(args, parser):
    model_cls = MODELS[args.model_type] if args.model_type in MODELS else ABLATION_MODELS[args.model_type]
    model_cls.add_args(parser)
    return model_cls


MODELS = {"gnn": GNN, "gnn-transformer": GNNTransformer, "pna-transformer": PNATransformer}
ABLATION_MODELS = {"pna": PNANet}
