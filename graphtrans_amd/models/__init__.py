"""Model registry (models/__init__.py:9-15): `gnn` (the GCN / GIN baseline with a sum / mean / max read-out), `gnn-transformer`
and `pna-transformer`.  The reference's other three entries remain out: `pna` (MLP heads), `transformer` and `transformer-gnn`."""
from .gnn import GNN
from .gnn_transformer import GNNTransformer
from .pna_transformer import PNATransformer


def get_model_and_parser(args, parser):
    model_cls = MODELS[args.model_type]
    model_cls.add_args(parser)
    return model_cls


MODELS = {"gnn": GNN, "gnn-transformer": GNNTransformer, "pna-transformer": PNATransformer}
