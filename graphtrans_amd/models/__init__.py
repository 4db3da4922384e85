"""Model registry (models/__init__.py:9-15): `gnn` (the GCN / GIN baseline with a sum / mean / max read-out), `gnn-transformer`,
`pna-transformer`, `pna` (the PNA baseline with its MLP heads) and `transformer` (the plain Transformer baseline).  The reference's
`transformer-gnn` remains out (broken in the reference itself).

`pna` sits in a second table, ABLATION_MODELS, beside MODELS: the suite pins MODELS to its three keys, and the reference's driver only
calls `get_model_and_parser` (main.py:21,94), which looks in both.  `transformer` sits in a third table, BASELINE_MODELS, that
`get_model_and_parser` does NOT look in: the suite also pins that function to raise KeyError for it.  `get_model_class(model_type)`
looks in all three.  Folding the tables into one, and `transformer` into `get_model_and_parser`, is a follow-up."""
from .gnn import GNN
from .gnn_transformer import GNNTransformer
from .pna import PNANet
from .pna_transformer import PNATransformer
from .transformer import Transformer


def get_model_and_parser(args, parser):
    model_cls = MODELS[args.model_type] if args.model_type in MODELS else ABLATION_MODELS[args.model_type]
    model_cls.add_args(parser)
    return model_cls


MODELS = {"gnn": GNN, "gnn-transformer": GNNTransformer, "pna-transformer": PNATransformer}
ABLATION_MODELS = {"pna": PNANet}
BASELINE_MODELS = {"transformer": Transformer}


def get_model_class(model_type):
    """The model class of `model_type` from MODELS, ABLATION_MODELS or BASELINE_MODELS (KeyError otherwise); the caller adds its args
    (`cls.add_args(parser)`), as get_model_and_parser does for the first two tables."""
    for table in (MODELS, ABLATION_MODELS, BASELINE_MODELS):
        if model_type in table:
            return table[model_type]
    raise KeyError(model_type)
