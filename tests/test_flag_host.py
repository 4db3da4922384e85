"""FLAG on the fused step, host side (no GPU): the --fused_flag flag of the two transformer parsers and the three constructors, the
`perturb` / `d_perturb` tail of the driver's batch struct, the two new entry points, and what gt_model_prepare rejects."""
import argparse
import ctypes as C

import pytest

from test_frozen_gnn_host import BUILDERS
from test_gnn_baseline_host import INVALID, _args, _build, _driver_batch, _driver_model, _prepare


def test_parsers_accept_fused_flag():
    from graphtrans_amd.models.gnn import GNN
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from graphtrans_amd.models.pna_transformer import PNATransformer
    for cls in (GNNTransformer, PNATransformer):
        parser = argparse.ArgumentParser(conflict_handler="resolve")
        cls.add_args(parser)
        a = parser.parse_args([])
        assert a.fused_flag is False and a.fused_freeze is False
        a = parser.parse_args(["--fused_flag"])
        assert a.fused_flag is True and a.fused_freeze is False
    parser = argparse.ArgumentParser()
    GNN.add_args(parser)   # empty, as in the reference: the flag reaches a GNN through its args object only
    assert vars(parser.parse_args([])) == {}


@pytest.mark.parametrize("kind", ["gnn", "pna"])
def test_transformers_read_fused_flag(kind):
    build = BUILDERS[kind]
    assert build().fused_flag is False
    assert build(fused_flag=True).fused_flag is True
    assert build(fused_flag=True).fused_freeze is False


def test_gnn_baseline_reads_fused_flag():
    assert _build(_args()).fused_flag is False
    assert _build(_args(fused_flag=True)).fused_flag is True


def test_batch_struct_ends_with_perturb_and_its_gradient():
    from graphtrans_amd import _lib, engine
    names = [f[0] for f in engine.BatchDesc._fields_]
    assert names[-4:] == ["lay_S", "lay_meta", "perturb", "d_perturb"]
    assert engine.BatchDesc.perturb.offset == engine.BatchDesc.lay_meta.offset + 8
    assert engine.BatchDesc.d_perturb.offset == engine.BatchDesc.perturb.offset + 8
    assert C.sizeof(engine.BatchDesc) == engine.BatchDesc.d_perturb.offset + 8
    out = (C.c_int64 * 4)()
    assert _lib.lib().gt_model_abi_sizes(out) == 0
    assert out[0] == C.sizeof(engine.ModelDesc) and out[1] == C.sizeof(engine.BatchDesc)
    engine._ABI_OK.clear()
    engine._check_abi()
    bt = engine.BatchDesc()
    assert bt.perturb is None and bt.d_perturb is None   # a zeroed struct is a call without a perturbation


def test_new_symbols_are_declared_and_exported():
    from graphtrans_amd import _lib, build
    L = _lib.lib()
    for name, nargs in (("gt_embed_sum_fwd_add", 11), ("gt_flag_ascent", 5)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    # gt_embed_sum_fwd keeps its signature: the same arguments but for the row operand and its index
    add, plain = _lib.SIGNATURES["gt_embed_sum_fwd_add"][1], _lib.SIGNATURES["gt_embed_sum_fwd"][1]
    assert add[:5] + add[7:] == plain
    assert "flag.hip" in build.SOURCES


def test_flag_ascent_rejects_a_count_that_is_no_multiple_of_4_on_the_host():
    from graphtrans_amd import _lib
    L = _lib.lib()
    assert L.gt_flag_ascent(0x10000, 0x20000, 6, 0.5, None) == -2   # GT_ERR_UNSUPPORTED, before anything is launched
    assert b"multiple of 4" in L.gt_last_error()
    assert L.gt_flag_ascent(0x10000, 0x20000, 0, 0.5, None) == 0    # nothing to do


def _prepared(change):
    cm, keep = _driver_model()
    bt, sizes = _driver_batch()
    change(bt)
    rc, sz, err = _prepare(cm, bt)
    return rc, err


FAKE_P, FAKE_D = 0xA0000, 0xB0000


def test_prepare_accepts_a_perturbation():
    def both(bt):
        bt.perturb, bt.d_perturb = FAKE_P, FAKE_D

    assert _prepared(lambda bt: None)[0] == 0
    assert _prepared(lambda bt: setattr(bt, "perturb", FAKE_P))[0] == 0   # no gradient asked for: the forward only adds
    assert _prepared(both)[0] == 0


def test_prepare_rejects_perturb_with_gnn_frozen():
    def frozen(bt):
        bt.perturb, bt.gnn_frozen = FAKE_P, 1

    rc, err = _prepared(frozen)
    assert rc == INVALID and b"perturb with gnn_frozen" in err


def test_prepare_rejects_d_perturb_without_perturb():
    rc, err = _prepared(lambda bt: setattr(bt, "d_perturb", FAKE_D))
    assert rc == INVALID and b"d_perturb without perturb" in err

    def no_backward(bt):
        bt.perturb, bt.d_perturb, bt.will_bwd = FAKE_P, FAKE_D, 0

    rc, err = _prepared(no_backward)
    assert rc == INVALID and b"d_perturb without perturb" in err


def test_prepare_rejects_a_misaligned_perturbation():
    rc, err = _prepared(lambda bt: setattr(bt, "perturb", FAKE_P + 4))
    assert rc == INVALID and b"16-byte aligned" in err
