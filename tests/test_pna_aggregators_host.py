"""Host side of PNAConv's aggregator list (modules/pna/aggregators.py:37-44: sum, mean, min, max, var, std): construction with the
reference's parameter shapes, the slot count K the list selects, and the gather maps that restack the post-Linear's weight onto the
kernel's [x | K slots] operand.  No GPU: nothing here launches."""
import pytest
import torch

ALL6 = ["sum", "mean", "min", "max", "var", "std"]
DEG = torch.tensor([0, 5, 9, 7, 3, 1, 0, 2])


def _conv(aggregators, scalers, D=16, towers=4):
    from graphtrans_amd.modules.pna.pna_module import PNAConv

    return PNAConv(D, D, aggregators=aggregators, scalers=scalers, deg=DEG, towers=towers, divide_input=True)


@pytest.mark.parametrize("aggregators,slots", [(["sum"], 6), (["var"], 6), (ALL6, 6), (["var", "mean", "sum"], 6),
                                               (["mean", "max", "min", "std"], 4), (["std", "mean"], 4)])
@pytest.mark.parametrize("scalers", [["identity"], ["amplification", "attenuation"], ["identity", "amplification", "attenuation"]])
def test_pnaconv_constructs_with_the_references_shapes(aggregators, slots, scalers):
    conv = _conv(aggregators, scalers)
    T, F = 4, 4
    A, S = len(aggregators), len(scalers)
    assert conv.agg_slots == slots
    shapes = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    expect = {"lin.weight": (16, 16), "lin.bias": (16,)}
    for t in range(T):
        expect[f"pre_nns.{t}.0.weight"] = (F, 2 * F)
        expect[f"pre_nns.{t}.0.bias"] = (F,)
        expect[f"post_nns.{t}.0.weight"] = (F, (A * S + 1) * F)
        expect[f"post_nns.{t}.0.bias"] = (F,)
    assert shapes == expect


@pytest.mark.parametrize("aggregators", [["median"], ["mean", "median"], ["sum", "moment3"]])
def test_unknown_aggregator_is_rejected(aggregators):
    with pytest.raises(NotImplementedError, match="aggregator"):
        _conv(aggregators, ["identity"])


def _parent_maps(conv):
    """The restacking maps as they were with the fixed [x | mean | max | min | std] operand (5 F columns), restated independently."""
    slot4 = {"mean": 0, "max": 1, "min": 2, "std": 3}
    Fi, Fo, A, S = conv.F_in, conv.F_out, len(conv.aggregators), len(conv._blocks)
    cols = (A * len(conv.scalers) + 1) * Fi
    first = S - len(conv.scalers)
    wmap = torch.full((S * Fo, 5 * Fi), Fo * cols, dtype=torch.int64)
    for s in range(S):
        for o in range(Fo):
            for f in range(Fi):
                if s == 0:
                    wmap[s * Fo + o, f] = o * cols + f
                if s >= first:
                    for ai, a in enumerate(conv.aggregators):
                        wmap[s * Fo + o, Fi + slot4[a] * Fi + f] = o * cols + Fi + (s - first) * A * Fi + ai * Fi + f
    bmap = torch.full((S * Fo,), Fo, dtype=torch.int64)
    bmap[:Fo] = torch.arange(Fo)
    return wmap.reshape(-1), bmap


@pytest.mark.parametrize("aggregators,scalers", [(ALL6, ["identity", "amplification", "attenuation"]),
                                                 (["var", "mean", "sum"], ["amplification", "linear", "inverse_linear"]),
                                                 (["sum"], ["identity"]), (["var"], ["attenuation", "identity"])])
def test_post_maps_k6_place_every_weight_once(aggregators, scalers):
    from graphtrans_amd.modules.pna.pna_module import _AGG_SLOT

    conv = _conv(aggregators, scalers, D=32)
    Fi, Fo, A, S = conv.F_in, conv.F_out, len(aggregators), len(conv._blocks)
    cols = (A * len(scalers) + 1) * Fi
    wmap, bmap = conv._post_maps("cpu")
    assert conv.agg_slots == 6 and wmap.shape == (S * Fo * 7 * Fi,) and bmap.shape == (S * Fo,)
    zero = Fo * cols
    used = wmap[wmap < zero]
    assert torch.equal(torch.sort(used).values, torch.arange(zero))          # every post weight element, exactly once
    # _winv inverts _wmap: source j sits at restacked position _winv[j]
    assert conv._winv.shape == (zero,) and torch.equal(wmap[conv._winv], torch.arange(zero))
    assert torch.equal(bmap[conv._binv], torch.arange(Fo))
    # where each element lands: row block = scaler block, column block = 1 + the aggregator's kernel slot (0 for x_i)
    first = S - len(scalers)
    w = wmap.view(S, Fo, 7, Fi)
    for s in range(S):
        for slot in range(7):
            blk = w[s, :, slot, :]
            names = [a for a in aggregators if _AGG_SLOT[a] == slot - 1]
            if slot == 0 and s == 0:
                src_block = 0
            elif slot > 0 and s >= first and names:
                src_block = 1 + (s - first) * A + aggregators.index(names[0])
            else:
                assert (blk == zero).all()
                continue
            o, f = torch.arange(Fo).view(Fo, 1), torch.arange(Fi).view(1, Fi)
            assert torch.equal(blk, o * cols + src_block * Fi + f)


@pytest.mark.parametrize("aggregators,scalers", [(["mean", "max", "min", "std"], ["identity", "amplification", "attenuation"]),
                                                 (["std", "mean", "min", "max"], ["amplification", "attenuation"]),
                                                 (["mean", "std"], ["linear"])])
def test_post_maps_k4_unchanged(aggregators, scalers):
    conv = _conv(aggregators, scalers, D=32)
    assert conv.agg_slots == 4
    wmap, bmap = conv._post_maps("cpu")
    pw, pb = _parent_maps(conv)
    assert torch.equal(wmap, pw) and torch.equal(bmap, pb)


def test_layer_descriptor_mirrors_agg_slots():
    """layers.PnaLayerDesc::agg_slots takes the place of the trailing pad of gt_pna_layer: same size, same offset, zero by default."""
    import ctypes as C

    from graphtrans_amd import layers

    d = layers.PnaLayerDesc()
    assert d.agg_slots == 0
    f = layers.PnaLayerDesc.agg_slots
    assert f.size == 4 and f.offset + 4 == C.sizeof(layers.PnaLayerDesc) and f.offset == layers.PnaLayerDesc.dropout_p.offset + 4
