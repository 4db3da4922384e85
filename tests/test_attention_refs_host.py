"""CPU checks of tests/attention_refs.py, the yardstick of tests/test_hip_attention_kernels.py: the float64 reference against
torch's own multi-head attention and against the masked_fill reference, the properties of keep_mask, the probe algebra (the three
constructions recover the mask they were given, before they touch a GPU), and the SENSITIVITY of the value comparison: at the common
shapes and the fp32 tolerance it rejects five deliberately wrong statements of the dropout decision.

What the value comparison can NOT see: one wrong decision of a query with n valid keys moves that query's ctx by |v| / (n (1 - p)),
at n = 200 about 7e-3 |v| -- above the fp32 tolerance (1e-4) and below the bf16 one (2e-2).  bf16 value checks cannot see a single
wrong decision at length 200 (test_one_wrong_decision_at_length_200_...), which is why the decision check of the GPU tests (check A)
reads the decisions themselves and compares them exactly, in both storage types.
"""
import numpy as np
import pytest
import torch

import attention_refs as R
from conftest import assert_close

P = 0.3


def _close(got, want, tol, what):
    """the comparison of check B"""
    assert_close(got, want, atol=tol, rtol=tol, what=what)


# ---- layouts and work lists --------------------------------------------------------------------------------------------------
def test_layouts_of_the_common_lengths_and_left_padding_at_S_201():
    """the desc / row_stride / rows / max_npos of tests/test_hip_attention.py:make_layout (which needs a GPU to run), and S = 201"""
    packed = R.Layout("packed", R.LENS)
    assert packed.rows == sum(R.LENS) and packed.row_stride == 1 and packed.max_npos == 200
    assert packed.desc.tolist()[:3] == [[0, 1, 0, 1], [1, 31, 0, 31], [32, 32, 0, 32]]
    padded = R.Layout("padded", R.LENS, S=R.S_PADDED)
    assert padded.rows == 201 * 10 and padded.row_stride == 10 and padded.max_npos == 201
    assert (padded.desc[:, 2] >= 1).all() and padded.desc[:, 2].tolist() == [201 - n for n in R.LENS]
    assert sorted(n for n, off in zip(R.LENS, padded.desc[:, 2]) if off % 2) == [n for n in R.LENS if n % 2 == 0]   # odd kv_off
    assert padded.valid_rows().numel() == sum(R.LENS) and padded.position_rows().numel() == padded.rows


@pytest.mark.parametrize("kind", ["packed", "padded"])
def test_work_lists_hold_every_tile_once(kind):
    lay = R.Layout(kind, R.LENS, S=R.S_PADDED if kind == "padded" else None)
    ntiles = len(lay.tiles())
    assert ntiles == (17 if kind == "packed" else 40)
    w = R.check_work(lay, R.oracle_work(R.LENS, kind))
    assert w.shape[0] % 8 == 0 and (w[:, 0] >= 0).sum() == ntiles
    s = R.shuffled_work(lay, 5, pad_at=(3, 4, 9))
    assert s.shape[0] == ntiles + 3 and s[[3, 4, 9]].tolist() == [[-1, 0]] * 3
    assert not np.array_equal(s[s[:, 0] >= 0], np.asarray(lay.tiles(), np.int32))     # shuffled
    R.check_work(lay, s)
    with pytest.raises(AssertionError):
        R.check_work(lay, s[1:])                   # a tile missing
    assert s[0, 0] >= 0
    with pytest.raises(AssertionError):
        R.check_work(lay, np.concatenate([s, s[:1]]))   # a tile twice
    with pytest.raises(AssertionError):
        R.check_work(lay, np.concatenate([s, [[-1, 1]]]))   # a padding entry that is not {-1, 0}


# ---- the float64 reference -----------------------------------------------------------------------------------------------------
def test_reference_matches_torch_multi_head_attention_float64():
    """F.multi_head_attention_forward in float64 with identity projections and the key_padding_mask of the left-padded layout
    (row = b + position * B is exactly torch's (S, B, E)): ctx and gradients; lse against a batched logsumexp of the same scores."""
    torch.manual_seed(0)
    lens, S, nhead, hd = [1, 5, 32, 33, 70], 71, 3, 8
    d = nhead * hd
    lay = R.Layout("padded", lens, S=S)
    B = lay.B
    qkv = torch.randn(lay.rows, 3 * d, dtype=torch.float64)
    d_ctx = torch.randn(lay.rows, d, dtype=torch.float64)
    ctx, d_qkv, lse = R.reference(qkv, d_ctx, lay, nhead, hd ** -0.5)
    x = qkv.clone().requires_grad_(True)
    q, k, v = (x[:, i * d:(i + 1) * d].reshape(S, B, d) for i in range(3))
    pad = torch.arange(S).reshape(1, -1) < torch.from_numpy(lay.desc[:, 2].astype(np.int64)).reshape(-1, 1)     # [B][S], True = padding
    eye = torch.eye(d, dtype=torch.float64)
    out, _ = torch.nn.functional.multi_head_attention_forward(
        q, k, v, d, nhead, None, None, None, None, False, 0.0, eye, None, training=False, key_padding_mask=pad, need_weights=False,
        use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    out = out.reshape(S * B, d)
    (out * d_ctx).sum().backward()
    assert float((ctx - out.detach()).abs().max()) < 1e-12
    assert float((d_qkv - x.grad).abs().max()) < 1e-12
    qh, kh = (t.detach().reshape(S, B, nhead, hd).permute(1, 2, 0, 3) for t in (q, k))       # [B][nhead][S][hd]
    s = (qh @ kh.transpose(-2, -1)) * hd ** -0.5
    want = torch.logsumexp(s.masked_fill(pad.reshape(B, 1, 1, S), float("-inf")), dim=-1)    # [B][nhead][S]
    got = lse.reshape(nhead, S, B).permute(2, 0, 1)
    assert float((got - want).abs().max()) < 1e-12


def test_reference_dense_form_matches_the_masked_fill_reference():
    from test_hip_attention_head_dims import _masked_fill_reference
    torch.manual_seed(1)
    B, T, nhead, hd = 3, 70, 3, 8
    d = nhead * hd
    lay = R.Layout("packed", [T] * B)
    qkv = torch.randn(B * T, 3 * d, dtype=torch.float64)
    d_ctx = torch.randn(B * T, d, dtype=torch.float64)
    dense, valid = R.dense_masks(B, T)
    ctx, d_qkv, lse = R.reference(qkv, d_ctx, lay, nhead, hd ** -0.5, dense_mask=dense, key_valid=valid, mask_value=-1e6)
    x = qkv.clone().requires_grad_(True)
    want = _masked_fill_reference(x, B, T, nhead, hd ** -0.5, dense, valid)
    (want * d_ctx).sum().backward()
    assert float((ctx - want.detach()).abs().max()) < 1e-12
    assert float((d_qkv - x.grad).abs().max()) < 1e-12
    row = 1 * T + 5                                                       # the fully masked row: uniform weights over all T keys
    assert float((lse[:, row] - (-1e6 + np.log(T))).abs().max()) < 1e-6


# ---- keep_mask -------------------------------------------------------------------------------------------------------------------
def _hash_halves(seed, seq, head, nhead, npos):
    """the 16-bit halves behind keep_mask, recovered from it by bisection over thr (keep = half >= thr)"""
    lo = torch.zeros(npos, npos, dtype=torch.int64)
    for bit in range(15, -1, -1):
        trial = lo + (1 << bit)
        ge = torch.zeros(npos, npos, dtype=torch.bool)
        for t in trial.unique().tolist():
            m = R.keep_mask(seed, seq, head, nhead, npos, t / 65536.0)
            assert R.drop_thr(t / 65536.0) == max(t, 1)
            ge |= m & (trial == t)
        lo = torch.where(ge, trial, lo)
    return lo


def test_drop_thr_rounds_and_clamps():
    assert R.drop_thr(0.0) == 0
    assert R.drop_thr(1e-9) == 1 and R.drop_thr(2.0 ** -18) == 1              # p -> 0: never "keep everything" while dropout is on
    assert R.drop_thr(0.999999) == 65535 and R.drop_thr(1.0 - 2.0 ** -20) == 65535      # p -> 1: 1 / 65536 of the weights survive
    assert R.drop_thr(0.5) == 32768 and R.drop_thr(0.1) == 6554 and R.drop_thr(0.3) == 19661
    assert R.drop_thr(0.3) == int(float(np.float32(0.3)) * 65536 + 0.5)
    full = R.keep_mask(R.SEED, 0, 0, 3, 64, 1e-9)
    assert int((~full).sum()) <= 2                                              # thr 1 drops a half only when it is 0
    assert 0 < int(R.keep_mask(R.SEED, 0, 0, 3, 512, 0.999999).sum()) <= 16     # thr 65535: 4 expected of 262144
    assert bool(R.keep_mask(R.SEED, 0, 0, 3, 16, 0.0).all())


def test_keep_mask_first_entries_by_hand():
    """the definition evaluated with Python integers for a few (q, k)"""
    M = 0xFFFFFFFF
    seed, seq, head, nhead, p = R.SEED, 7, 2, 3, 0.3
    m = R.keep_mask(seed, seq, head, nhead, 140, p)
    for q, k in [(0, 0), (0, 1), (5, 2), (63, 31), (64, 32), (65, 33), (139, 138), (139, 139), (17, 96)]:
        x = ((q * 0x9E3779B1) & M) ^ (((seq * nhead + head) * 0xC2B2AE3D + (seed >> 32)) & M)
        x ^= ((k & ~1) * 0x85EBCA77 + (seed & M)) & M
        x ^= x >> 16; x = (x * 0x7feb352d) & M
        x ^= x >> 15; x = (x * 0x846ca68b) & M
        x ^= x >> 16
        half = (x >> 16) if k & 1 else (x & 0xFFFF)
        assert bool(m[q, k]) == (half >= 19661), (q, k)


def test_keep_mask_pairs_share_one_hash():
    """keys 2j and 2j + 1: the low and the high half of ONE 32-bit hash -- rebuilt from the recovered halves, the 32-bit value of every
    pair is the definition's hash of (q, 2j)"""
    seed, seq, head, nhead, npos = R.SEED, 3, 1, 3, 12
    halves = _hash_halves(seed, seq, head, nhead, npos)
    M = 0xFFFFFFFF
    q = torch.arange(npos, dtype=torch.int64).reshape(-1, 1)
    k = torch.arange(0, npos, 2, dtype=torch.int64).reshape(1, -1)
    want = R._mix((((q * 0x9E3779B1) & M) ^ (((seq * nhead + head) * 0xC2B2AE3D + (seed >> 32)) & M)) ^ ((k * 0x85EBCA77 + (seed & M)) & M))
    assert torch.equal(halves[:, 0::2] | (halves[:, 1::2] << 16), want)


def test_keep_mask_depends_on_position_seed_sequence_and_head_only():
    a = R.keep_mask(R.SEED, 4, 1, 3, 201, P)
    assert torch.equal(a, R.keep_mask(R.SEED, 4, 1, 3, 201, P))
    assert torch.equal(a[:130, :130], R.keep_mask(R.SEED, 4, 1, 3, 130, P))        # a function of the position, not of npos
    for kind in ("packed", "padded"):                                               # nor of the layout's row numbering
        lay = R.Layout(kind, [201] * 6)
        assert torch.equal(R.keep_masks(lay, 3, P, R.SEED)[(4, 1)], a)
    for other in (R.keep_mask(R.SEED + 1, 4, 1, 3, 201, P), R.keep_mask(R.SEED + (1 << 32), 4, 1, 3, 201, P),
                  R.keep_mask(R.SEED, 5, 1, 3, 201, P), R.keep_mask(R.SEED, 4, 2, 3, 201, P)):
        differ = float((other != a).double().mean())
        assert abs(differ - 2 * P * (1 - P)) < 0.02, differ                         # independent masks differ in 2 p (1 - p) of the entries
    assert torch.equal(R.keep_mask(R.SEED, 1, 1, 3, 64, P), R.keep_mask(R.SEED, 2, 0, 2, 64, P))   # only bh = seq * nhead + head enters


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_rate_within_five_sigma(p):
    for kind in ("packed", "padded"):
        lay = R.Layout(kind, R.LENS, S=R.S_PADDED if kind == "padded" else None)
        m = R.masks_on_valid_keys(R.keep_masks(lay, R.NHEAD, p, R.SEED), lay)
        rate, bound = R.rate_bound(R.drop_thr(p), m.numel())
        assert bound < 0.01                                      # (a fixed 0.05 would be five to ten times as wide)
        assert abs(float(m.double().mean()) - rate) <= bound, (kind, p, float(m.double().mean()), rate, bound)


# ---- the probe algebra -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["packed", "padded"])
def test_probes_recover_the_mask_they_were_given(kind):
    """The constructions of check A evaluated on the float64 reference with an ARBITRARY mask (random, not keep_mask): the forward, dV
    and dQ read-outs return exactly that mask; a query with all keys kept or all dropped has an all-zero dQ probe row."""
    lens, nhead, hd, p = [1, 2, 9, 33, 70], 2, 16, 0.25
    lay = R.Layout(kind, lens, S=72 if kind == "padded" else None)
    g = torch.Generator().manual_seed(3)
    given = {(b, h): torch.rand(int(lay.desc[b, 1]), int(lay.desc[b, 1]), generator=g) < 0.7 for b in range(lay.B) for h in range(nhead)}
    given[(3, 0)][4] = True      # all kept
    given[(3, 1)][6] = False     # all dropped
    scale, inv_keep = hd ** -0.5, 1.0 / (1.0 - p)
    fwd, dv, dq = (R.new_probe_values(lay, nhead) for _ in range(3))
    chunks = R.probe_chunks(lay, hd)
    assert len(chunks) == -(-lay.max_npos // hd)
    for c0 in chunks:
        qkv, d_ctx = R.probe_inputs(lay, nhead, hd, c0, "v")
        ctx, d_qkv, _ = R.reference(qkv, d_ctx, lay, nhead, scale, given, inv_keep)
        R.read_fwd(fwd, ctx, lay, nhead, hd, c0)
        R.read_dv(dv, d_qkv, lay, nhead, hd, c0)
        qkv, d_ctx = R.probe_inputs(lay, nhead, hd, c0, "k")
        _, d_qkv, _ = R.reference(qkv, d_ctx, lay, nhead, scale, given, inv_keep)
        R.read_dq(dq, d_qkv, lay, nhead, hd, c0)
    for (b, h), want in given.items():
        off, n = int(lay.desc[b, 2]), int(lay.desc[b, 3])
        cols = slice(off, off + n)
        f, v, q = fwd[(b, h)][:, cols], dv[(b, h)][:, cols], dq[(b, h)][:, cols]
        w64 = want[:, cols].double()
        assert not f.isnan().any() and not v.isnan().any() and not q.isnan().any()       # every decision was probed
        assert torch.equal(f > 0, want[:, cols]) and torch.equal(v > 0, want[:, cols])
        level = 1.0 / (n * (1 - p))
        assert float((f - w64 * level).abs().max()) < 1e-15 and float((v - w64 * level).abs().max()) < 1e-15
        skip = R.undecided_queries(want, off, n)
        assert float(q[skip].abs().max() if skip.any() else 0.0) < 1e-17
        assert torch.equal(q[~skip] > 0, want[:, cols][~skip]) and torch.equal(q[~skip] < 0, ~want[:, cols][~skip])
        delta = w64.sum(1, keepdim=True) * level
        assert float((q - scale / n * (w64 * inv_keep - delta)).abs().max()) < 1e-15
    assert bool(R.undecided_queries(given[(3, 0)], int(lay.desc[3, 2]), 33)[4]) and bool(R.undecided_queries(given[(3, 1)], int(lay.desc[3, 2]), 33)[6])


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
_CASES = {}


def _value_case(kind):
    """the common shapes at fp32 / head dim 32: inputs and the reference under the RIGHT mask, computed once"""
    if kind not in _CASES:
        lay = R.Layout(kind, R.LENS, S=R.S_PADDED if kind == "padded" else None)
        hd = 32
        qkv, d_ctx = R.random_inputs(lay, R.NHEAD, hd, torch.float32, 11, nan_padding=kind == "padded")
        right = R.reference(qkv, d_ctx, lay, R.NHEAD, hd ** -0.5, R.keep_masks(lay, R.NHEAD, P, R.SEED), 1.0 / (1.0 - P))
        _CASES[kind] = (lay, hd, qkv, d_ctx, right)
    return _CASES[kind]


def _flags(got, want, rows, tol):
    """does check B's comparison reject `got` against `want`?  (ctx, d_qkv and lse on the valid rows; lse does not see dropout)"""
    flagged = []
    for name, g, w in zip(("ctx", "d_qkv"), got, want):
        try:
            _close(g[rows], w[rows], tol, name)
        except AssertionError:
            flagged.append(name)
    return flagged


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_value_comparison_rejects_a_wrong_dropout_decision(flaw):
    """a kernel that computed exactly the reference under a flawed mask fails check B at the fp32 tolerance, in ctx AND in d_qkv"""
    kind = "padded" if flaw == "keys_relative" else "packed"       # (keys relative to kv_off: the same mask when kv_off = 0)
    lay, hd, qkv, d_ctx, right = _value_case(kind)
    wrong_masks = R.keep_masks(lay, R.NHEAD, P, R.SEED, flaw)
    changed = float((R.masks_on_valid_keys(wrong_masks, lay) != R.masks_on_valid_keys(R.keep_masks(lay, R.NHEAD, P, R.SEED), lay)).double().mean())
    assert changed > 0.2, changed
    wrong = R.reference(qkv, d_ctx, lay, R.NHEAD, hd ** -0.5, wrong_masks, 1.0 / (1.0 - P))
    rows = lay.valid_rows()
    assert _flags(wrong, right, rows, R.TOL[torch.float32]) == ["ctx", "d_qkv"]
    assert _flags(right, right, rows, R.TOL[torch.float32]) == []
    assert not right[0][rows].isnan().any() and not right[1][rows].isnan().any()         # NaN in the padding rows' K / V reached nothing


def test_keys_relative_flaw_is_invisible_in_the_packed_layout():
    lay = R.Layout("packed", R.LENS)
    a, b = R.keep_masks(lay, R.NHEAD, P, R.SEED), R.keep_masks(lay, R.NHEAD, P, R.SEED, "keys_relative")
    assert all(torch.equal(a[key], b[key]) for key in a)


def test_one_wrong_decision_at_length_200_is_seen_at_the_fp32_tolerance_only():
    lay, hd, qkv, d_ctx, right = _value_case("packed")
    masks = {key: m.clone() for key, m in R.keep_masks(lay, R.NHEAD, P, R.SEED).items()}
    b = R.LENS.index(200)
    masks[(b, 1)][150, 77] ^= True
    wrong = R.reference(qkv, d_ctx, lay, R.NHEAD, hd ** -0.5, masks, 1.0 / (1.0 - P))
    rows = lay.valid_rows()
    assert _flags(wrong, right, rows, R.TOL[torch.float32]) == ["ctx", "d_qkv"]
    assert _flags(wrong, right, rows, R.TOL[torch.bfloat16]) == []
