"""References, inputs and guarded launchers for the fused attention kernels of csrc/attention.hip (k_attn_fwd, k_attn_bwd_dq,
k_attn_bwd_dkv), used by tests/test_attention_refs_host.py (CPU) and tests/test_hip_attention_kernels.py (GPU).  Nothing here needs
a GPU to import.

* `Layout`: desc / row_stride / rows / max_npos of both token layouts (tests/test_hip_attention.py:make_layout), a padded S larger than
  the longest sequence (every sequence left padded), optionally a work list; `Layout.from_desc` for hand-made descriptors.
* `reference`: float64, one sequence and head at a time, from the contract in include/graphtrans_hip.h: ctx, d_qkv (autograd) and
  lse = natural-log logsumexp of the scaled, masked scores; takes an explicit keep mask and 1 / (1 - p), and dense / key_valid masks
  with masked_fill(mask == 0, mask_value) semantics.
* `keep_mask`: THE SPECIFICATION of the attention dropout: the keep decision as a pure function of (seed, sequence, head, query
  position, key position), restated with int64 tensors from the definition in the comments of csrc/attention.hip (rng_qpart,
  rng_kpart, rng_mix, AttnArgs::drop_thr).  Its `flaw` argument builds deliberately WRONG variants, used only by the host tests to show
  that the value comparison can tell them from the right one.
* work lists: `oracle_work` (tests/test_model_driver_host.py:numpy_layout, the suite's layout oracle) and `shuffled_work`.
* probes: inputs with q = 0 (uniform weights 1 / n) from whose outputs the keep decisions of each kernel can be read off exactly.
* `launch_fwd` / `launch_bwd`: raw launchers of gt_attn_fwd(_last) / gt_attn_bwd(_last) through kernel_refs._call.  Every output is
  allocated here, prefilled with NaN (d_qkv of the pooled backward: with the zeros its contract demands) and followed by a guard band
  that is checked after the launch; the descriptors, the work list and every buffer size are checked on the host before the launch.
"""
import math

import numpy as np
import torch

from kernel_refs import DEV, _call, _code, _ok, _p, _stream
from test_model_driver_host import numpy_layout

NAN = float("nan")
GUARD = 256
TILE_Q = 64          # positions per work item (BLOCK_N of csrc/attention.hip)

LENS = (1, 31, 32, 33, 63, 64, 65, 97, 129, 200)   # key step 32, query block 64, odd lengths, 4 query blocks x 7 key steps
NHEAD = 3                                          # bh = seq * nhead + head with an nhead that is no power of two
S_PADDED = 201                                     # every sequence left padded; kv_off odd for the even lengths
SEED = 0x12345678_9ABCDEF1                         # non-zero high half (seed_hi enters the query part of the hash)
INSTANTIATIONS = {
    "fp32-hd32": (torch.float32, 32),     # the default bf16x6 products
    "fp32-hd48": (torch.float32, 48),     # the exact fp32 chains, LDS columns padded to 64
    "bf16-hd64": (torch.bfloat16, 64),
    "bf16-hd128": (torch.bfloat16, 128),  # TilePairWide staging
}
TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}  # the op's own (tests/test_hip_attention.py), atol = rtol in conftest.assert_close
FLAWS = ("halves_swapped", "query_block_shift", "key_step_shift", "bh_sum", "keys_relative")


# ----------------------------------------------------------------------------------------------------------------------------
# layouts and work lists
# ----------------------------------------------------------------------------------------------------------------------------
class Layout:
    """desc [B][4] int32 = {row0, npos, kv_off, kv_len}; position p of sequence b is token row row0 + p * row_stride"""

    def __init__(self, kind, lens, S=None, work=None):
        lens = [int(n) for n in lens]
        if kind == "packed":
            ptr = np.concatenate([[0], np.cumsum(lens)])
            desc = [[int(ptr[i]), n, 0, n] for i, n in enumerate(lens)]
            self._set(desc, 1, int(ptr[-1]))
        else:
            assert kind == "padded"
            S = max(lens) if S is None else int(S)
            assert S >= max(lens)
            self._set([[i, S, S - n, n] for i, n in enumerate(lens)], len(lens), S * len(lens))
        self.kind = kind
        self.work = None if work is None else check_work(self, work)

    @classmethod
    def from_desc(cls, desc, row_stride, rows, work=None):
        self = cls.__new__(cls)
        self._set(desc, row_stride, rows)
        self.kind = "custom"
        self.work = None if work is None else check_work(self, work)
        return self

    def _set(self, desc, row_stride, rows):
        self.desc = np.asarray(desc, np.int32).reshape(-1, 4)
        self.B, self.row_stride, self.rows = self.desc.shape[0], int(row_stride), int(rows)
        self.max_npos = int(self.desc[:, 1].max()) if self.B else 0
        d = self.desc.astype(np.int64)
        assert (d >= 0).all() and (d[:, 2] + d[:, 3] <= d[:, 1]).all(), "kv range outside the sequence"
        assert ((d[:, 1] == 0) | (d[:, 0] + (d[:, 1] - 1) * self.row_stride < self.rows)).all(), "a position beyond the token rows"
        assert ((d[:, 1] == 0) | (d[:, 3] > 0)).all(), "a sequence with positions and no valid key"
        owner = np.full(self.rows, -1)
        for b in range(self.B):
            r = self.token_rows(b)
            assert (owner[r] == -1).all(), "two positions share a token row"
            owner[r] = b

    def with_work(self, work):
        other = Layout.from_desc(self.desc, self.row_stride, self.rows, work)
        other.kind = self.kind
        return other

    def token_rows(self, b):
        row0, npos = int(self.desc[b, 0]), int(self.desc[b, 1])
        return row0 + np.arange(npos, dtype=np.int64) * self.row_stride

    def valid_rows(self):
        """token rows of the positions that hold a key (not padding), all sequences"""
        out = [self.token_rows(b)[int(self.desc[b, 2]):int(self.desc[b, 2] + self.desc[b, 3])] for b in range(self.B)]
        return torch.from_numpy(np.concatenate(out) if out else np.zeros(0, np.int64))

    def position_rows(self):
        """token rows of every position, padding included"""
        out = [self.token_rows(b) for b in range(self.B)]
        return torch.from_numpy(np.concatenate(out) if out else np.zeros(0, np.int64))

    def last_rows(self):
        return torch.from_numpy(np.asarray([self.token_rows(b)[-1] for b in range(self.B)], np.int64))

    def last_tile_rows(self):
        """token rows of the 64-position tile that holds each sequence's last position: what the pooled forward writes"""
        out = [self.token_rows(b)[(int(self.desc[b, 1]) - 1) // TILE_Q * TILE_Q:] for b in range(self.B)]
        return torch.from_numpy(np.concatenate(out))

    def tiles(self):
        """every (sequence, 64-position tile) that exists"""
        return [(b, t) for b in range(self.B) for t in range((int(self.desc[b, 1]) + TILE_Q - 1) // TILE_Q)]


def check_work(lay, work):
    """a work list of `lay`: int32 [num_work][2], every tile of the layout exactly once, every other entry {-1, 0}"""
    work = np.ascontiguousarray(work, np.int32).reshape(-1, 2)
    real = [(int(s), int(t)) for s, t in work if s >= 0]
    assert sorted(real) == sorted(lay.tiles()), "the work list is not the layout's tiles, each exactly once"
    assert all(int(t) == 0 for s, t in work if s < 0) and all(int(s) == -1 for s, t in work if s < 0), "a padding entry that is not {-1, 0}"
    return work


def oracle_work(lens, kind):
    """the work list numpy_layout builds for these lengths (no truncation, no CLS): XCD slices by length rank, {-1, 0} padded"""
    return numpy_layout(list(lens), kind, 1 << 20, False)[3]


def shuffled_work(lay, seed, pad_at=()):
    """every (sequence, tile) of the layout exactly once in a seeded shuffled order; the FINAL list holds {-1, 0} at the indices pad_at"""
    tiles = lay.tiles()
    order = np.random.RandomState(seed).permutation(len(tiles))
    out = [list(tiles[i]) for i in order]
    for at in sorted(pad_at):
        assert 0 <= at <= len(out)
        out.insert(at, [-1, 0])
    return np.asarray(out, np.int32).reshape(-1, 2)


# ----------------------------------------------------------------------------------------------------------------------------
# the dropout decision
# ----------------------------------------------------------------------------------------------------------------------------
def drop_thr(p):
    """AttnArgs::drop_thr: clamp(int(p * 65536 + 0.5), 1, 65535) of the fp32 p the entry point receives; 0 (no dropout) for p = 0"""
    if not p > 0:
        return 0
    return int(min(max(float(np.float32(p)) * 65536.0 + 0.5, 1.0), 65535.0))


def _mix(x):
    M = 0xFFFFFFFF
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & M
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & M
    return x ^ (x >> 16)


def keep_mask(seed, seq, head, nhead, npos, p, flaw=None, kv_off=0):
    """bool [npos][npos], [q][k] True = the weight of query position q on key position k is kept.

        h    = mix((q * 0x9E3779B1) ^ (bh * 0xC2B2AE3D + seed_hi), (k & ~1) * 0x85EBCA77 + seed_lo),   bh = seq * nhead + head
        mix(a, b): x = a ^ b; x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (all mod 2^32)
        half = h & 0xffff for an even k, h >> 16 for an odd k        (one hash decides a pair of adjacent keys)
        keep = half >= thr,   thr = clamp(int(p * 65536 + 0.5), 1, 65535)

    q and k are POSITIONS inside the sequence (padding positions count), so the decision does not depend on the token layout's row
    numbering, on the head dim or on the storage type.  `flaw` (one of FLAWS) and `kv_off` exist for the host tests only."""
    M = 0xFFFFFFFF
    s_lo, s_hi = seed & M, (seed >> 32) & M
    q = torch.arange(npos, dtype=torch.int64).reshape(-1, 1)
    k = torch.arange(npos, dtype=torch.int64).reshape(1, -1)
    bh = seq * nhead + head
    if flaw == "query_block_shift":
        q = q + 64
    elif flaw == "key_step_shift":
        k = k + 32
    elif flaw == "bh_sum":
        bh = seq + head
    elif flaw == "keys_relative":
        k = (k - kv_off) & M
    else:
        assert flaw in (None, "halves_swapped")
    qpart = ((q * 0x9E3779B1) & M) ^ ((bh * 0xC2B2AE3D + s_hi) & M)
    kpart = (((k & ~1) * 0x85EBCA77) + s_lo) & M
    h = _mix(qpart ^ kpart)
    odd = (k & 1) == 1
    if flaw == "halves_swapped":
        odd = ~odd
    half = torch.where(odd, h >> 16, h & 0xFFFF)
    return half >= drop_thr(p)


def keep_masks(lay, nhead, p, seed, flaw=None):
    """{(sequence, head): keep_mask} of a layout"""
    return {(b, h): keep_mask(seed, b, h, nhead, int(lay.desc[b, 1]), p, flaw, int(lay.desc[b, 2]))
            for b in range(lay.B) for h in range(nhead)}


def rate_bound(thr, decisions):
    """(expected keep rate, 5 binomial standard deviations of the observed rate over `decisions` independent decisions)"""
    rate = 1.0 - thr / 65536.0
    return rate, 5.0 * math.sqrt(rate * (1.0 - rate) / decisions)


def masks_on_valid_keys(masks, lay):
    """the decisions that exist: every query position x the keys of [kv_off, kv_off + kv_len), all (sequence, head) in one vector"""
    out = [m[:, int(lay.desc[b, 2]):int(lay.desc[b, 2] + lay.desc[b, 3])].reshape(-1) for (b, h), m in sorted(masks.items())]
    return torch.cat(out)


# ----------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ----------------------------------------------------------------------------------------------------------------------------
def reference(qkv, d_ctx, lay, nhead, scale, keep=None, inv_keep=1.0, dense_mask=None, key_valid=None, mask_value=-1e6):
    """(ctx [rows][d], d_qkv [rows][3d], lse [nhead][rows]) in float64.  Per sequence and head: s = scale q k^T over the keys of
    [kv_off, kv_off + kv_len) only (rows outside it are never read as keys or values), masked_fill(mask == 0, mask_value) for the
    dense [B][T][T] and key_valid [B][T] masks, lse = logsumexp(s), P = softmax(s) * keep * inv_keep, ctx = P v for EVERY query
    position of the sequence; d_qkv is the gradient of sum(ctx * d_ctx).  Rows that are no position of any sequence stay 0 / NaN (lse)."""
    x = qkv.detach().double().clone().requires_grad_(True)
    rows, d = x.shape[0], x.shape[1] // 3
    hd = d // nhead
    ctx = torch.zeros(rows, d, dtype=torch.float64)
    lse = torch.full((nhead, rows), NAN, dtype=torch.float64)
    for b in range(lay.B):
        npos, kv_off, kv_len = (int(v) for v in lay.desc[b, 1:])
        if npos == 0:
            continue
        idx = torch.from_numpy(lay.token_rows(b))
        xq, xkv = x[idx], x[idx[kv_off:kv_off + kv_len]]
        for h in range(nhead):
            q = xq[:, h * hd:(h + 1) * hd]
            k = xkv[:, d + h * hd:d + (h + 1) * hd]
            v = xkv[:, 2 * d + h * hd:2 * d + (h + 1) * hd]
            s = (q @ k.t()) * scale
            if dense_mask is not None:
                s = s.masked_fill(dense_mask[b][:, kv_off:kv_off + kv_len] == 0, mask_value)
            if key_valid is not None:
                s = s.masked_fill(key_valid[b][kv_off:kv_off + kv_len].reshape(1, -1) == 0, mask_value)
            lse[h, idx] = torch.logsumexp(s.detach(), dim=-1)
            w = torch.softmax(s, dim=-1)
            if keep is not None:
                w = w * keep[(b, h)][:, kv_off:kv_off + kv_len].double() * inv_keep
            ctx[idx, h * hd:(h + 1) * hd] = w @ v
    (ctx * d_ctx.double()).sum().backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return ctx.detach(), grad, lse


def random_inputs(lay, nhead, hd, dtype, seed, nan_padding=False, last_only=False):
    """(qkv [rows][3d], d_ctx [rows][d]) fp32 on the CPU, already rounded to `dtype`.  nan_padding: the K and V thirds of the rows at
    positions < kv_off hold NaN (their Q third and d_ctx stay finite: the kernels load those as query positions).  last_only: d_ctx is
    zero outside each sequence's last position (the pooled backward's contract)."""
    g = torch.Generator().manual_seed(seed)
    d = nhead * hd
    qkv = torch.randn(lay.rows, 3 * d, generator=g).to(dtype).float()
    d_ctx = torch.randn(lay.rows, d, generator=g).to(dtype).float()
    if last_only:
        keep = torch.zeros(lay.rows, 1)
        keep[lay.last_rows()] = 1.0
        d_ctx = d_ctx * keep
    if nan_padding:
        for b in range(lay.B):
            pad = torch.from_numpy(lay.token_rows(b)[:int(lay.desc[b, 2])])
            qkv[pad, d:] = NAN
    return qkv, d_ctx


def dense_masks(B, T):
    """the mask pattern of tests/test_hip_attention_head_dims.py:test_dense_masks_fp32_head_dim_128"""
    g = torch.Generator().manual_seed(6)
    dense = (torch.rand(B, T, T, generator=g) < 0.6).float()
    dense[1, 5] = 0.0
    valid = torch.ones(B, T)
    valid[0, 50:] = 0.0
    valid[2, :3] = 0.0
    return dense, valid


# ----------------------------------------------------------------------------------------------------------------------------
# probes: q = 0, so every score is 0 and every weight 1 / n (n = kv_len) whatever K holds
# ----------------------------------------------------------------------------------------------------------------------------
def probe_chunks(lay, hd):
    """first key / query position of every probe launch: ceil(max_npos / hd) chunks of hd positions"""
    return list(range(0, lay.max_npos, hd))


def probe_inputs(lay, nhead, hd, chunk0, which):
    """(qkv, d_ctx) fp32 of one probe launch over the positions [chunk0, chunk0 + hd), per head:
    "v" (forward and dK/dV): V[key j] = e_(j - chunk0) and d_ctx[query i] = e_(i - chunk0) inside the chunk, 0 elsewhere:
        ctx[i][c] = keep(i, chunk0 + c) / (n (1 - p)),   dV[j][c] = keep(chunk0 + c, j) / (n (1 - p));
    "k" (dQ): K[key j] = e_(j - chunk0) inside the chunk, V = e_0 for every key, d_ctx = e_0 for every query:
        dQ[i][c] = scale / n * (keep(i, chunk0 + c) / (1 - p) - delta_i),   delta_i = kept_i / (n (1 - p))."""
    d = nhead * hd
    qkv = torch.zeros(lay.rows, 3 * d)
    d_ctx = torch.zeros(lay.rows, d)
    for b in range(lay.B):
        npos, kv_off, kv_len = (int(v) for v in lay.desc[b, 1:])
        pos = np.arange(npos)
        rows = lay.token_rows(b)
        valid = (pos >= kv_off) & (pos < kv_off + kv_len)
        inch = (pos >= chunk0) & (pos < chunk0 + hd)
        for h in range(nhead):
            if which == "v":
                qkv[rows[valid & inch], 2 * d + h * hd + pos[valid & inch] - chunk0] = 1.0
                d_ctx[rows[inch], h * hd + pos[inch] - chunk0] = 1.0
            else:
                assert which == "k"
                qkv[rows[valid & inch], d + h * hd + pos[valid & inch] - chunk0] = 1.0
                qkv[rows[valid], 2 * d + h * hd] = 1.0
                d_ctx[rows, h * hd] = 1.0
    return qkv, d_ctx


def new_probe_values(lay, nhead):
    """{(sequence, head): float64 [npos][npos] of NaN}: filled chunk by chunk by the read_* functions, [query][key]"""
    return {(b, h): torch.full((int(lay.desc[b, 1]),) * 2, NAN, dtype=torch.float64) for b in range(lay.B) for h in range(nhead)}


def _chunk_keys(lay, b, chunk0, hd):
    npos, kv_off, kv_len = (int(v) for v in lay.desc[b, 1:])
    lo, hi = max(chunk0, kv_off), min(chunk0 + hd, kv_off + kv_len)
    return np.arange(lo, max(lo, hi))


def read_fwd(values, ctx, lay, nhead, hd, chunk0):
    """values[(b, h)][i][j] = ctx[query i][j - chunk0] for the valid keys j of the chunk ("v" probe)"""
    ctx = ctx.double()
    for b in range(lay.B):
        rows, keys = torch.from_numpy(lay.token_rows(b)), _chunk_keys(lay, b, chunk0, hd)
        for h in range(nhead):
            values[(b, h)][:, keys] = ctx[rows][:, h * hd + keys - chunk0]


def read_dv(values, d_qkv, lay, nhead, hd, chunk0):
    """values[(b, h)][i][j] = dV[key j][i - chunk0] for the queries i of the chunk and every valid key j ("v" probe)"""
    d_qkv = d_qkv.double()
    d = nhead * hd
    for b in range(lay.B):
        npos, kv_off, kv_len = (int(v) for v in lay.desc[b, 1:])
        rows = torch.from_numpy(lay.token_rows(b)[kv_off:kv_off + kv_len])
        qs = np.arange(min(chunk0, npos), min(chunk0 + hd, npos))
        for h in range(nhead):
            values[(b, h)][qs, kv_off:kv_off + kv_len] = d_qkv[rows][:, 2 * d + h * hd + qs - chunk0].t()


def read_dq(values, d_qkv, lay, nhead, hd, chunk0):
    """values[(b, h)][i][j] = dQ[query i][j - chunk0] for the valid keys j of the chunk ("k" probe): > 0 kept, < 0 dropped"""
    d_qkv = d_qkv.double()
    for b in range(lay.B):
        rows, keys = torch.from_numpy(lay.token_rows(b)), _chunk_keys(lay, b, chunk0, hd)
        for h in range(nhead):
            values[(b, h)][:, keys] = d_qkv[rows][:, h * hd + keys - chunk0]


def undecided_queries(mask, kv_off, kv_len):
    """bool [npos]: the queries whose valid keys are all kept or all dropped -- their dQ probe row is 0 in every column"""
    kept = mask[:, kv_off:kv_off + kv_len].sum(1)
    return (kept == 0) | (kept == kv_len)


# ----------------------------------------------------------------------------------------------------------------------------
# guarded raw launchers
# ----------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """an output of n elements followed by GUARD more, all prefilled with `fill` (NaN or 0); check() after the launch"""

    def __init__(self, shape, dtype, fill):
        self.n, self.fill = int(np.prod(shape)), fill
        self.buf = torch.full((self.n + GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[:self.n].view(*shape)

    def check(self, what):
        tail = self.buf[self.n:]
        ok = tail.isnan().all() if math.isnan(self.fill) else (tail == self.fill).all()
        assert bool(ok), f"{what}: a store behind the end of the output"
        return self.t


class DeviceLayout:
    """desc and work list of a Layout on the device (copies of the host arrays unless the tensors of a real SeqLayout are given)"""

    def __init__(self, lay, desc=None, work=None):
        self.lay = lay
        self.desc = torch.from_numpy(lay.desc).to(DEV).contiguous() if desc is None else desc
        self.work = work if work is not None else (None if lay.work is None else torch.from_numpy(lay.work).to(DEV).contiguous())


def _int32_ok(t, n, what):
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() == n, what
    assert t.data_ptr() % 4 == 0, what


def _check_inputs(dl, qkv, nhead, dense_mask, key_valid, use_work):
    lay = dl.lay
    dtype = qkv.dtype
    rows, d3 = qkv.shape
    d = d3 // 3
    assert rows == lay.rows and d3 == 3 * d and d % nhead == 0 and (d // nhead) % 8 == 0
    _ok(qkv, dtype, rows * d3, "qkv")
    _int32_ok(dl.desc, 4 * lay.B, "seq_desc")
    assert np.array_equal(dl.desc.cpu().numpy().reshape(-1, 4), lay.desc), "seq_desc on the device is not the layout's"
    if use_work:
        assert dl.work is not None
        _int32_ok(dl.work, 2 * lay.work.shape[0], "work_items")
        check_work(lay, dl.work.cpu().numpy())
    T = lay.max_npos
    if dense_mask is not None or key_valid is not None:
        assert (lay.desc[:, 1] == T).all(), "dense masks: every sequence has npos == max_npos"
    if dense_mask is not None:
        _ok(dense_mask, torch.float32, lay.B * T * T, "dense_mask")
    if key_valid is not None:
        _ok(key_valid, torch.float32, lay.B * T, "key_valid")
    return rows, d


def launch_fwd(dl, qkv, nhead, scale, p=0.0, seed=0, use_work=False, pooled=False, dense_mask=None, key_valid=None, mask_value=0.0):
    """(ctx [rows][d], lse [2][nhead][rows]) of gt_attn_fwd, or gt_attn_fwd_last when pooled; both NaN wherever the kernel wrote nothing"""
    lay = dl.lay
    rows, d = _check_inputs(dl, qkv, nhead, dense_mask, key_valid, use_work)
    ctx = Guarded((rows, d), qkv.dtype, NAN)
    lse = Guarded((2, nhead, rows), torch.float32, NAN)
    common = dict(dtype=_code(qkv.dtype), qkv=_p(qkv), ctx=_p(ctx.buf), lse=_p(lse.buf), total_rows=rows, d_model=d, nhead=nhead,
                  seq_desc=_p(dl.desc), num_seqs=lay.B, row_stride=lay.row_stride, max_npos=lay.max_npos)
    tail = dict(scale=float(scale), dropout_p=float(p), seed=int(seed), stream=_stream())
    if pooled:
        assert not use_work and dense_mask is None and key_valid is None
        _call("gt_attn_fwd_last", **common, **tail)
    else:
        _call("gt_attn_fwd", **common, work_items=_p(dl.work) if use_work else None, num_work=int(lay.work.shape[0]) if use_work else 0,
              dense_mask=_p(dense_mask), key_valid=_p(key_valid), mask_value=float(mask_value), **tail)
    torch.cuda.synchronize()
    return ctx.check("ctx"), lse.check("lse")


def launch_bwd(dl, qkv, ctx, d_ctx, lse, nhead, scale, p=0.0, seed=0, use_work=False, pooled=False, dense_mask=None, key_valid=None,
               mask_value=0.0):
    """(d_qkv [rows][3d], delta [nhead][rows]) of gt_attn_bwd, or gt_attn_bwd_last when pooled.  d_qkv is prefilled with NaN; the
    pooled backward's with 0, as its contract demands."""
    lay = dl.lay
    rows, d = _check_inputs(dl, qkv, nhead, dense_mask, key_valid, use_work)
    _ok(ctx, qkv.dtype, rows * d, "ctx")
    _ok(d_ctx, qkv.dtype, rows * d, "d_ctx")
    _ok(lse, torch.float32, 2 * nhead * rows, "lse")
    assert ctx.numel() == rows * d and d_ctx.numel() == rows * d and lse.numel() == 2 * nhead * rows
    d_qkv = Guarded((rows, 3 * d), qkv.dtype, 0.0 if pooled else NAN)
    delta = Guarded((nhead, rows), torch.float32, NAN)
    head = dict(dtype=_code(qkv.dtype), qkv=_p(qkv), ctx=_p(ctx), d_ctx=_p(d_ctx), lse=_p(lse), delta=_p(delta.buf), d_qkv=_p(d_qkv.buf),
                total_rows=rows, d_model=d, nhead=nhead, seq_desc=_p(dl.desc), num_seqs=lay.B, row_stride=lay.row_stride,
                max_npos=lay.max_npos, work_items=_p(dl.work) if use_work else None, num_work=int(lay.work.shape[0]) if use_work else 0)
    tail = dict(scale=float(scale), dropout_p=float(p), seed=int(seed), stream=_stream())
    if pooled:
        assert dense_mask is None and key_valid is None
        _call("gt_attn_bwd_last", **head, **tail)
    else:
        _call("gt_attn_bwd", **head, dense_mask=_p(dense_mask), key_valid=_p(key_valid), mask_value=float(mask_value), **tail)
    torch.cuda.synchronize()
    return d_qkv.check("d_qkv"), delta.check("delta")


def lse_natural(lse):
    """[nhead][rows] float64 natural-log logsumexp from the kernels' [2][nhead][rows] (running max, log2 of the sum; log2 domain)"""
    lse = lse.double().cpu()
    return (lse[0] + lse[1]) * math.log(2.0)
