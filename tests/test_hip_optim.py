"""FusedAdamW (gt_adamw_step) against torch.optim.AdamW (the reference's optimizer, main.py:178)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _models():
    torch.manual_seed(0)
    a = torch.nn.Sequential(torch.nn.Linear(37, 301), torch.nn.ReLU(), torch.nn.Linear(301, 5), torch.nn.Embedding(11, 3)).to(DEV)
    b = torch.nn.Sequential(torch.nn.Linear(37, 301), torch.nn.ReLU(), torch.nn.Linear(301, 5), torch.nn.Embedding(11, 3)).to(DEV)
    b.load_state_dict(a.state_dict())
    return a, b


def _loss(m, x, use_emb):
    y = m[2](m[1](m[0](x))).square().mean()
    if use_emb:
        y = y + m[3].weight.sum() * 0.1
    return y


@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_fused_adamw_matches_torch(wd):
    from graphtrans_amd.optim import FusedAdamW
    a, b = _models()
    oa = torch.optim.AdamW(a.parameters(), lr=3e-3, weight_decay=wd, betas=(0.9, 0.99), eps=1e-8)
    ob = FusedAdamW(b.parameters(), lr=3e-3, weight_decay=wd, betas=(0.9, 0.99), eps=1e-8)
    sched = torch.optim.lr_scheduler.StepLR(ob, step_size=3, gamma=0.5)
    scheda = torch.optim.lr_scheduler.StepLR(oa, step_size=3, gamma=0.5)
    for i in range(8):
        x = torch.randn(64, 37, device=DEV)
        use_emb = i % 3 != 1  # the embedding has no gradient on some steps: torch skips it (its step count lags)
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad(set_to_none=True)
            _loss(m, x, use_emb).backward()
            o.step()
        sched.step()
        scheda.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-5, atol=1e-7), (pa - pb).abs().max()
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for k in sa:
        assert float(sa[k]["step"]) == float(sb[k]["step"])
        assert torch.allclose(sa[k]["exp_avg"], sb[k]["exp_avg"], rtol=1e-5, atol=1e-8)
        assert torch.allclose(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"], rtol=1e-5, atol=1e-10)


def test_fused_adamw_state_dict_roundtrip():
    from graphtrans_amd.optim import FusedAdamW
    a, b = _models()
    oa = FusedAdamW(a.parameters(), lr=1e-2)
    x = torch.randn(16, 37, device=DEV)
    for _ in range(3):
        oa.zero_grad(set_to_none=True)
        _loss(a, x, True).backward()
        oa.step()
    b.load_state_dict(a.state_dict())
    ob = FusedAdamW(b.parameters(), lr=1e-2)
    ob.load_state_dict(oa.state_dict())
    for m, o in ((a, oa), (b, ob)):
        o.zero_grad(set_to_none=True)
        _loss(m, x, True).backward()
        o.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


def test_fused_adamw_rejects_cpu_parameters():
    from graphtrans_amd.optim import FusedAdamW
    m = torch.nn.Linear(4, 4)
    o = FusedAdamW(m.parameters())
    m(torch.randn(2, 4)).sum().backward()
    with pytest.raises(RuntimeError):
        o.step()


@pytest.mark.parametrize("max_norm", [0.05, 1e3])
def test_fused_adamw_grad_clip_matches_clip_grad_norm(max_norm):
    """trainers/base_trainer.py:34-36: clip_grad_norm_(model.parameters(), grad_clip) then optimizer.step();
    0.05 clips on every step here, 1e3 never does (coefficient clamped to 1)."""
    from graphtrans_amd.optim import FusedAdamW
    a, b = _models()
    oa = torch.optim.AdamW(a.parameters(), lr=3e-3, weight_decay=0.01)
    ob = FusedAdamW(b.parameters(), lr=3e-3, weight_decay=0.01, max_grad_norm=max_norm)
    for i in range(5):
        x = torch.randn(64, 37, device=DEV)
        use_emb = i != 2
        oa.zero_grad(set_to_none=True)
        _loss(a, x, use_emb).backward()
        norm = torch.nn.utils.clip_grad_norm_(a.parameters(), max_norm)
        oa.step()
        ob.zero_grad(set_to_none=True)
        _loss(b, x, use_emb).backward()
        ob.step()
        assert torch.allclose(ob.last_grad_norm, norm, rtol=1e-5), (ob.last_grad_norm, norm)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-5, atol=1e-7), (pa - pb).abs().max()


def _against_torch_adamw(params, ref_params, grads_of, max_norm, steps=4):
    """FusedAdamW (weight decay and clipping on) on `params` against torch.optim.AdamW + clip_grad_norm_ on `ref_params`, both fed the
    gradients grads_of(step, i) -- for `params` through whatever tensor grads_of hands out (its pointer is what the kernel reads)."""
    from graphtrans_amd.optim import FusedAdamW
    oa = torch.optim.AdamW(ref_params, lr=3e-3, weight_decay=0.01)
    ob = FusedAdamW(params, lr=3e-3, weight_decay=0.01, max_grad_norm=max_norm)
    clipped = []
    for s in range(steps):
        for i, (pa, pb) in enumerate(zip(ref_params, params)):
            pb.grad = grads_of(s, i)
            pa.grad = pb.grad.detach().clone()
        norm = torch.nn.utils.clip_grad_norm_(ref_params, max_norm)
        clipped.append(float(norm) > max_norm)
        oa.step()
        ob.step()
        assert torch.allclose(ob.last_grad_norm, norm, rtol=1e-5), (s, ob.last_grad_norm, norm)
    assert True in clipped and False in clipped   # both sides of the clamp
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for i, (pa, pb) in enumerate(zip(ref_params, params)):
        assert torch.allclose(pa, pb, rtol=1e-5, atol=1e-7), (i, (pa - pb).abs().max())
        assert float(sa[i]["step"]) == float(sb[i]["step"]) == steps
        assert torch.allclose(sa[i]["exp_avg"], sb[i]["exp_avg"], rtol=1e-5, atol=1e-8), i
        assert torch.allclose(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"], rtol=1e-5, atol=1e-10), i


def test_fused_adamw_splits_launches_beyond_384_tensors():
    """401 tensors in one group: gt_grad_sqnorm and gt_adamw_step take at most GT_ADAMW_MAX_TENSORS = 384 gradient pointers per launch,
    so both run as two launches (tensor_begin / chunk_begin != 0 in the second).  400 parameters of 1 to 9 elements and one of 5000
    (three chunks) that sits in the second launch."""
    g = torch.Generator().manual_seed(3)
    sizes = [1 + i % 9 for i in range(400)]
    sizes.insert(390, 5000)
    init = [torch.randn(n, generator=g) for n in sizes]
    params = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    ref = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    # gradients of the neighbouring tests' size (1e-2): the moments' absolute tolerances are sized for those
    scale = [0.003, 0.01, 0.005, 0.02]   # gradient norms of about 0.25, 0.84, 0.42, 1.68 around max_norm = 0.5
    grads = [[(scale[s] * torch.randn(n, generator=g)).to(DEV) for n in sizes] for s in range(4)]
    _against_torch_adamw(params, ref, lambda s, i: grads[s][i], 0.5)


def test_fused_adamw_unaligned_pointers_take_the_scalar_path():
    """Parameters and gradients that are contiguous views at ODD element offsets of flat buffers: 4-byte aligned pointers, which the
    kernel may not read as float4 (sizes 3, 7 and 2051: a chunk boundary inside the last).  The elements of the flat parameter buffer
    between and behind the views stay as they were."""
    g = torch.Generator().manual_seed(4)
    sizes, offs = [3, 7, 2051], [1, 5, 13]
    total = offs[-1] + sizes[-1] + 5
    pbuf = torch.randn(total, generator=g).to(DEV)
    before = pbuf.clone()
    params = [torch.nn.Parameter(pbuf[o:o + n]) for o, n in zip(offs, sizes)]
    assert all(p.data_ptr() % 16 != 0 and p.data_ptr() % 8 == 4 for p in params)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    scale = [0.003, 0.01, 0.005, 0.02]   # gradient norms of about 0.14, 0.45, 0.23, 0.91 around max_norm = 0.3
    gbufs = [(scale[s] * torch.randn(total, generator=g)).to(DEV) for s in range(4)]

    def grads_of(s, i):
        v = gbufs[s][offs[i]:offs[i] + sizes[i]]
        assert v.is_contiguous() and v.data_ptr() % 8 == 4
        return v
    _against_torch_adamw(params, ref, grads_of, 0.3)
    keep = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        keep[o:o + n] = False
    assert int(keep.sum()) == 8
    assert torch.equal(pbuf.cpu()[keep], before.cpu()[keep])
    for p, o, n in zip(params, offs, sizes):   # (and the parameters still ARE the views: the step wrote in place)
        assert p.data_ptr() == pbuf.data_ptr() + 4 * o and not torch.equal(p.detach(), before[o:o + n])
