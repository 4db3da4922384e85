"""Everything the whole-model driver (csrc/model.hip, engine.py) computes, on a fixed grid of fused models, into one file:
python tools/driver_dump.py OUT.pt [name filter] [--digest]

For every entry of the grid in the fp32, mixed and bf16 modes: one training forward + backward (dropout on, fixed seeds), one eval
forward, and the training step once more with the backward in its three stages (a one-rank GradSync that asks for them) -- logits,
every gradient, every buffer (the BatchNorm statistics), and what gt_model_prepare answered (gt_model_sizes).  Two revisions of the
driver that launch the same kernels in the same order write files whose tensors are torch.equal:
python tools/driver_dump.py --compare A.pt B.pt
--digest keeps a SHA-256 of every tensor's bytes (with dtype and shape) in the tensor's place: a file of a few hundred KB that
compares the same way."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

DEV = "cuda:0"
MODES = {"fp32": (torch.float32, torch.float32), "mixed": (torch.float32, torch.bfloat16), "bf16": (torch.bfloat16, torch.bfloat16)}


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = sorted(set(a) ^ set(b))
    n = 0
    for k in sorted(set(a) & set(b)):
        for f in sorted(set(a[k]) | set(b[k])):
            x, y = a[k].get(f), b[k].get(f)
            same = torch.equal(x, y) if torch.is_tensor(x) and torch.is_tensor(y) else x == y
            n += 1
            if not same:
                bad.append(f"{k}: {f}")
    print(f"{len(a)} / {len(b)} entries, {n} fields compared, {len(bad)} differ")
    for s in bad[:40]:
        print("  DIFFERS", s)
    return 1 if bad else 0


def grid():
    """name -> (build(compute_dtype) -> model, batch, loss(out))"""
    from test_hip_engine import CASES, GIN_CASES, ROWS_CASES, _args
    from graphtrans_amd import losses, synth
    from graphtrans_amd.encoders import ASTNodeEncoder, AtomEncoder, BondEncoder
    from graphtrans_amd.models.gnn_transformer import GNNTransformer
    from graphtrans_amd.models.pna_transformer import PNATransformer
    from oracle import reference_math as rm

    def ident(kw):
        return ",".join(f"{k}={v}" for k, v in sorted(kw.items()) if k != "compute_dtype") or "default"

    def labels(B, n, seed):
        return torch.randint(0, 50, (B, n), generator=torch.Generator().manual_seed(seed)).to(DEV)

    def code2(kw, B, seed, D=64, frozen=False, host_sizes=False):
        def build(dt):
            args = _args(**{**kw, "compute_dtype": dt})
            model = GNNTransformer(50, ASTNodeEncoder(D, 98, 300, 20), lambda d: torch.nn.Linear(2, d), args).to(DEV)
            if frozen:
                model.gnn_node.requires_grad_(False)
            b = synth.code2_like(B=B, seed=seed, num_nodeattributes=300)
            if host_sizes:   # the per-graph sizes a training loop knows: the token layout is built on the host (else on the device)
                b._sizes = torch.bincount(b.batch, minlength=B).numpy()
            b = b.to(DEV)
            if model.max_seq_len is None:
                return model, b, lambda out: out.float().square().mean()
            y = labels(B, 5, seed)
            return model, b, lambda out: losses.code2_loss(out, y)
        return build

    def mol(kw):
        def build(dt):
            args = _args(**{**kw, "compute_dtype": dt, "max_seq_len": None})
            model = GNNTransformer(16, AtomEncoder(64), lambda d: BondEncoder(d), args).to(DEV)
            b = synth.molpcba_like(B=24, seed=4).to(DEV)
            g = torch.Generator().manual_seed(4)
            y = (torch.rand(24, 16, generator=g) > 0.5).float()
            y[torch.rand(24, 16, generator=g) < 0.2] = float("nan")
            y = y.to(DEV)
            return model, b, lambda out: losses.mol_loss(out, y)
        return build

    def dense(case):
        def build(dt):
            args = _args(max_seq_len=None, gnn_virtual_node=False, gnn_JK="last", compute_dtype=dt)
            if case == "tud":
                model = GNNTransformer(2, torch.nn.Linear(37, 64), lambda d: (lambda _e: 0), args).to(DEV)
                b = synth.nci1_like(B=16, seed=3).to(DEV)
            else:
                model = GNNTransformer(2, torch.nn.Linear(64, 64), lambda d: torch.nn.Linear(2, d), args).to(DEV)
                b = synth.er_stress(B=6, seed=3, n=40, avg_deg=4.0, feat_dim=64).to(DEV)
            return model, b, lambda out: losses.tud_loss(out, b.y)
        return build

    def pna(dt):   # the model of tests/test_hip_pna.py::test_pna_fused_path_equals_module_path, with GNN dropout
        args = rm.default_args(gnn_virtual_node=False, gnn_num_layer=3, gnn_emb_dim=64, gnn_JK="last", gnn_residual=True, gnn_dropout=0.25,
                               d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.1, num_encoder_layers=2,
                               transformer_norm_input=True, graph_pooling="cls", max_seq_len=3, aggregators=["mean", "max", "min", "std"],
                               scalers=["identity", "amplification", "attenuation"], deg=torch.tensor([0, 40, 25, 9, 3]), compute_dtype=dt)
        b = synth.code2_like(B=24, seed=2, mean_nodes=20.0, max_nodes=60).to(DEV)
        model = PNATransformer(50, ASTNodeEncoder(64, 98, 10030, 20), None, args).to(DEV)
        return model, b, lambda out: losses.code2_loss(out, b.y_arr)

    g = {}
    for kw in CASES:
        g["case:" + ident(kw)] = code2(kw, 12, 5)
    for kw in GIN_CASES:
        kw = dict(kw)
        feat = kw.pop("feat")
        kw.setdefault("gnn_type", "gin")
        g[f"gin:{feat}," + ident(kw)] = mol(kw) if feat == "mol" else code2(kw, 12, 5)
    for kw in ROWS_CASES:
        g["rows:" + ident(kw)] = code2(dict(gnn_emb_dim=128, d_model=128, dim_feedforward=256, **kw), 24, 21, D=128, host_sizes=True)
    def gnn(kw, B, seed, D=64):   # the read-out mode (gt_model::readout): models.gnn.GNN, no token rows (every mode is fp32-stored)
        def build(dt):
            from graphtrans_amd.models.gnn import GNN
            a = dict(gnn_virtual_node=True, gnn_num_layer=3, gnn_emb_dim=D, gnn_JK="last", gnn_dropout=0.1, gnn_residual=False,
                     gnn_type="gcn", graph_pooling="mean", max_seq_len=3, model_type="gnn")
            a.update(kw)
            from types import SimpleNamespace
            model = GNN(50, ASTNodeEncoder(D, 98, 300, 20), lambda d: torch.nn.Linear(2, d), SimpleNamespace(**a)).to(DEV)
            b = synth.code2_like(B=B, seed=seed, num_nodeattributes=300)
            b._sizes = torch.bincount(b.batch, minlength=B).numpy()
            b = b.to(DEV)
            y = labels(B, 5, seed)
            return model, b, lambda out: losses.code2_loss(out, y)
        return build

    def pnanet(msl):   # the read-out mode over the PNA stack: head kind 1 (max_seq_len None: the narrow MLP) or 2 (the position heads)
        def build(dt):
            from types import SimpleNamespace
            from graphtrans_amd.models.pna import PNANet
            a = SimpleNamespace(gnn_num_layer=3, gnn_emb_dim=64, gnn_dropout=0.25, gnn_residual=True, graph_pooling="mean", max_seq_len=msl,
                                model_type="pna", aggregators=["mean", "max", "min", "std"],
                                scalers=["identity", "amplification", "attenuation"], deg=torch.tensor([0, 40, 25, 9, 3]))
            model = PNANet(50, ASTNodeEncoder(64, 98, 300, 20), None, a).to(DEV)
            b = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
            y = labels(12, 5, 5)
            return model, b, (lambda out: out.float().square().mean()) if msl is None else (lambda out: losses.code2_loss(out, y))
        return build

    def transformer(feat):   # the encoder-only mode (models.transformer.Transformer with fused_step): table and Linear input encoder
        def build(dt):
            from types import SimpleNamespace
            from graphtrans_amd.models.transformer import Transformer
            a = SimpleNamespace(d_model=64, nhead=4, dim_feedforward=128, transformer_dropout=0.1, transformer_activation="relu",
                                num_encoder_layers=2, max_input_len=100, transformer_norm_input=True, graph_pooling="cls",
                                max_seq_len=(3 if feat == "ast" else None), model_type="transformer", gnn_type="gcn", gnn_virtual_node=False,
                                fused_step=True, compute_dtype=dt)
            if feat == "ast":
                model = Transformer(50, ASTNodeEncoder(64, 98, 300, 20), None, a).to(DEV)
                b = synth.code2_like(B=12, seed=5, num_nodeattributes=300).to(DEV)
                y = labels(12, 5, 5)
                return model, b, lambda out: losses.code2_loss(out, y)
            model = Transformer(2, torch.nn.Linear(37, 64), None, a).to(DEV)
            b = synth.nci1_like(B=16, seed=3).to(DEV)
            return model, b, lambda out: losses.tud_loss(out, b.y)
        return build

    g["pna"] = pna
    g["pnanet:mlp"], g["pnanet:positions"] = pnanet(None), pnanet(3)
    g["transformer:ast"], g["transformer:linear"] = transformer("ast"), transformer("linear")
    for pool in ("sum", "mean", "max"):
        for kw in (dict(), dict(gnn_type="gin", gnn_virtual_node=False)):
            g[f"gnn:{pool}," + ident(kw)] = gnn(dict(graph_pooling=pool, **kw), 12, 5)
    g["gnn:max,B=128,D=160"] = gnn(dict(graph_pooling="max"), 128, 3, D=160)   # > 4096 rows: the pooling's row chunks, the weight images
    g["frozen"] = code2(dict(fused_freeze=True, gnn_dropout=0.25), 12, 5, frozen=True)
    g["pos_encoder"] = code2(dict(pos_encoder=True, token_layout="packed", gnn_dropout=0.25), 12, 5)
    g["dense:tud"], g["dense:er"] = dense("tud"), dense("er")
    # GCN with and without a virtual node across the driver's dispatch lines: a few hundred nodes; > 1024 (weight images, transposed
    # weights, BatchNorm statistics in the exact dX kernel); > 12288 (row map, broadcast epilogue, the register-row kernel)
    # (with GNN dropout, and without it -- the encoder's dropout stays on --: only then do the BatchNorm-backward statistics ride in the
    # dX epilogue, in the exact kernel from 1024 nodes without a virtual node)
    for vn in (True, False):
        for B in (4, 12, 128):
            for p in (0.1, 0.0):
                g[f"gcn160:vn={vn},B={B},gnn_dropout={p}"] = code2(dict(gnn_virtual_node=vn, gnn_emb_dim=160, gnn_JK="last", gnn_dropout=p),
                                                                   B, 3, D=160, host_sizes=True)
    return g


def asked(model, N, mm, dt):
    """The driver's dispatch questions for a GCN / GIN model, asked of the library the way gt_model_prepare asks them (the plan's
    weight images bound): which entries of the grid take which path.  A record for the log; the driver's own answers are opaque."""
    import contextlib
    from graphtrans_amd import _lib, engine, ops
    from graphtrans_amd._lib import GT_BF16, GT_F32
    plan, L = engine._plan(model), _lib.lib()
    if plan.kind == "pna" or getattr(plan, "enc_only", False):
        return {}
    tok_bf16 = dt == torch.bfloat16
    imgs = None
    if mm != torch.bfloat16 and N >= 1024:
        imgs = plan.imgs3 if tok_bf16 else (plan.imgs3e or plan.imgs3)
    compute, tdt = ops.f32_compute_code(), GT_BF16 if tok_bf16 else GT_F32
    D, d, Kc = plan.D, plan.d, (2 if plan.jk_cat else 1) * plan.D
    gcn, vn, frozen = plan.kind == "gcn", plan.has_vn, plan.frozen
    ro = bool(plan.readout)   # (no gnn2transformer: the two questions about its GEMM are not asked)
    w, w0 = (0 if ro else model.gnn2transformer.weight.data_ptr()), plan.w3_weights[0].data_ptr()
    with (imgs.bound() if imgs is not None else contextlib.nullcontext()):
        a = dict(cat2=bool(not ro and plan.jk_cat and imgs is not None and L.gt_linear_cat2_ok(compute, w, N, d, D, D)),
                 fuse_rows=bool(not ro and L.gt_linear_rows_ok(compute, GT_F32, tdt, w, N, d, Kc)),
                 bc=bool(gcn and vn and not frozen and L.gt_linear_bwd_bcast_ok(compute, GT_F32, GT_F32, w0, N, D, D)))
        rows = exact = int(L.gt_linear_bwd_bnstats_rows(N))
        if imgs is not None:
            rows = int(L.gt_linear_bwd_bnstats_rows_for(compute, GT_F32, GT_F32, w0, N, D, D))
        a["fuse_bn"] = bool(plan.L > 1 and not frozen and gcn and model.gnn_node.drop_ratio == 0 and rows > 0
                            and L.gt_linear_bwd_bnstats_ok(compute, GT_F32, GT_F32, N) and (rows != exact or (not vn and N <= 65536)))
    a["want_wt"] = bool(not frozen and compute != GT_BF16 and N >= 1024 and (imgs is None or (not vn and gcn)))
    return a


def main(out_path, only=None, digest=False):
    from graphtrans_amd import _lib, engine, ops
    from graphtrans_amd.dist import GradSync

    class Staged(GradSync):   # one rank, nothing on a wire: only asks the fused backward for its stages
        active = True

        def reduce_flat(self, flat, lo, hi):
            self.ranges = getattr(self, "ranges", []) + [(lo, hi)]

    L = _lib.lib()
    sizes, prepare = [], L.gt_model_prepare

    def wrapped(m, b, ctx, sz):   # (the way tools/host_phases.py wraps the driver's entry points)
        rc = prepare(m, b, ctx, sz)
        s = sz._obj
        sizes.append([int(getattr(s, k)) for k in ("rows", "max_npos", "num_work", "arena_bytes", "barena_bytes", "exact")])
        return rc
    L.gt_model_prepare = wrapped

    def step(model, b, loss, seed):
        for p in model.parameters():
            p.grad = None
        torch.manual_seed(seed)
        out = model(b)
        logits = torch.stack(list(out)) if isinstance(out, (list, tuple)) else out
        loss(out).backward()
        return logits.detach().float().clone()

    res = {}
    for name, build in grid().items():
        if only and only not in name:
            continue
        for mode, (mm, dt) in MODES.items():
            ops.set_matmul_dtype(mm)
            torch.manual_seed(0)
            model, b, loss = build(dt)
            with torch.no_grad():   # non-trivial 1-d parameters (BatchNorm / LayerNorm affine, biases)
                for p in model.parameters():
                    if p.dim() == 1:
                        p.add_(torch.randn_like(p) * 0.1)
            model.train()
            key, r = f"{name}|{mode}", {}
            r["eligible"] = bool(engine.eligible(model, b, None))
            if r["eligible"]:
                del sizes[:]
                r["N"] = int(b.batch.numel())
                r["asked"] = ",".join(k for k, v in asked(model, r["N"], mm, dt).items() if v)
                r["train.logits"] = step(model, b, loss, 7)
                for n, p in model.named_parameters():
                    if p.grad is not None:
                        r["grad." + n] = p.grad.detach().clone()
                model.eval()
                with torch.no_grad():
                    out = model(b)
                    r["eval.logits"] = (torch.stack(list(out)) if isinstance(out, (list, tuple)) else out).float().clone()
                model.train()
                sync = Staged(model.parameters(), world_size=1).attach(model)
                r["staged.logits"] = step(model, b, loss, 7)
                r["staged.ranges"] = len(getattr(sync, "ranges", []))
                for n, p in model.named_parameters():
                    if p.grad is not None:
                        r["staged.grad." + n] = p.grad.detach().clone()
                for n, t in model.named_buffers():
                    r["buffer." + n] = t.detach().clone()
                r["sizes"] = [list(s) for s in sizes]
                torch.cuda.synchronize()
            res[key] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()}
            if digest:
                res[key] = {k: (f"{v.dtype} {tuple(v.shape)} " + hashlib.sha256(v.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
                                if torch.is_tensor(v) else v) for k, v in res[key].items()}
            print(key, "N", r.get("N"), "eligible", r["eligible"], "stages", r.get("staged.ranges"), "asked", r.get("asked"), "sizes", r.get("sizes"), flush=True)
    ops.set_matmul_dtype(torch.float32)
    torch.save(res, out_path)
    print("wrote", out_path, len(res), "entries")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    rest = [a for a in sys.argv[2:] if a != "--digest"]
    main(sys.argv[1], rest[0] if rest else None, digest="--digest" in sys.argv)
