"""FLAG adversarial augmentation (the reference's `-m 3` trainer, trainers/flag_trainer.py:30-50), one batch at a time.

FLAG ("free large-scale adversarial augmentation on graphs") trains on node features perturbed inside an L-inf ball: per batch it
draws a perturbation uniformly in (-step, step), then runs the model `m` times -- each loss scaled by 1 / m, each backward
accumulating into the parameters' `.grad` -- and between two runs moves the perturbation one step along the sign of its own
gradient.  One optimizer step closes the batch.

    perturb ~ U(-step, step)  [N, gnn_emb_dim]
    loss = calc_loss(model(batch, perturb), batch) / m
    m - 1 times:  loss.backward();  perturb += step * sign(perturb.grad);  perturb.grad = 0;  loss = (the same forward) / m
    loss.backward();  optimizer.step()

`flag_step` runs on either data path.  With `model.fused_flag` (--fused_flag) every forward / backward is the fused step: the
perturbation is added inside the input encoder's kernel, `perturb.grad` is the d h_list[0] the backward computes anyway, and the
second and third backward accumulate with one add over the flat gradient buffer (engine._FusedModel).  Without it the model runs
module by module, as it always did with a perturbation.  The ascent is one kernel either way (gt_flag_ascent).
"""
import torch

from . import _lib, engine
from .graph import _stream


def ascent(perturb, step_size):
    """perturb <- perturb + step_size * sign(perturb.grad); perturb.grad <- 0, in place, one launch (gt_flag_ascent)."""
    g = perturb.grad
    if g is None:
        raise RuntimeError("graphtrans_amd.flag: the perturbation has no gradient (did the loss depend on it?)")
    if not (perturb.is_cuda and perturb.dtype == torch.float32 and perturb.is_contiguous() and g.dtype == torch.float32
            and g.is_contiguous() and g.shape == perturb.shape and g.device == perturb.device):
        raise ValueError("graphtrans_amd.flag: perturb and its gradient must be contiguous fp32 tensors of one shape on the GPU")
    _lib.launch("gt_flag_ascent", perturb.data_ptr(), g.data_ptr(), perturb.numel(), float(step_size), _stream())


def flag_step(model, batch, optimizer, calc_loss, m=3, step_size=8e-3, perturb=None):
    """One FLAG training step on `batch` (already on the model's device): `m` forward / backward passes with loss / m, `m - 1`
    ascents of the perturbation, then `optimizer.step()`.  Returns the last (scaled) loss, as the reference's trainer does.

    `perturb`: the starting perturbation (fp32 [N, gnn_emb_dim] on the device; it is updated in place and gets `requires_grad`), or
    None to draw uniform(-step_size, step_size) on the device.  Gradients are cleared with `optimizer.zero_grad(set_to_none=True)`
    first: the first backward then writes the flat buffer directly and the later ones accumulate into it."""
    if m < 1:
        raise ValueError("graphtrans_amd.flag: m >= 1")
    dev = batch.batch.device
    if perturb is None:
        perturb = torch.empty((int(batch.batch.numel()), engine.emb_dim(model)), dtype=torch.float32, device=dev)
        perturb.uniform_(-step_size, step_size)
    perturb.requires_grad_(True)   # (a leaf: the caller's tensor itself, which therefore sees the ascents and the last gradient)
    perturb.grad = None
    model.train()
    optimizer.zero_grad(set_to_none=True)
    loss = calc_loss(model(batch, perturb), batch) / m
    for _ in range(m - 1):
        loss.backward()
        ascent(perturb, step_size)
        loss = calc_loss(model(batch, perturb), batch) / m
    loss.backward()
    optimizer.step()
    return loss.detach()
