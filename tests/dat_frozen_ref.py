"""Reference numbers for DAT steps with frozen BatchNorm statistics -- TEST INFRASTRUCTURE shared by tests/test_dat_frozen_ref.py (CPU)
and tests/test_gpu_dat_frozen.py: torch autograd over oracle.dat_oracle.dat_forward OUTSIDE its train_mode, i.e. every BatchNorm with
its running statistics (eval semantics), parameters as leaf tensors.  Pinned against the reference's own DAT in eval mode with grad
enabled by G18 (tools/make_golden_dat_frozen.py)."""
from __future__ import annotations

import torch

from oracle import dat_oracle as DO

_NOT_PARAM = ("running_mean", "running_var")


def eval_loss_and_grads(sd, cfg, x, target, drop=None):
    """-> (L1 loss, output, {parameter name: gradient}) of one step with every BatchNorm frozen; drop: [n_blocks, 2, B] DropPath factors"""
    leaf = {}
    for k, v in sd.items():
        is_param = v.is_floating_point() and not (k.endswith(_NOT_PARAM) or "rpe_biases" in k or "attn_mask" in k)
        leaf[k] = v.detach().clone().requires_grad_(True) if is_param else v
    out = DO.dat_forward(leaf, cfg, x, drop)
    loss = (out - target).abs().mean()
    names = [k for k, v in leaf.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
    return float(loss.detach()), out.detach(), {k: (g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(names, grads)}


def grad_errors(got: dict, want: dict, floor: float):
    """{name: |got - want| / max(|want|, floor * the largest gradient norm of the model)}"""
    biggest = max(float(v.norm()) for v in want.values())
    return {n: float((got[n].float() - w).norm()) / max(float(w.norm()), floor * biggest) for n, w in want.items()}
