"""Generate tests/golden/g18_dat_frozen_bn*.npz by running the REFERENCE's DAT with BatchNorm layers in eval mode and grad enabled
(build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/make_golden_dat_frozen.py   (from the repo root)

G18: one fine-tuning step of the tiny DAT of G14 / G14c (weights oracle.dat_oracle.random_state_dict(seed 16, scale 2.0), pinned by
their SHA-1; the running buffers of that state dict are non-trivial) with frozen BatchNorm statistics:

    a   model.eval(), 24 x 40 (padded window frame), batch 2
    b   model.eval(), 32 x 32, batch 1 (a training-mode BatchNorm over the batch of pooled vectors refuses this batch)
    c   model.train() with drop_path_rate 0 and only the attn.dwconv.1 BatchNorms in eval, 32 x 32, batch 2 (mixed state)

Each case stores x, target, y, the L1 loss, every parameter's gradient and the BatchNorm buffers after the step.  The script itself
asserts that no buffer moves in (a) and (b), that in (c) exactly the un-frozen BatchNorms move, and that the gradients of (a) differ
from the train-mode gradients of the same batch by more than the GPU test's tolerance (0.1 per tensor, measured as the test does) in at
least 50 tensors: the tolerance tells the two modes apart.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import dat_oracle as DO  # noqa: E402
from oracle.make_golden import DAT_TINY, save, sha1  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

SEED, SCALE = 16, 2.0
TOL, FLOOR = 0.1, 2e-3              # tests/test_gpu_dat_frozen.py: per-tensor error against max(|ref|, FLOOR * largest gradient norm)
CASES = {                            # tag -> (mode, (H, W), batch)
    "a": ("eval", (24, 40), 2),
    "b": ("eval", (32, 32), 1),
    "c": ("train_dwconv_frozen", (32, 32), 2),
}
BUF_SUFFIXES = ("running_mean", "running_var", "num_batches_tracked")


def batch(tag: str):
    _, hw, B = CASES[tag]
    g = torch.Generator().manual_seed(1800 + ord(tag))
    return torch.rand(B, 3, *hw, generator=g), torch.rand(B, 3, hw[0] * 2, hw[1] * 2, generator=g)


def set_mode(m, mode: str):
    if mode == "eval":
        return m.eval()
    m.train()
    if mode == "train_dwconv_frozen":
        for n, mod in m.named_modules():
            if n.endswith("attn.dwconv.1"):
                mod.eval()
    return m


def step(da, cfg, sd, mode: str, x, t):
    torch.manual_seed(0)
    m = da.DAT(**cfg.kwargs(), drop_path_rate=0.0)
    m.load_state_dict(sd, strict=True)
    set_mode(m, mode)
    y = m(x)
    assert y.grad_fn is not None
    loss = torch.nn.functional.l1_loss(y, t)
    loss.backward()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for n, p in m.named_parameters()}
    bufs = {n: b.detach().clone() for n, b in m.named_buffers() if n.endswith(BUF_SUFFIXES)}
    return y.detach(), float(loss), grads, bufs


def main():
    da = import_reference("dat_arch")
    cfg = DO.DATConfig(**DAT_TINY)
    sd = DO.random_state_dict(cfg, seed=SEED, scale=SCALE)
    arrays = {"weight_seed": np.array(SEED), "weight_scale": np.array(SCALE),
              "weight_sha1": np.array(sha1(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()])))}
    for tag, (mode, hw, B) in CASES.items():
        x, t = batch(tag)
        y, loss, grads, bufs = step(da, cfg, sd, mode, x, t)
        assert all(g is not None for g in grads.values())
        moved = sorted(n for n, b in bufs.items() if not torch.equal(b, sd[n]))
        if mode == "eval":
            assert not moved, moved
        else:          # exactly the BatchNorms left in training mode move (all three of their buffers)
            want = sorted(n for n in bufs if ".dwconv.1." not in n)
            assert moved == want, (len(moved), len(want))
        arrays[f"{tag}.x"], arrays[f"{tag}.t"], arrays[f"{tag}.y"], arrays[f"{tag}.loss"] = x.numpy(), t.numpy(), y.numpy(), np.array(loss)
        for n, g in grads.items():
            arrays[f"{tag}.grad.{n}"] = g.numpy()
        for n, b in bufs.items():
            arrays[f"{tag}.buf.{n}"] = b.numpy()
        print(f"case {tag}: {mode} {hw} batch {B}: loss {loss:.6f}, {len(grads)} gradients, {len(moved)} buffers moved")
        if tag == "a":          # the same batch in train mode: the tolerance of the GPU test separates the two sets of gradients
            _, _, gtrain, _ = step(da, cfg, sd, "train", x, t)
            biggest = max(float(g.norm()) for g in grads.values())
            errs = {n: float((gtrain[n] - g).norm()) / max(float(g.norm()), FLOOR * biggest) for n, g in grads.items()}
            far = [n for n, e in errs.items() if e > TOL]
            print(f"case a vs train mode: {len(far)} of {len(errs)} gradient tensors differ by more than {TOL}, worst {max(errs.values()):.3g}")
            assert len(far) >= 50
    save("g18_dat_frozen_bn", **arrays)


if __name__ == "__main__":
    main()
