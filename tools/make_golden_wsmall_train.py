"""Generate tests/golden/g19_swinir_wsmall_train*.npz by running the REFERENCE's SwinIR at window sizes below 8 forward and backward
(build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/make_golden_wsmall_train.py   (from the repo root)

G19: the four tiny models of G17 (tools/make_golden_wsmall.py: the '' head of the JPEG models and both pixel-shuffle heads at window 7,
'pixelshuffle' at window 4) in one training step: drop_path_rate 0, a 2 x C x 16 x 19 batch (reflect padding: 882 tokens at window 7,
640 at window 4) and a target at the output size, both from recorded seeds.  Recorded: the reference's L1 loss, every parameter's
gradient and the name-ordered gradient norms.  The weights are G17's (oracle.swinir_oracle.random_state_dict, its weight_seed /
weight_scale) and are not stored; data only, nothing of the reference's program text.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_golden_wsmall import SCALE, SEED, WSMALL, weight_sha1  # noqa: E402
from oracle import swinir_oracle as O  # noqa: E402
from oracle.make_golden import build_ref_model, save  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

HW = (16, 19)
X_SEED, T_SEED = 1901, 1902


def batch(cfg):
    """the recorded-seed batch: input in [0, 1] and a target at the output size (tests rebuild it from the seeds)"""
    x = torch.rand(2, cfg.in_chans, *HW, generator=torch.Generator().manual_seed(X_SEED))
    t = torch.rand(2, cfg.in_chans, HW[0] * cfg.upscale, HW[1] * cfg.upscale, generator=torch.Generator().manual_seed(T_SEED))
    return x, t


def main():
    ns = import_reference("network_swinir")
    arrays = {}
    for tag, kw in WSMALL.items():
        cfg = O.SwinIRConfig(**kw)
        sd = O.random_state_dict(cfg, seed=SEED, scale=SCALE)
        m = build_ref_model(ns, cfg, sd)          # drop_path_rate 0
        m.train()
        x, t = batch(cfg)
        loss = torch.nn.functional.l1_loss(m(x), t)
        loss.backward()
        names = [n for n, _ in m.named_parameters()]
        assert names == O.param_keys(cfg), "parameter order differs from the oracle's"
        arrays[f"{tag}.weight_sha1"] = np.array(weight_sha1(sd))
        arrays[f"{tag}.loss"] = np.array(float(loss), dtype=np.float64)
        arrays[f"{tag}.grad_norms"] = np.array([float(p.grad.double().norm()) for _, p in m.named_parameters()], dtype=np.float64)
        for n, p in m.named_parameters():
            arrays[f"{tag}.grad.{n}"] = p.grad.numpy().astype(np.float32)
    arrays["weight_seed"], arrays["weight_scale"] = np.array(SEED), np.array(SCALE)
    arrays["x_seed"], arrays["t_seed"], arrays["hw"] = np.array(X_SEED), np.array(T_SEED), np.array(HW)
    save("g19_swinir_wsmall_train", **arrays)


if __name__ == "__main__":
    main()
