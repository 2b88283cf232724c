"""Generate tests/golden/g21_wide_head_train*.npz: loss and parameter gradients of the REFERENCE's SwinIR in train mode for the
one-step 'pixelshuffledirect' heads wider than 16 channels (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/make_golden_wide_head_train.py   (from the repo root)

G21: the psd3 / psd4 / psd8g models of tests/golden_scales.py (27 / 48 / 64 head channels) in TRAIN mode with drop_path_rate = 0, on
one seeded 16 x 16 input and one seeded 11 x 13 input (reflect padding and crop) with a seeded target each: F.l1_loss(model(x), t) and
its gradient with respect to every parameter.  The weights are the oracle's random_state_dict from the recorded seed (a digest is
stored, as in G20) and are not stored themselves; data only, nothing of the reference's program text.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_scales import CASES, config, weights  # noqa: E402
from oracle.make_golden import save, sha1  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402
from wide_head_ref import G21_NAME, G21_SIZES, G21_TAGS, g21_input, g21_target  # noqa: E402


def main():
    arrays = {}
    mod = import_reference("network_swinir")
    for tag in G21_TAGS:
        _, _, batch, seed, scale = CASES[tag]
        cfg = config(tag)
        sd = weights(tag)
        torch.manual_seed(0)
        m = mod.SwinIR(**{**cfg.kwargs(), "drop_path_rate": 0.0})
        assert list(m.state_dict().keys()) == list(sd.keys()), f"{tag}: schema order drifted"
        missing, unexpected = m.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        m.train()
        arrays[f"{tag}.weight_seed"], arrays[f"{tag}.weight_scale"] = np.array(seed), np.array(scale)
        arrays[f"{tag}.weight_sha1"] = np.array(sha1(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()])))
        for hw in G21_SIZES:
            x, t = g21_input(tag, hw), g21_target(tag, hw)
            m.zero_grad(set_to_none=True)
            y = m(x)
            assert tuple(y.shape) == tuple(t.shape), (tag, hw, tuple(y.shape))
            loss = torch.nn.functional.l1_loss(y, t)
            loss.backward()
            key = f"{tag}.{hw[0]}x{hw[1]}"
            arrays[f"{key}.x"], arrays[f"{key}.target"] = x.numpy(), t.numpy()
            arrays[f"{key}.loss"] = np.array(float(loss.detach()), dtype=np.float64)
            for n, p in m.named_parameters():
                assert p.grad is not None, (tag, n)
                arrays[f"{key}.grad.{n}"] = p.grad.detach().numpy().astype(np.float32)
            print(tag, hw, "loss", float(loss.detach()), "max|dW_head|", float(m.upsample[0].weight.grad.abs().max()))
    save(G21_NAME, **arrays)


if __name__ == "__main__":
    main()
