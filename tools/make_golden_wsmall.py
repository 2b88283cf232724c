"""Generate tests/golden/g17_swinir_wsmall*.npz by running the REFERENCE's SwinIR at window sizes below 8 (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/make_golden_wsmall.py   (from the repo root)

G17: tiny SwinIR models (embed 24, depths (2, 2), heads (2, 2), mlp_ratio 2) at window_size 7 -- the constructor's default and the
window of the SwinIR JPEG-artifact models -- and 4: the '' head of the JPEG models (in_chans 1, upscale 1, img_range 255), both
pixel-shuffle heads, at img_size (one mask set), at a larger size (masks recomputed for the map, network_swinir.py:253-257) and at a
size that needs the reflect padding of check_image_size (:783-788).  Weights come from oracle.swinir_oracle.random_state_dict
(seed 17, scale 3.0) and are pinned by their SHA-1, as in G16.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import swinir_oracle as O  # noqa: E402
from oracle.make_golden import build_ref_model, save, sha1  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

TINY = dict(embed_dim=24, depths=(2, 2), num_heads=(2, 2), mlp_ratio=2, resi_connection="1conv")
# tag -> constructor options (kept in step with tests/test_oracle_golden_wsmall.py::WSMALL)
WSMALL = {
    "car": dict(TINY, window_size=7, img_size=14, in_chans=1, upscale=1, img_range=255.0, upsampler=""),
    "ps": dict(TINY, window_size=7, img_size=14, in_chans=3, upscale=2, img_range=1.0, upsampler="pixelshuffle"),
    "psd": dict(TINY, window_size=7, img_size=14, in_chans=3, upscale=2, img_range=1.0, upsampler="pixelshuffledirect"),
    "ws4": dict(TINY, window_size=4, img_size=12, in_chans=3, upscale=2, img_range=1.0, upsampler="pixelshuffle"),
}
SIZES = ((14, 14), (21, 28), (16, 19))
SEED, SCALE = 17, 3.0


def weight_sha1(sd) -> str:
    return sha1(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()]))


def main():
    ns = import_reference("network_swinir")
    arrays = {}
    for tag, kw in WSMALL.items():
        cfg = O.SwinIRConfig(**kw)
        sd = O.random_state_dict(cfg, seed=SEED, scale=SCALE)
        m = build_ref_model(ns, cfg, sd)
        assert list(m.state_dict().keys()) == [k for k, _, _ in O.state_dict_schema(cfg)]
        arrays[f"{tag}.weight_sha1"] = np.array(weight_sha1(sd))
        for hw in SIZES:
            x = torch.rand(2, cfg.in_chans, *hw, generator=torch.Generator().manual_seed(hw[0] * 7 + hw[1]))
            with torch.no_grad():
                y = m(x)
            arrays[f"{tag}.x_{hw[0]}x{hw[1]}"], arrays[f"{tag}.y_{hw[0]}x{hw[1]}"] = x.numpy(), y.numpy()
    arrays["weight_seed"], arrays["weight_scale"] = np.array(SEED), np.array(SCALE)
    save("g17_swinir_wsmall", **arrays)


if __name__ == "__main__":
    main()
