"""Generate tests/golden/g20_scales*.npz by running the REFERENCE's SwinIR / HAT / DAT at the scales the command lines did not reach:
x3 and x8, and the one-step 'pixelshuffledirect' head with more than 16 output channels (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/make_golden_scales.py   (from the repo root)

G20: tiny models (the TINY / HAT_TINY / DAT_TINY widths of tests/test_oracle_golden.py) in eval mode on a 16 x 16 input and on an
11 x 13 input (reflect padding and crop for SwinIR / HAT; DAT pads inside its attention), both from recorded seeds:

    psd3, psd4     SwinIR 'pixelshuffledirect' x3 / x4, RGB          (27 / 48 head channels)
    psd8g          SwinIR 'pixelshuffledirect' x8, gray              (64 head channels: the engine's cap)
    ps8            SwinIR 'pixelshuffle' x8 (three x2 stages)
    hat3           HAT x3
    dat3           DAT x3

The weights are the oracles' random_state_dict (seed and scale recorded, a digest stored) and are not stored themselves; data only,
nothing of the reference's program text.  tests/golden_scales.py restates the configurations for the tests.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_scales import CASES, NAME, SIZES, config, weights  # noqa: E402
from oracle.make_golden import save, sha1  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

REF = {"swinir": ("network_swinir", "SwinIR"), "hat": ("hat_arch", "HAT"), "dat": ("dat_arch", "DAT")}


def main():
    arrays = {}
    for tag, (family, _, batch, seed, scale) in CASES.items():
        cfg = config(tag)
        sd = weights(tag)
        mod = import_reference(REF[family][0])
        torch.manual_seed(0)
        kw = cfg.kwargs()
        m = getattr(mod, REF[family][1])(**({**kw, "drop_path_rate": 0.0}))
        assert list(m.state_dict().keys()) == list(sd.keys()), f"{tag}: schema order drifted"
        missing, unexpected = m.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        m.eval()
        arrays[f"{tag}.weight_seed"], arrays[f"{tag}.weight_scale"] = np.array(seed), np.array(scale)
        arrays[f"{tag}.weight_sha1"] = np.array(sha1(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()])))
        for hw in SIZES:
            x = torch.rand(batch, cfg.in_chans, *hw, generator=torch.Generator().manual_seed(2000 + hw[0] * 100 + hw[1]))
            with torch.no_grad():
                y = m(x)
            assert tuple(y.shape) == (batch, cfg.in_chans, hw[0] * cfg.upscale, hw[1] * cfg.upscale), (tag, hw, tuple(y.shape))
            arrays[f"{tag}.x_{hw[0]}x{hw[1]}"] = x.numpy()
            arrays[f"{tag}.y_{hw[0]}x{hw[1]}"] = y.numpy().astype(np.float32)
            print(tag, hw, "max|y|", float(y.abs().max()))
    save(NAME, **arrays)


if __name__ == "__main__":
    main()
