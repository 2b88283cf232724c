"""The tiny light-width SwinIR of the one-step-head tests (tests/test_gpu_wide_head.py) and of tools/record_head_controls.py, which
records the output digests of the control cases on the commit before the head was widened."""
import hashlib

import numpy as np
import torch

from oracle import swinir_oracle as O

WIDE = ((3, 3), (4, 3), (8, 1), (5, 1))          # (upscale, in_chans): 27 (ragged second n-block), 48, 64 (the cap), 25 head channels
CONTROLS = ((4, 1), (2, 3))                      # 16 and 12 head channels: the path that was there before
SIZES = ((8, 8), (11, 13))
BATCH = 2
IMG_RANGE = 2.0                                  # 1 / img_range = 0.5 is exact in fp32 and is not 1: a dropped factor shows


def config(s, c):
    return O.SwinIRConfig(img_size=16, in_chans=c, embed_dim=60, depths=(2,), num_heads=(6,), window_size=8, mlp_ratio=2, upscale=s,
                          img_range=IMG_RANGE, upsampler="pixelshuffledirect", resi_connection="1conv")


def state(s, c):
    """seeded weights; the head's weight and bias are bf16-representable, so the kernel's operands are the reference's operands"""
    sd = O.random_state_dict(config(s, c), seed=100 * s + c, scale=1.5)
    for k in ("upsample.0.weight", "upsample.0.bias"):
        sd[k] = sd[k].to(torch.bfloat16).float()
    return sd


def model(s, c):
    import tpu_superresolution_amd as T
    m = T.SwinIR(drop_path_rate=0.0, **config(s, c).kwargs())
    m.load_state_dict(state(s, c), strict=True)
    return m.cuda().eval()


def image(c, hw):
    return torch.rand(BATCH, c, *hw, generator=torch.Generator().manual_seed(7000 + 100 * hw[0] + hw[1] + c))


def digest(y: torch.Tensor) -> str:
    return hashlib.sha1(np.ascontiguousarray(y.detach().cpu().numpy()).tobytes()).hexdigest()


def key(s, c, hw) -> str:
    return f"s{s}_c{c}_{hw[0]}x{hw[1]}"
