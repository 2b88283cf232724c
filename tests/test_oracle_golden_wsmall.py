"""G17: the CPU oracle at window sizes below 8 against the reference's own SwinIR (fixture from tools/make_golden_wsmall.py)."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import swinir_oracle as O

TINY = dict(embed_dim=24, depths=(2, 2), num_heads=(2, 2), mlp_ratio=2, resi_connection="1conv")
WSMALL = {
    "car": dict(TINY, window_size=7, img_size=14, in_chans=1, upscale=1, img_range=255.0, upsampler=""),
    "ps": dict(TINY, window_size=7, img_size=14, in_chans=3, upscale=2, img_range=1.0, upsampler="pixelshuffle"),
    "psd": dict(TINY, window_size=7, img_size=14, in_chans=3, upscale=2, img_range=1.0, upsampler="pixelshuffledirect"),
    "ws4": dict(TINY, window_size=4, img_size=12, in_chans=3, upscale=2, img_range=1.0, upsampler="pixelshuffle"),
}
SIZES = ((14, 14), (21, 28), (16, 19))


def wsmall_weights(tag):
    g = load_golden("g17_swinir_wsmall")
    cfg = O.SwinIRConfig(**WSMALL[tag])
    sd = O.random_state_dict(cfg, seed=int(g["weight_seed"]), scale=float(g["weight_scale"]))
    digest = hashlib.sha1(np.ascontiguousarray(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()]))
                          .tobytes()).hexdigest()
    assert digest == str(g[f"{tag}.weight_sha1"])
    return g, cfg, sd


@pytest.mark.parametrize("tag", sorted(WSMALL))
def test_g17_small_window_forward(tag):
    """The oracle at window_size 7 / 4 (49- / 16-token windows, masks recomputed off img_size, reflect padding to a multiple of the
    window, the '' head of the JPEG models with img_range 255) against the reference."""
    g, cfg, sd = wsmall_weights(tag)
    for hw in SIZES:
        x = torch.from_numpy(g[f"{tag}.x_{hw[0]}x{hw[1]}"])
        with torch.no_grad():
            y = O.swinir_forward(sd, cfg, x)
        ref = torch.from_numpy(g[f"{tag}.y_{hw[0]}x{hw[1]}"])
        assert y.shape == ref.shape == (2, cfg.in_chans, hw[0] * cfg.upscale, hw[1] * cfg.upscale)
        assert float((y - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), (tag, hw)


def test_g17_models_build_at_small_windows_with_strict_state_dicts():
    """The package's SwinIR at these window sizes holds exactly the reference's state_dict (CPU: construction and loading only)."""
    import tpu_superresolution_amd as T
    for tag in WSMALL:
        _, cfg, sd = wsmall_weights(tag)
        m = T.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
        missing, unexpected = m.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
