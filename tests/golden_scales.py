"""The tiny models of the G20 fixture (tools/make_golden_scales.py): x3, x8 and the wide one-step head, shared by the generator, the CPU
oracle test (tests/test_oracle_golden_scales.py) and the GPU tests (tests/test_gpu_wide_head.py)."""
import hashlib

import numpy as np

from conftest import load_golden

NAME = "g20_scales"
SIZES = ((16, 16), (11, 13))
TINY = dict(img_size=16, in_chans=3, embed_dim=24, depths=(2, 2), num_heads=(2, 2), window_size=8, mlp_ratio=2, img_range=1.0, resi_connection="1conv")
HAT_TINY = dict(img_size=32, in_chans=3, embed_dim=24, depths=(2, 2), num_heads=(2, 2), window_size=16, compress_ratio=3, squeeze_factor=6,
                conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=2.0, upscale=3, img_range=1.0, upsampler="pixelshuffle")
DAT_TINY = dict(img_size=32, in_chans=3, embed_dim=48, split_size=(8, 32), depth=(3, 2), num_heads=(4, 4), expansion_factor=2.0, upscale=3,
                img_range=1.0, resi_connection="1conv", upsampler="pixelshuffle")
# tag: (family, config keywords, batch, weight seed, weight scale)
CASES = {
    "psd3": ("swinir", dict(TINY, upscale=3, upsampler="pixelshuffledirect"), 2, 20, 1.5),
    "psd4": ("swinir", dict(TINY, upscale=4, upsampler="pixelshuffledirect"), 2, 20, 1.5),
    "psd8g": ("swinir", dict(TINY, upscale=8, upsampler="pixelshuffledirect", in_chans=1), 2, 20, 1.5),
    "ps8": ("swinir", dict(TINY, upscale=8, upsampler="pixelshuffle"), 1, 20, 1.5),
    "hat3": ("hat", HAT_TINY, 1, 13, 2.0),
    "dat3": ("dat", DAT_TINY, 1, 14, 2.0),
}


def _oracle(family):
    if family == "swinir":
        from oracle import swinir_oracle as M
        return M, M.SwinIRConfig, M.swinir_forward
    if family == "hat":
        from oracle import hat_oracle as M
        return M, M.HATConfig, M.hat_forward
    from oracle import dat_oracle as M
    return M, M.DATConfig, M.dat_forward


def config(tag):
    family, kw = CASES[tag][:2]
    return _oracle(family)[1](**kw)


def weights(tag):
    family, _, _, seed, scale = CASES[tag]
    return _oracle(family)[0].random_state_dict(config(tag), seed=seed, scale=scale)


def forward(tag):
    """the CPU oracle's forward of the tag's family: (sd, cfg, x) -> y"""
    return _oracle(CASES[tag][0])[2]


def checked_weights(tag):
    """-> (golden, cfg, sd); the weights are regenerated from the recorded seed and held to the stored digest"""
    g = load_golden(NAME)
    sd = weights(tag)
    digest = hashlib.sha1(np.ascontiguousarray(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()])).tobytes()).hexdigest()
    assert digest == str(g[f"{tag}.weight_sha1"]), f"{tag}: weight generator drifted from the one the fixtures were made with"
    return g, config(tag), sd
