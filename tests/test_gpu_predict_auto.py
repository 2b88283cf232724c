"""predict.main --arch auto --scale auto on the device: saved tiny checkpoints of the three families, one per envelope kind, on four small
files (L, RGB, RGBA 19 x 23, I;16).  Every written file equals pack(model_path(unpack(file))) composed with the ops and a model
constructed from the KNOWN keywords, byte for byte (the method of tests/test_gpu_predict.py); --tile and --self_ensemble once each; a
DAT-light-shaped file raises before any file is written."""
from functools import partial

import numpy as np
import pytest
import torch
from PIL import Image

from tpu_superresolution_amd import augment as A
from tpu_superresolution_amd import ops
from tpu_superresolution_amd import predict as P
from tpu_superresolution_amd import tiling as T
from tpu_superresolution_amd._lib import SrkUnsupported

pytestmark = pytest.mark.gpu

FILES = [("a_gray.png", "L", (24, 20), np.uint8), ("b_rgb.png", "RGB", (24, 20, 3), np.uint8), ("d_rgba.png", "RGBA", (19, 23, 4), np.uint8),
         ("e_gray16.png", "I;16", (16, 16), np.uint16)]
SWIN = dict(img_size=16, in_chans=3, embed_dim=24, depths=(2, 2), num_heads=(2, 2), window_size=8, mlp_ratio=2, img_range=1.0, resi_connection="1conv")
# kind: (family, known keywords, envelope, weight seed)
KINDS = {
    "light4": ("swinir", dict(SWIN, upscale=4, upsampler="pixelshuffledirect"), "params_ema", 31),
    "real3conv4": ("swinir", dict(SWIN, embed_dim=32, num_heads=(8, 8), upscale=4, upsampler="nearest+conv", resi_connection="3conv"), "params", 32),
    "hat3": ("hat", dict(img_size=64, in_chans=3, embed_dim=24, depths=(2, 2), num_heads=(2, 2), window_size=16, compress_ratio=3, squeeze_factor=6,
                         conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=2.0, upscale=3, img_range=1.0, upsampler="pixelshuffle"), "model", 33),
    "dats2": ("dat", dict(img_size=32, in_chans=3, embed_dim=48, split_size=(8, 16), depth=(3, 2), num_heads=(4, 4), expansion_factor=2.0, upscale=2,
                          img_range=1.0, resi_connection="1conv", upsampler="pixelshuffle"), None, 34),
    "dn_gray": ("swinir", dict(SWIN, in_chans=1, upscale=1, upsampler=""), "params", 35),
    "jpeg_gray": ("swinir", dict(SWIN, in_chans=1, upscale=1, upsampler="", window_size=7, img_size=21, img_range=255.0), "params_ema", 36),
}


def _rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, size=shape, dtype=np.uint32).astype(dtype)


@pytest.fixture(scope="module")
def image_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("lq")
    arrays = {}
    for i, (name, mode, shape, dtype) in enumerate(FILES):
        a = _rand(shape, dtype, seed=40 + i)
        if mode == "I;16":
            Image.frombytes("I;16", (shape[1], shape[0]), a.astype("<u2").tobytes()).save(d / name)
        else:
            Image.fromarray(a, mode=mode).save(d / name)
        arrays[name] = a
    return d, arrays


def _known(kind):
    """-> (state_dict, a constructor of the model from the known keywords)"""
    import tpu_superresolution_amd as pkg
    family, kw, _, seed = KINDS[kind]
    if family == "swinir":
        from oracle import swinir_oracle as O
        cfg = O.SwinIRConfig(**kw)
        return O.random_state_dict(cfg, seed=seed, scale=1.5), lambda: pkg.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
    if family == "hat":
        from oracle import hat_oracle as O
        cfg = O.HATConfig(**kw)
        return O.random_state_dict(cfg, seed=seed, scale=2.0), lambda: pkg.HAT(**cfg.kwargs())
    from oracle import dat_oracle as O
    cfg = O.DATConfig(**kw)
    return O.random_state_dict(cfg, seed=seed, scale=2.0), lambda: pkg.DAT(**cfg.kwargs())


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """{kind: (checkpoint path, the model of the known keywords on the device)}"""
    d = tmp_path_factory.mktemp("ckpt")
    out = {}
    for kind, (_, _, envelope, _) in KINDS.items():
        sd, make = _known(kind)
        torch.save(sd if envelope is None else {envelope: sd, "iter": 1}, d / f"{kind}.pt")
        m = make()
        m.load_state_dict(sd, strict=True)
        out[kind] = (str(d / f"{kind}.pt"), m.cuda().eval())
    return out


def _written_out(model_path, a, scale, channels):
    """One image through the ops: unpack -> model path -> pack (alpha resized beside the model)."""
    a4 = a[None, :, :, None] if a.ndim == 2 else a[None]
    H, W, ch = a4.shape[1:]
    raw = torch.from_numpy(a4.view(np.int16)).view(torch.uint16) if a4.dtype == np.uint16 else torch.from_numpy(a4)
    with torch.no_grad():
        x, alpha = ops.image_unpack(raw.cuda(), channels, want_alpha=True)
        pred = model_path(x).float()
        assert tuple(pred.shape[-2:]) == (H * scale, W * scale)
        if alpha is not None and scale != 1:
            alpha = ops.resize_aa(alpha, (H * scale, W * scale))
        out = ops.image_pack(pred.contiguous(), alpha, out_chans=ch, bits=8 * a.dtype.itemsize)[0].cpu()
    return out.view(torch.int16).numpy().view(np.uint16) if out.dtype == torch.uint16 else out.numpy()


def _check_outputs(out_dir, arrays, model_path, scale, channels):
    for name, mode, _, _ in FILES:
        with Image.open(out_dir / (name[:-4] + "_sr.png")) as im:
            got_mode, got = im.mode, np.asarray(im)
        want = _written_out(model_path, arrays[name], scale, channels)
        assert got_mode == mode, name
        assert got.dtype == want.dtype and np.array_equal(got.reshape(want.shape), want), f"{name}: the file differs from the written-out composition"


def _main(ckpt, image_dir, out_dir, *extra):
    return P.main(["--input", str(image_dir), "--output", str(out_dir), "--arch", "auto", "--scale", "auto", "--ckpt", ckpt, "--device", "cuda", *extra])


@pytest.mark.parametrize("kind", list(KINDS))
def test_predict_auto_equals_the_model_of_the_known_keywords(tmp_path, capsys, image_dir, checkpoints, kind):
    d, arrays = image_dir
    ckpt, model = checkpoints[kind]
    family, kw, envelope, _ = KINDS[kind]
    r = _main(ckpt, d, tmp_path / "o")
    out = capsys.readouterr().out
    assert r["n"] == len(FILES)
    assert ("[ckpt] loaded raw state_dict" if envelope is None else f"[ckpt] loaded state_dict from '{envelope}' key") in out
    name = {"swinir": "SwinIR", "hat": "HAT", "dat": "DAT"}[family]
    assert f"[arch] {family}: {name}(" in out and f"upscale={kw['upscale']}" in out and f"in_chans={kw['in_chans']}, embed_dim={kw['embed_dim']}" in out
    assert "[arch] note: img_range=" in out and (kind != "jpeg_gray" or "img_range=255.0" in out)
    assert (f"[predict] b_rgb.png 24x20 RGB 8 -> {24 * kw['upscale']}x{20 * kw['upscale']} |") in out
    _check_outputs(tmp_path / "o", arrays, model, kw["upscale"], kw["in_chans"])


@pytest.mark.parametrize("extra,path_of", [
    (("--tile", "16", "--tile_overlap", "4"), lambda m: partial(T.tiled_forward, m, tile=16, overlap=4)),
    (("--self_ensemble",), lambda m: partial(A.self_ensemble, m))], ids=["tiled", "self_ensemble"])
def test_predict_auto_tiled_and_self_ensembled(tmp_path, capsys, image_dir, checkpoints, extra, path_of):
    d, arrays = image_dir
    ckpt, model = checkpoints["light4"]
    r = _main(ckpt, d, tmp_path / "o", *extra)
    out = capsys.readouterr().out
    assert r["n"] == len(FILES) and (("[tile] 16 overlap 4" in out) or ("[self_ensemble] x8" in out))
    _check_outputs(tmp_path / "o", arrays, path_of(model), 4, 3)


def test_explicit_scale_must_be_the_files(tmp_path, image_dir, checkpoints):
    d, arrays = image_dir
    ckpt, model = checkpoints["hat3"]
    with pytest.raises(SystemExit, match=r"--scale X4 does not match the checkpoint: .* is a x3 model"):
        P.main(["--input", str(d), "--output", str(tmp_path / "o"), "--arch", "auto", "--scale", "X4", "--ckpt", ckpt, "--device", "cuda"])
    assert not (tmp_path / "o").exists()
    r = P.main(["--input", str(d / "b_rgb.png"), "--output", str(tmp_path / "o"), "--arch", "auto", "--scale", "X3", "--ckpt", ckpt, "--device", "cuda"])
    assert r["n"] == 1


def test_dat_light_shaped_file_raises_before_any_file_is_written(tmp_path, image_dir):
    import tpu_superresolution_amd as pkg
    d, _ = image_dir
    sd = pkg.DAT(img_size=32, in_chans=3, embed_dim=32, split_size=[8, 32], depth=[4], num_heads=[2], expansion_factor=2, upscale=4, resi_connection="3conv",
                 upsampler="pixelshuffledirect", drop_path_rate=0.0).state_dict()
    torch.save({"params": sd}, tmp_path / "light.pt")
    with pytest.raises(SrkUnsupported, match=r"DAT\(.*depth=\[4\].*does not cover resi_connection='3conv'"):
        _main(str(tmp_path / "light.pt"), d, tmp_path / "o")
    assert not (tmp_path / "o").exists()
