"""predict.main on the device with the tiny SwinIR / HAT of tests/test_gpu_tile.py: every written file equals
pack(resize(model_path(unpack(file)))) written out with the ops ONE IMAGE AT A TIME, byte for byte -- plain, tiled, self-ensembled,
with --outscale, with the 'nearest+conv' head -- and the non-finite guard writes nothing."""
from functools import partial

import numpy as np
import pytest
import torch
from PIL import Image

from tpu_superresolution_amd import augment as A
from tpu_superresolution_amd import ops
from tpu_superresolution_amd import predict as P
from tpu_superresolution_amd import tiling as T

pytestmark = pytest.mark.gpu


def _rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, size=shape, dtype=np.uint32).astype(dtype)


FILES = [("a_gray.png", "L", (24, 20), np.uint8), ("b_rgb.png", "RGB", (24, 20, 3), np.uint8), ("c_rgb.png", "RGB", (24, 20, 3), np.uint8),
         ("d_rgba.png", "RGBA", (19, 23, 4), np.uint8), ("e_gray16.png", "I;16", (16, 16), np.uint16)]


@pytest.fixture(scope="module")
def image_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("lq")
    arrays = {}
    for i, (name, mode, shape, dtype) in enumerate(FILES):
        a = _rand(shape, dtype, seed=i)
        if mode == "I;16":
            Image.frombytes("I;16", (shape[1], shape[0]), a.astype("<u2").tobytes()).save(d / name)
        else:
            Image.fromarray(a, mode=mode).save(d / name)
        arrays[name] = a
    return d, arrays


def _tiny(kind):
    import tpu_superresolution_amd as pkg
    from test_oracle_golden import hat_tiny_weights, tiny_weights
    if kind == "hat":
        _, cfg, sd = hat_tiny_weights()
        return lambda: pkg.HAT(**cfg.kwargs()), sd
    _, cfg, sd = tiny_weights(kind)
    return lambda: pkg.SwinIR(drop_path_rate=0.0, **cfg.kwargs()), sd


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """{kind: (constructor, checkpoint path, the loaded model)} -- seeded random weights saved as a 'params' envelope."""
    d = tmp_path_factory.mktemp("ckpt")
    out = {}
    for kind in ("ps4", "hat", "nc4"):
        make, sd = _tiny(kind)
        torch.save({"params": sd}, d / f"{kind}.pt")
        m = make()
        m.load_state_dict(sd, strict=True)
        out[kind] = (make, str(d / f"{kind}.pt"), m.cuda().eval())
    return out


def _written_out(model_path, a, scale, outscale=None):
    """One image through the ops: unpack -> model path -> resize -> pack."""
    a4 = a[None, :, :, None] if a.ndim == 2 else a[None]
    H, W, ch = a4.shape[1:]
    raw = torch.from_numpy(a4.view(np.int16)).view(torch.uint16) if a4.dtype == np.uint16 else torch.from_numpy(a4)
    with torch.no_grad():
        x, alpha = ops.image_unpack(raw.cuda(), 3, want_alpha=True)
        pred = model_path(x).float()
        size = P.out_size(H, W, float(scale if outscale is None else outscale))
        if tuple(pred.shape[-2:]) != size:
            pred = ops.resize_aa(pred.contiguous(), size)
        if alpha is not None:
            alpha = ops.resize_aa(alpha, size)
        out = ops.image_pack(pred.contiguous(), alpha, out_chans=ch, bits=8 * a.dtype.itemsize)[0].cpu()
    return out.view(torch.int16).numpy().view(np.uint16) if out.dtype == torch.uint16 else out.numpy()


def _read(path):
    with Image.open(path) as im:
        return im.mode, np.asarray(im)


def _check_outputs(out_dir, arrays, model_path, scale, outscale=None):
    for name, mode, _, _ in FILES:
        got_mode, got = _read(out_dir / (name[:-4] + "_sr.png"))
        want = _written_out(model_path, arrays[name], scale, outscale)
        assert got_mode == mode, name
        assert got.dtype == want.dtype and np.array_equal(got.reshape(want.shape), want), f"{name}: the file differs from the written-out composition"


def _main(monkeypatch, make, ckpt, image_dir, out_dir, *extra):
    monkeypatch.setattr(P, "build_model", lambda args, scale_int: make())
    return P.main(["--input", str(image_dir), "--output", str(out_dir), "--arch", "swinir", "--scale", "X4", "--ckpt", ckpt, "--device", "cuda",
                   "--param_key", "params", *extra])


@pytest.mark.parametrize("extra,path_of,outscale", [
    ((), lambda m: m, None),
    (("--batch_size", "2"), lambda m: m, None),
    (("--tile", "16", "--tile_overlap", "4", "--batch_size", "2"), lambda m: partial(T.tiled_forward, m, tile=16, overlap=4), None),
    (("--self_ensemble",), lambda m: partial(A.self_ensemble, m), None),
    (("--outscale", "3", "--batch_size", "2"), lambda m: m, 3.0),
], ids=["plain", "grouped", "tiled", "self_ensemble", "outscale3"])
def test_predict_main_on_a_small_swinir(monkeypatch, tmp_path, capsys, image_dir, checkpoints, extra, path_of, outscale):
    d, arrays = image_dir
    make, ckpt, model = checkpoints["ps4"]
    r = _main(monkeypatch, make, ckpt, d, tmp_path / "o", *extra)
    out = capsys.readouterr().out
    grouped = "--batch_size" in extra
    assert r["n"] == 5 and r["groups"] == ([1, 2, 1, 1] if grouped else [1] * 5)          # the two RGB files share a model call
    assert "[ckpt] loaded state_dict from 'params' key" in out and "[done] 5 images |" in out
    assert ("[tile] 16 overlap 4 batch 1 blend mean" in out) == ("--tile" in extra) and ("[self_ensemble] x8" in out) == ("--self_ensemble" in extra)
    size = "72x60" if outscale else "96x80"
    assert f"[predict] b_rgb.png 24x20 RGB 8 -> {size} |" in out and f"[predict] e_gray16.png 16x16 I;16 16 -> {'48x48' if outscale else '64x64'} |" in out
    _check_outputs(tmp_path / "o", arrays, path_of(model), 4, outscale)
    if not extra:          # negative control: the files are not the truncation of save_tensor_as_png
        want = _written_out(model, arrays["b_rgb.png"], 4)
        with torch.no_grad():
            y = model(ops.image_unpack(torch.from_numpy(arrays["b_rgb.png"]).cuda(), 3)[0])
        trunc = y[0].clamp(0, 1).mul(255).byte().permute(1, 2, 0).cpu().numpy()
        assert (trunc != want).any()


def test_predict_main_on_a_small_hat(monkeypatch, tmp_path, image_dir, checkpoints):
    d, arrays = image_dir
    make, ckpt, model = checkpoints["hat"]
    r = _main(monkeypatch, make, ckpt, d, tmp_path / "o")
    assert r["n"] == 5
    _check_outputs(tmp_path / "o", arrays, model, 4)


def test_nearest_conv_head(monkeypatch, tmp_path, image_dir, checkpoints):
    d, arrays = image_dir
    make, ckpt, model = checkpoints["nc4"]
    built = []
    monkeypatch.setattr(P, "build_real_sr_model", lambda scale_int: (built.append(scale_int), make())[1])
    r = P.main(["--input", str(d), "--output", str(tmp_path / "o"), "--arch", "swinir", "--scale", "X4", "--ckpt", ckpt, "--device", "cuda",
                "--upsampler", "nearest+conv"])
    assert r["n"] == 5 and built == [4]
    _check_outputs(tmp_path / "o", arrays, model, 4)


def test_non_finite_guard_writes_no_file(monkeypatch, tmp_path, image_dir, checkpoints):
    d, _ = image_dir
    make, ckpt, _ = checkpoints["ps4"]

    def make_bad():
        m = make()

        def plant(mod, inp, out):
            out = out.clone()
            out[0, 0, 0, 0] = float("nan")
            return out
        m.register_forward_hook(plant)
        return m

    with pytest.raises(RuntimeError, match=r"non-finite values: count=1 in a_gray\.png"):
        _main(monkeypatch, make_bad, ckpt, d, tmp_path / "o")
    assert list((tmp_path / "o").iterdir()) == []
