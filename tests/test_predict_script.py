"""predict.py without a GPU: the parser, file discovery and naming, grouping, and `predict.upscale` / `predict.run` on the CPU with an
exact stub model (nearest-neighbour x2 in torch).  Written files are read back with PIL and compared byte for byte with the
written-out composition of the numpy restatement (tests/image_io_ref.py)."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

import image_io_ref as R
from tpu_superresolution_amd import predict as P

BASE = ["--input", "in", "--output", "out", "--arch", "swinir", "--scale", "X2", "--ckpt", "w.pt"]


class Stub:
    """x2 nearest neighbour: exact, any channel count; records the batch sizes it saw."""

    def __init__(self, scale=2):
        self.scale, self.calls = scale, []

    def __call__(self, x):
        self.calls.append(x.shape[0])
        return x.repeat_interleave(self.scale, 2).repeat_interleave(self.scale, 3)


def _rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, size=shape, dtype=np.uint32).astype(dtype)


def _expected(a, channels=3, scale=2, bits=None):
    """unpack -> nearest x scale -> pack, written out with the restatement for ONE image.  Alpha does not go through the model: it is
    resized to the output size by the antialiased bicubic (on the CPU torch's own, the convention ops.resize_aa restates).
    That is the call predict._resize makes for a CPU tensor, so these CPU tests pin where the alpha plane goes (its slot, its size,
    its quantisation) and not the resampling itself; tests/test_gpu_predict.py holds the device path to ops.resize_aa, which
    tests/test_gpu_resize.py holds to its own reference."""
    a4 = a[None, :, :, None] if a.ndim == 2 else a[None]
    x, alpha = R.unpack_ref(a4, channels, want_alpha=True)
    up = lambda t: np.repeat(np.repeat(t, scale, 2), scale, 3)
    if alpha is not None:
        alpha = torch.nn.functional.interpolate(torch.from_numpy(alpha), size=(a4.shape[1] * scale, a4.shape[2] * scale), mode="bicubic",
                                                antialias=True, align_corners=False).numpy()
    out, counts = R.pack_ref(up(x), alpha, out_chans=a4.shape[3], bits=bits or 8 * a.dtype.itemsize)
    return out[0], counts


def _args(**kw):
    d = dict(input="in", output="out", suffix="_sr", tile=0, tile_overlap=32, tile_batch=1, tile_blend="mean", self_ensemble=False,
             batch_size=1, outscale=None, out_bits="auto", channels=3)
    d.update(kw)
    return types.SimpleNamespace(**d)


# ---- parser ----------------------------------------------------------------------------------------------------------------------------
def test_parser_defaults():
    a = P.parse_args(BASE)
    assert (a.suffix, a.param_key, a.window_size, a.task, a.channels, a.upsampler) == ("_sr", "auto", 8, "sr", 3, "pixelshuffle")
    assert (a.tile, a.tile_overlap, a.tile_batch, a.tile_blend, a.self_ensemble) == (0, 32, 1, "mean", False)
    assert (a.batch_size, a.outscale, a.out_bits, a.device) == (1, None, "auto", None)
    car = P.parse_args(BASE[:6] + ["--scale", "X1", "--ckpt", "w.pt", "--task", "car"])
    assert car.window_size == 7


@pytest.mark.parametrize("extra", [
    ["--tile", "-1"], ["--tile", "16", "--tile_overlap", "16"], ["--tile_batch", "0"], ["--tile_overlap", "-1"],
    ["--window_size", "9"], ["--window_size", "1"], ["--batch_size", "0"], ["--outscale", "0"], ["--outscale", "nan"], ["--outscale", "-2"],
    ["--out_bits", "12"], ["--task", "dn"], ["--channels", "1"], ["--suffix", "a/b"], ["--upsampler", "nearest+conv", "--window_size", "7"],
    ["--tile_blend", "feather"], ["--param_key", "weights"], ["--upsampler", "bilinear"]])
def test_parser_refusals(extra):
    with pytest.raises(SystemExit):
        P.parse_args(BASE + extra)


def test_parser_refusals_by_arch_and_scale():
    hat = ["--input", "in", "--output", "out", "--arch", "hat", "--scale", "X2", "--ckpt", "w.pt"]
    for extra in (["--window_size", "7"], ["--upsampler", "nearest+conv"]):
        with pytest.raises(SystemExit):
            P.parse_args(hat + extra)
    with pytest.raises(SystemExit):
        P.parse_args(["--input", "in", "--output", "out", "--arch", "hat", "--scale", "X1", "--ckpt", "w.pt", "--task", "dn"])
    with pytest.raises(SystemExit):
        P.parse_args(["--input", "in", "--output", "out", "--arch", "swinir", "--scale", "X1", "--ckpt", "w.pt"])          # X1 without a task
    with pytest.raises(SystemExit):
        P.parse_args(BASE[:8])                                                                                           # no --ckpt
    ok = P.parse_args(["--input", "in", "--output", "out", "--arch", "swinir", "--scale", "X1", "--ckpt", "w.pt", "--task", "dn", "--channels", "1"])
    assert ok.channels == 1 and ok.window_size == 8
    assert P.parse_args(BASE + ["--upsampler", "nearest+conv"]).upsampler == "nearest+conv"


def test_real_sr_model_has_the_nearest_conv_head():
    from tpu_superresolution_amd.finetune_swinir import build_model
    m, base = P.build_real_sr_model(4), build_model(4)
    keys, base_keys = set(m.state_dict()), set(base.state_dict())
    assert m.upsampler == "nearest+conv" and m.window_size == 8 and m.embed_dim == 180
    assert {"conv_up1.weight", "conv_up2.weight", "conv_hr.weight", "conv_last.weight"} <= keys - {k for k in base_keys if k.startswith("upsample")}
    body = lambda ks: {k for k in ks if k.startswith(("layers.", "conv_first", "conv_after_body", "norm."))}
    assert body(keys) == body(base_keys)          # the same body as build_model: only the head differs


def test_arch_on_cpu_exits(tmp_path):
    with pytest.raises(SystemExit, match="HIP path only"):
        P.main(["--input", str(tmp_path), "--output", str(tmp_path / "o"), "--arch", "swinir", "--scale", "X2", "--ckpt", "none.pt", "--device", "cpu"])
    assert not (tmp_path / "o").exists()


# ---- files -----------------------------------------------------------------------------------------------------------------------------
def _write_dir(d):
    d.mkdir()
    Image.fromarray(_rand((6, 5, 3), np.uint8, 1), mode="RGB").save(d / "b.png")
    Image.fromarray(_rand((6, 5), np.uint8, 2), mode="L").save(d / "a.png")
    Image.fromarray(_rand((4, 4, 3), np.uint8, 3), mode="RGB").convert("P").save(d / "c_pal.png")
    Image.fromarray(_rand((4, 4), np.uint8, 4) > 127).save(d / "d_bilevel.png")
    Image.fromarray(_rand((4, 4, 4), np.uint8, 5), mode="CMYK").save(d / "e_cmyk.tif")
    (d / "notes.txt").write_text("not an image")
    (d / "sub").mkdir()
    Image.fromarray(_rand((3, 3), np.uint8, 6), mode="L").save(d / "sub" / "inner.png")


def test_discovery_order_skip_and_convert(tmp_path):
    d = tmp_path / "in"
    _write_dir(d)
    lines = []
    files = P.discover(d, log=lines.append)
    assert [p.name for p in files] == ["a.png", "b.png", "c_pal.png", "d_bilevel.png", "e_cmyk.tif"]          # sorted, not recursive
    assert sorted(lines) == sorted(["[skip] notes.txt: PIL cannot open it (UnidentifiedImageError)", "[skip] sub: not a file"])
    assert [p.name for p in P.discover(d / "b.png", log=lines.append)] == ["b.png"]
    with pytest.raises(FileNotFoundError):
        P.discover(d / "missing.png")
    conv = []
    modes = [P.load_image(p, log=conv.append)[1] for p in files]
    assert modes == ["L", "RGB", "RGB", "RGB", "RGB"]
    assert conv == ["[convert] c_pal.png: mode P -> RGB", "[convert] d_bilevel.png: mode 1 -> RGB", "[convert] e_cmyk.tif: mode CMYK -> RGB"]


def test_palette_with_transparency_becomes_rgba(tmp_path):
    img = Image.fromarray(_rand((4, 4, 3), np.uint8, 3), mode="RGB").convert("P")
    img.save(tmp_path / "t.png", transparency=0)
    conv = []
    a, mode = P.load_image(tmp_path / "t.png", log=conv.append)
    assert mode == "RGBA" and a.shape == (4, 4, 4) and conv == ["[convert] t.png: mode P -> RGBA"]


def test_naming_and_overwrite_refusal(tmp_path):
    assert P.output_path(tmp_path / "x.jpg", tmp_path / "o") == tmp_path / "o" / "x_sr.png"
    assert P.output_path(tmp_path / "x.png", tmp_path, "_x4") == tmp_path / "x_x4.png"
    with pytest.raises(ValueError, match="overwrite"):
        P.output_path(tmp_path / "x.png", tmp_path, "")
    # run() refuses before it writes anything
    Image.fromarray(_rand((4, 4), np.uint8, 1), mode="L").save(tmp_path / "x.png")
    stub = Stub()
    with pytest.raises(ValueError, match="overwrite"):
        P.run(stub, _args(input=str(tmp_path), output=str(tmp_path), suffix=""), 2, torch.device("cpu"))
    assert stub.calls == [] and sorted(p.name for p in tmp_path.iterdir()) == ["x.png"]
    # x.png and x.tif would share x_sr.png
    Image.fromarray(_rand((4, 4), np.uint8, 1), mode="L").save(tmp_path / "x.tif")
    with pytest.raises(ValueError, match="share one output"):
        P.run(stub, _args(input=str(tmp_path), output=str(tmp_path / "o")), 2, torch.device("cpu"))


# ---- upscale on the CPU with the exact stub --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape,dtype", [("L", (7, 5), np.uint8), ("LA", (7, 5, 2), np.uint8), ("RGB", (7, 5, 3), np.uint8),
                                              ("RGBA", (7, 5, 4), np.uint8), ("I;16", (7, 5), np.uint16)])
def test_every_mode_round_trips_through_files(tmp_path, mode, shape, dtype, capsys):
    a = _rand(shape, dtype, seed=len(mode))
    src = tmp_path / "img.png"
    if mode == "I;16":
        Image.frombytes("I;16", (shape[1], shape[0]), a.astype("<u2").tobytes()).save(src)
    else:
        Image.fromarray(a, mode=mode).save(src)
    stub = Stub()
    r = P.run(stub, _args(input=str(src), output=str(tmp_path / "o")), 2, torch.device("cpu"))
    assert r["n"] == 1 and r["written"] == [str(tmp_path / "o" / "img_sr.png")] and stub.calls == [1]
    with Image.open(tmp_path / "o" / "img_sr.png") as im:
        assert im.mode == mode                                                # gray in gives gray out, alpha kept, 16-bit kept
        got = np.asarray(im)
    want, _ = _expected(a)
    assert got.dtype == a.dtype and np.array_equal(got.reshape(want.shape), want)
    # the stub is exact, so the colour samples of the file are the nearest-neighbour x2 of the input's
    colour = slice(0, 1) if mode == "LA" else slice(0, 3) if mode == "RGBA" else slice(None)
    assert np.array_equal(got.reshape(want.shape)[..., colour], np.repeat(np.repeat(a.reshape(shape[0], shape[1], -1), 2, 0), 2, 1)[..., colour])
    if mode in ("LA", "RGBA"):          # alpha is kept: the resized plane, not an opaque one
        assert (got[..., -1] != 255).any()
    out = capsys.readouterr().out
    assert f"[predict] img.png 7x5 {mode} {8 * a.dtype.itemsize} -> 14x10 |" in out and "[done] 1 images |" in out


def test_upscale_returns_arrays_and_counts():
    arrays = [_rand((4, 6, 3), np.uint8, 1), _rand((4, 6, 4), np.uint8, 2), _rand((5, 3), np.uint16, 3)]
    r = P.upscale(Stub(), arrays, scale=2, device="cpu", log=lambda s: None)
    assert r["groups"] == [1, 1, 1] and r["clipped"] == 0 and r["pixels"] == 2 * (8 * 12) + 10 * 6
    for a, out in zip(arrays, r["outputs"]):
        want, _ = _expected(a)
        assert out.dtype == a.dtype and np.array_equal(out, want)


def test_grouping_under_batch_size():
    same = [_rand((4, 6, 3), np.uint8, s) for s in range(5)]
    arrays = same[:3] + [_rand((4, 6), np.uint8, 9)] + same[3:] + [_rand((4, 6, 3), np.uint16, 10)]
    for bs, want in ((1, [1] * 7), (2, [2, 1, 1, 2, 1]), (4, [3, 1, 2, 1]), (8, [3, 1, 2, 1])):
        stub = Stub()
        r = P.upscale(stub, arrays, scale=2, device="cpu", batch_size=bs, log=lambda s: None)
        assert stub.calls == want and r["groups"] == want
        for a, out in zip(arrays, r["outputs"]):          # grouped and single calls of the stub give the same samples
            assert np.array_equal(out, _expected(a)[0])


def test_run_groups_files_and_decodes_each_once(tmp_path, monkeypatch):
    d = tmp_path / "in"
    d.mkdir()
    for name, a in (("a.png", _rand((4, 6, 3), np.uint8, 1)), ("b.png", _rand((4, 6, 3), np.uint8, 2)), ("c.png", _rand((4, 6), np.uint8, 3)),
                    ("d.png", _rand((4, 6, 3), np.uint8, 4))):
        Image.fromarray(a).save(d / name)
    loads = []
    real = P.load_image
    monkeypatch.setattr(P, "load_image", lambda p, log=print: (loads.append(p.name), real(p, log))[1])
    stub = Stub()
    r = P.run(stub, _args(input=str(d), output=str(tmp_path / "o"), batch_size=4), 2, torch.device("cpu"))
    assert stub.calls == [2, 1, 1] and r["groups"] == [2, 1, 1] and loads == ["a.png", "b.png", "c.png", "d.png"]
    assert sorted(p.name for p in (tmp_path / "o").iterdir()) == ["a_sr.png", "b_sr.png", "c_sr.png", "d_sr.png"]


@pytest.mark.parametrize("outscale,size", [(None, (14, 10)), (2.0, (14, 10)), (3.0, (21, 15)), (1.5, (11, 8)), (0.05, (1, 1)), (2.5, (18, 13))])
def test_outscale_sizes(outscale, size):
    assert P.out_size(7, 5, 2.0 if outscale is None else outscale) == size
    a = _rand((7, 5, 4), np.uint8, 3)
    stub = Stub()
    r = P.upscale(stub, [a], scale=2, device="cpu", outscale=outscale, log=lambda s: None)
    out = r["outputs"][0]
    assert out.shape == size + (4,) and out.dtype == np.uint8
    if size == (14, 10):          # the resize is skipped: the exact composition
        assert np.array_equal(out, _expected(a)[0])


def test_out_bits_override(tmp_path):
    a = _rand((5, 4), np.uint8, 1)
    r = P.upscale(Stub(), [a], scale=2, device="cpu", out_bits=16, log=lambda s: None)
    assert r["outputs"][0].dtype == np.uint16 and np.array_equal(r["outputs"][0], _expected(a, bits=16)[0])
    a16 = _rand((5, 4), np.uint16, 2)
    r = P.upscale(Stub(), [a16], scale=2, device="cpu", out_bits="8", log=lambda s: None)
    assert r["outputs"][0].dtype == np.uint8 and np.array_equal(r["outputs"][0], _expected(a16, bits=8)[0])
    Image.fromarray(_rand((4, 4, 3), np.uint8, 1)).save(tmp_path / "rgb.png")
    with pytest.raises(ValueError, match="gray files only"):
        P.run(Stub(), _args(input=str(tmp_path / "rgb.png"), output=str(tmp_path / "o"), out_bits="16"), 2, torch.device("cpu"))


def test_gray_model_on_rgb_files():
    """--channels 1: an RGB file goes in as its integer luma and comes out as three equal samples."""
    a = _rand((4, 6, 3), np.uint8, 8)
    r = P.upscale(Stub(), [a], scale=2, device="cpu", channels=1, log=lambda s: None)
    want, _ = _expected(a, channels=1)
    assert np.array_equal(r["outputs"][0], want) and (want[..., 0] == want[..., 2]).all()


def test_tile_and_self_ensemble_lines_and_exactness(capsys):
    a = _rand((12, 10, 3), np.uint8, 4)
    predict = P.make_predict(Stub(), tile=8, tile_overlap=2, tile_batch=2, tile_blend="center", self_ensemble=True)
    out = capsys.readouterr().out
    assert "[tile] 8 overlap 2 batch 2 blend center" in out and "[self_ensemble] x8" in out
    r = P.upscale(predict, [a], scale=2, device="cpu", log=lambda s: None)
    plain = P.upscale(Stub(), [a], scale=2, device="cpu", log=lambda s: None)
    # nearest neighbour commutes with tiling and with the dihedral transforms, and the mean of eight equal k / 255 values rounds back to k
    assert np.array_equal(r["outputs"][0], plain["outputs"][0])


def test_non_finite_guard_fires_and_writes_nothing(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    for name in ("a.png", "b.png"):
        Image.fromarray(_rand((4, 6, 3), np.uint8, 1)).save(d / name)
    Image.fromarray(_rand((4, 6), np.uint8, 1)).save(d / "0_first.png")

    class Bad(Stub):
        def __call__(self, x):
            y = super().__call__(x)
            if x.shape[0] == 2:
                y[1, 0, 0, 0] = float("nan")
                y[0, 1, 2, 2] = float("inf")
            return y

    with pytest.raises(RuntimeError, match=r"non-finite values: count=2 in a\.png, b\.png"):
        P.run(Bad(), _args(input=str(d), output=str(tmp_path / "o"), batch_size=2), 2, torch.device("cpu"))
    assert [p.name for p in (tmp_path / "o").iterdir()] == ["0_first_sr.png"]          # the group before it was complete; nothing of the bad one


def test_clipped_count_is_printed(capsys):
    a = _rand((4, 6, 3), np.uint8, 1)

    def model(x):
        y = Stub()(x)
        y[0, 0, 0, :3] = torch.tensor([1.5, -0.25, 1.0])
        return y

    r = P.upscale(model, [a], scale=2, device="cpu", names=["a.png"])
    assert r["clipped"] == 2 and "[clipped] 2 values outside [0, 1] in a.png" in capsys.readouterr().out
    assert r["outputs"][0][0, :3, 0].tolist() == [255, 0, 255]


def test_predict_line_without_modes_names_the_depth(capsys):
    P.upscale(Stub(), [_rand((4, 6), np.uint16, 1), _rand((4, 6, 2), np.uint8, 2)], scale=2, device="cpu", names=["g16", "la"])
    out = capsys.readouterr().out
    assert "[predict] g16 4x6 I;16 16 -> 8x12 |" in out and "[predict] la 4x6 LA 8 -> 8x12 |" in out


def test_nothing_to_process_is_an_error(tmp_path, capsys):
    (tmp_path / "notes.txt").write_text("not an image")
    for inp in (tmp_path / "notes.txt", tmp_path):
        stub = Stub()
        with pytest.raises(SystemExit, match="no image that PIL can open"):
            P.run(stub, _args(input=str(inp), output=str(tmp_path / "o")), 2, torch.device("cpu"))
        assert stub.calls == [] and not (tmp_path / "o").exists()
        assert "[skip] notes.txt" in capsys.readouterr().out


def test_upscale_argument_errors():
    a = _rand((4, 6, 3), np.uint8, 1)
    for kw in (dict(channels=2), dict(out_bits=12), dict(batch_size=0), dict(outscale=0.0), dict(outscale=float("inf"))):
        with pytest.raises(ValueError):
            P.upscale(Stub(), [a], scale=2, device="cpu", **kw)
    with pytest.raises(ValueError, match="the model returned"):
        P.upscale(lambda x: x[:, :1], [a], scale=2, device="cpu")
