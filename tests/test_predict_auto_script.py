"""predict --arch auto / --scale X3 | X8 | auto / --img_range without a GPU: what the parser takes and refuses, the scale mismatch message,
and the `[arch]` lines of build_auto_model (the model of checkpoint_arch.build_from_state is constructed on the CPU; nothing runs it)."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tpu_superresolution_amd import SwinIR
from tpu_superresolution_amd import predict as P
from tpu_superresolution_amd._lib import SrkUnsupported

IO = ["--input", "in", "--output", "out", "--ckpt", "w.pt"]
AUTO = IO + ["--arch", "auto", "--scale", "auto"]


def _tiny(**kw):
    d = dict(img_size=16, in_chans=3, embed_dim=24, depths=[2, 2], num_heads=[2, 2], window_size=8, mlp_ratio=2, upscale=4, img_range=1.0,
             upsampler="pixelshuffledirect", resi_connection="1conv")
    d.update(kw)
    return d


def _ckpt(tmp_path, kw, envelope="params_ema"):
    path = tmp_path / "w.pt"
    torch.save({envelope: SwinIR(drop_path_rate=0.0, **kw).state_dict()}, path)
    return str(path)


# ---- parser -----------------------------------------------------------------------------------------------------------------------------------
def test_parser_accepts_auto_and_the_new_scales():
    a = P.parse_args(AUTO)
    assert (a.arch, a.scale, a.img_range, a.window_size, a.task, a.channels, a.upsampler) == ("auto", "auto", None, 8, "sr", 3, "pixelshuffle")
    assert P.parse_args(AUTO + ["--img_range", "255"]).img_range == 255.0
    for s in ("X1", "X2", "X3", "X4", "X8"):          # an explicit scale with --arch auto is checked against the file later
        assert P.parse_args(IO + ["--arch", "auto", "--scale", s]).scale == s
    for arch in ("swinir", "hat", "dat"):
        assert P.parse_args(IO + ["--arch", arch, "--scale", "X3"]).scale == "X3"
    assert P.parse_args(IO + ["--arch", "swinir", "--scale", "X8"]).scale == "X8"
    assert P.PREDICT_SCALES == {"X1": 1, "X2": 2, "X3": 3, "X4": 4, "X8": 8}
    from tpu_superresolution_amd.data_cli import SCALES
    assert SCALES == {"X1": 1, "X2": 2, "X4": 4}          # the training parsers' table stays as it is


@pytest.mark.parametrize("argv", [
    AUTO + ["--window_size", "7"], AUTO + ["--window_size", "8"], AUTO + ["--task", "dn"], AUTO + ["--task", "car"], AUTO + ["--channels", "1"],
    AUTO + ["--upsampler", "nearest+conv"], AUTO + ["--img_range", "0"], AUTO + ["--img_range", "nan"], AUTO + ["--img_range", "-1"],
    AUTO + ["--tile_blend", "feather"],
    IO + ["--arch", "swinir", "--scale", "auto"], IO + ["--arch", "hat", "--scale", "auto"], IO + ["--arch", "dat", "--scale", "auto"],
    IO + ["--arch", "hat", "--scale", "X8"], IO + ["--arch", "dat", "--scale", "X8"], IO + ["--arch", "swinir", "--scale", "X2", "--img_range", "255"],
    IO + ["--arch", "swinir", "--scale", "X3", "--upsampler", "nearest+conv"], IO + ["--arch", "swinir", "--scale", "X8", "--upsampler", "nearest+conv"],
    IO + ["--arch", "swinir", "--scale", "X3", "--task", "dn"], IO + ["--arch", "swinir", "--scale", "X5"], IO + ["--arch", "auto", "--scale", "x3"],
    IO + ["--arch", "guess", "--scale", "auto"], IO + ["--arch", "auto"], IO + ["--scale", "auto"]],
    ids=lambda argv: " ".join(argv[6:]))
def test_parser_refusals(argv):
    with pytest.raises(SystemExit):
        P.parse_args(argv)


def test_refusal_messages_name_the_flags(capsys):
    with pytest.raises(SystemExit):
        P.parse_args(AUTO + ["--window_size", "7", "--channels", "1"])
    err = capsys.readouterr().err
    assert "--window_size 7, --channels 1: with --arch auto the checkpoint decides" in err
    with pytest.raises(SystemExit):
        P.parse_args(IO + ["--arch", "hat", "--scale", "auto"])
    assert "--scale auto goes with --arch auto" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        P.parse_args(IO + ["--arch", "dat", "--scale", "X8"])
    assert "--scale X8 is an option of --arch swinir and --arch auto" in capsys.readouterr().err


def test_arch_auto_on_cpu_exits(tmp_path):
    with pytest.raises(SystemExit, match="HIP path only"):
        P.main(["--input", str(tmp_path), "--output", str(tmp_path / "o"), "--arch", "auto", "--scale", "auto", "--ckpt", "none.pt", "--device", "cpu"])
    assert not (tmp_path / "o").exists()


# ---- build_auto_model ---------------------------------------------------------------------------------------------------------------------
def test_arch_lines_and_the_file_decides(tmp_path):
    ckpt = _ckpt(tmp_path, _tiny(in_chans=1, upscale=1, upsampler="", window_size=7, img_size=21, img_range=255.0))
    args = P.parse_args(["--input", "in", "--output", "out", "--ckpt", ckpt, "--arch", "auto", "--scale", "auto"])
    lines = []
    model, scale = P.build_auto_model(args, log=lines.append)
    assert scale == 1 and args.channels == 1 and isinstance(model, SwinIR) and model.img_range == 255.0 and model.window_size == 7
    assert lines[0] == "[ckpt] loaded state_dict from 'params_ema' key"
    assert lines[1] == ("[arch] swinir: SwinIR(img_size=21, in_chans=1, embed_dim=24, depths=[2, 2], num_heads=[2, 2], window_size=7, mlp_ratio=2, "
                        "ape=False, upscale=1, img_range=255.0, upsampler='', resi_connection='1conv')")
    assert lines[2:] == ["[arch] note: img_range=255: convention for the scale-1 head at window 7 (the published JPEG-artifact files); not in a state_dict"]
    # --img_range overrides the convention, and says so
    args = P.parse_args(["--input", "in", "--output", "out", "--ckpt", ckpt, "--arch", "auto", "--scale", "X1", "--img_range", "1"])
    lines = []
    model, _ = P.build_auto_model(args, log=lines.append)
    assert model.img_range == 1.0 and "img_range=1.0, " in lines[1] and lines[2:] == ["[arch] note: img_range=1.0: given by the caller"]


def test_scale_mismatch_names_both(tmp_path):
    ckpt = _ckpt(tmp_path, _tiny(upscale=4), envelope="params")
    args = P.parse_args(["--input", "in", "--output", "out", "--ckpt", ckpt, "--arch", "auto", "--scale", "X2"])
    with pytest.raises(SystemExit, match=r"--scale X2 does not match the checkpoint: .*w\.pt is a x4 model \(name --scale X4 or --scale auto\)"):
        P.build_auto_model(args, log=lambda s: None)
    args = P.parse_args(["--input", "in", "--output", "out", "--ckpt", ckpt, "--arch", "auto", "--scale", "X4"])
    model, scale = P.build_auto_model(args, log=lambda s: None)
    assert scale == 4 and model.upscale == 4 and model.upsampler == "pixelshuffledirect" and args.channels == 3


def test_an_uncovered_file_raises_before_any_output(tmp_path, monkeypatch):
    from tpu_superresolution_amd import DAT
    sd = DAT(img_size=32, in_chans=3, embed_dim=32, split_size=[8, 16], depth=[2], num_heads=[2], expansion_factor=2, upscale=2, resi_connection="3conv",
             upsampler="pixelshuffledirect", drop_path_rate=0.0).state_dict()
    torch.save({"params": sd}, tmp_path / "light.pt")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "a.png")
    monkeypatch.setattr(P.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.torch.cuda, "get_device_name", lambda i: "stub")
    ran = []
    monkeypatch.setattr(P, "run", lambda *a, **k: ran.append(1))
    with pytest.raises(SrkUnsupported, match="resi_connection='3conv'"):
        P.main(["--input", str(tmp_path / "a.png"), "--output", str(tmp_path / "o"), "--arch", "auto", "--scale", "auto", "--ckpt", str(tmp_path / "light.pt"),
                "--device", "cuda"])
    assert not ran and not (tmp_path / "o").exists()


def test_run_takes_the_hand_made_namespace_and_a_scale_3_stub(tmp_path):
    """run() needs no attribute that --arch auto added: the namespace of tests/test_predict_script.py drives it at x3."""
    Image.fromarray(np.arange(48, dtype=np.uint8).reshape(4, 4, 3)).save(tmp_path / "a.png")
    ns = types.SimpleNamespace(input=str(tmp_path / "a.png"), output=str(tmp_path / "o"), suffix="_sr", tile=0, tile_overlap=32, tile_batch=1,
                               tile_blend="mean", self_ensemble=False, batch_size=1, outscale=None, out_bits="auto", channels=3)
    r = P.run(lambda x: x.repeat_interleave(3, 2).repeat_interleave(3, 3), ns, 3, torch.device("cpu"))
    assert r["n"] == 1
    with Image.open(tmp_path / "o" / "a_sr.png") as im:
        assert im.size == (12, 12)
