"""The host side of the scale-1 restoration tasks (CPU only): RestoreSpec, the new flag combinations of finetune_swinir / evaluate,
build_restoration_model, and the saved `args` at the defaults."""
import random

import pytest
import torch

from tpu_superresolution_amd import evaluate as E
from tpu_superresolution_amd import finetune_swinir as T
from tpu_superresolution_amd.sr_datasets import DegradeSpec, FixedRestore, JpegSpec, RestoreSpec

BASE = ["--data_root", "d"]
EBASE = ["--ckpt", "c.pt", "--arch", "swinir"]


def test_restore_spec_ranges_and_fixed():
    s = RestoreSpec(sigma=(15 / 255, 50 / 255), jpeg_quality=(10, 40), gray_noise_p=0.25, subsample=True, seed=3)
    assert s.fixed() == FixedRestore(32.5 / 255, 25, False, True)
    assert RestoreSpec(sigma=(0.1, 0.1)).fixed() == FixedRestore(0.1, 0, False, False)
    assert RestoreSpec(jpeg_quality=(10, 13)).fixed().jpeg_quality == round(11.5) and RestoreSpec(gray_noise_p=0.5).fixed().gray_noise
    rng = s.rng()
    seen_q, seen_gray = set(), set()
    for _ in range(400):
        sigma, q, nid, gray = s.draw(rng, colour=True)
        assert 15 / 255 <= sigma <= 50 / 255 and 10 <= q <= 40 and isinstance(q, int) and 0 <= nid < 1 << 64
        seen_q.add(q)
        seen_gray.add(gray)
    assert seen_q == set(range(10, 41)) and seen_gray == {False, True}
    assert all(s.draw(rng, colour=False)[3] for _ in range(20))          # a one-channel image always gets gray noise
    assert all(RestoreSpec(sigma=(0.1, 0.2)).draw(rng, True)[1] == 0 for _ in range(5))          # no JPEG stage: quality 0
    for bad in (dict(sigma=(0.2, 0.1)), dict(sigma=(0.0, 1.5)), dict(sigma=(float("nan"), 0.1)), dict(sigma=0.1), dict(jpeg_quality=(0, 10)),
                dict(jpeg_quality=(50, 40)), dict(jpeg_quality=(10, 101)), dict(jpeg_quality=(10.5, 20)), dict(jpeg_quality=30),
                dict(gray_noise_p=1.5), dict(gray_noise_p=float("nan"))):
        with pytest.raises(ValueError):
            RestoreSpec(**bad)


def test_restore_spec_generator_is_its_own_and_takes_four_variates():
    s = RestoreSpec(sigma=(0.0, 0.2), jpeg_quality=(10, 40), gray_noise_p=0.5, seed=5)
    random.seed(123)
    state = random.getstate()
    a = [s.draw(s.rng(1), True) for _ in range(3)]
    assert random.getstate() == state          # the global generator places the crops and is not touched
    assert a[0] == a[1] == a[2] and s.draw(s.rng(1), True) != s.draw(s.rng(2), True)
    # not the stream of a DegradeSpec or a JpegSpec with the same seed
    r = s.rng(0)
    first = [r.random() for _ in range(4)]
    assert first != [DegradeSpec(seed=5).rng(0).random() for _ in range(4)] and first != [JpegSpec(seed=5).rng(0).random() for _ in range(4)]
    assert first == [random.Random("restore:5").random() for _ in range(1)] + first[1:]
    # a fixed number of variates per draw, whatever they decide: after n draws every spec has the generator in the same state
    states = []
    for spec in (s, RestoreSpec(sigma=(0.1, 0.1), seed=5), RestoreSpec(jpeg_quality=(5, 5), gray_noise_p=1.0, seed=5)):
        g = spec.rng()
        for colour in (True, False, True):
            spec.draw(g, colour)
        states.append(g.getstate())
    ref = random.Random("restore:5")
    for _ in range(3):
        ref.uniform(0, 1), ref.random(), ref.random(), ref.getrandbits(64)
    assert states[0] == states[1] == states[2] == ref.getstate()


def test_finetune_flag_combinations(capsys):
    a = T.parse_args(BASE + ["--scale", "X1", "--task", "dn", "--dn_sigma", "15", "50"])
    assert (a.task, a.channels, a.window_size, a.gpu_data, a.dn_bits) == ("dn", 3, 8, True, 0)
    spec = T.restore_spec(a)
    assert spec.sigma == (15 / 255, 50 / 255) and spec.jpeg_quality is None and spec.seed == 0
    a = T.parse_args(BASE + ["--scale", "X1", "--task", "car", "--jpeg_quality", "10", "40", "--channels", "1", "--jpeg_subsample", "420",
                             "--degrade_seed", "7", "--dn_bits", "8"])
    assert (a.task, a.channels, a.window_size, a.gpu_data, a.dn_bits) == ("car", 1, 7, True, 8)
    spec = T.restore_spec(a)
    assert spec.sigma == (0.0, 0.0) and spec.jpeg_quality == (10, 40) and spec.subsample and spec.seed == 7
    assert T.parse_args(BASE + ["--scale", "X1", "--task", "car", "--jpeg_quality", "10", "40", "--window_size", "8"]).window_size == 8
    assert T.parse_args(BASE + ["--scale", "X1", "--task", "dn", "--dn_sigma", "25", "25", "--window_size", "4"]).window_size == 4
    assert T.restore_spec(T.parse_args(BASE + ["--scale", "X2"])) is None
    dn, car = ["--task", "dn", "--dn_sigma", "25", "25"], ["--task", "car", "--jpeg_quality", "10", "40"]
    for bad, word in ((["--scale", "X1"], "X1"), (["--scale", "X2"] + dn, "X1"), (["--scale", "X4"] + car, "X1"),
                      (["--scale", "X1", "--task", "dn"], "--dn_sigma"), (["--scale", "X1", "--task", "car"], "--jpeg_quality"),
                      (["--scale", "X1"] + dn + ["--jpeg_quality", "10", "40"], "car"),
                      (["--scale", "X1"] + dn + ["--arch", "hat"], "swinir"), (["--scale", "X1"] + car + ["--arch", "dat"], "swinir"),
                      (["--scale", "X1"] + dn + ["--synth_lr", "--gpu_data"], "--synth_lr"), (["--scale", "X1"] + car + ["--jpeg_p", "0.5"], "--jpeg_p"),
                      (["--scale", "X1"] + dn + ["--channels", "1", "--val_bench_metric", "y"], "--channels 1"),
                      (["--scale", "X1", "--task", "dn", "--dn_sigma", "50", "25"], "sigma"),
                      (["--scale", "X1", "--task", "dn", "--dn_sigma", "25", "300"], "sigma"),
                      (["--scale", "X1", "--task", "car", "--jpeg_quality", "0", "40"], "quality"),
                      (["--scale", "X2", "--channels", "1"], "--task dn | car"), (["--scale", "X2", "--dn_sigma", "25", "25"], "--task dn | car"),
                      (["--scale", "X4", "--dn_bits", "8"], "--task dn | car"), (["--scale", "X1"] + dn + ["--channels", "2"], "--channels"),
                      (["--scale", "X1", "--task", "deblur"], "--task"), (["--scale", "X3"], "--scale")):
        with pytest.raises(SystemExit):
            T.parse_args(BASE + bad)
        assert word in capsys.readouterr().err, bad


def test_evaluate_flag_combinations(capsys):
    a = E.parse_args(EBASE + ["--scale", "X1", "--task", "dn", "--dn_sigma", "25"])
    assert (a.task, a.channels, a.window_size) == ("dn", 3, 8) and E.eval_restore(a) == FixedRestore(25 / 255, 0, False, False)
    a = E.parse_args(EBASE + ["--scale", "X1", "--task", "car", "--jpeg_quality", "10", "--jpeg_subsample", "420", "--channels", "1"])
    assert (a.task, a.channels, a.window_size) == ("car", 1, 7) and E.eval_restore(a) == FixedRestore(0.0, 10, False, True)
    assert E.parse_args(EBASE + ["--scale", "X1", "--task", "car", "--jpeg_quality", "10", "--window_size", "8"]).window_size == 8
    assert E.parse_args(EBASE + ["--scale", "X2"]).window_size == 8 and E.eval_restore(E.parse_args(EBASE + ["--scale", "X2"])) is None
    dn, car = ["--task", "dn", "--dn_sigma", "25"], ["--task", "car", "--jpeg_quality", "10"]
    for bad, word in ((["--scale", "X1"], "X1"), (["--scale", "X2"] + dn, "X1"), (["--scale", "X4"] + car, "X1"),
                      (["--scale", "X1", "--task", "dn"], "--dn_sigma"), (["--scale", "X1", "--task", "car"], "--jpeg_quality"),
                      (["--scale", "X1"] + dn + ["--jpeg_quality", "10"], "car"), (["--scale", "X1"] + dn + ["--arch", "hat"], "swinir"),
                      (["--scale", "X1"] + car + ["--arch", "ms_resunet"], "swinir"), (["--scale", "X1"] + dn + ["--synth_lr"], "--synth_lr"),
                      (["--scale", "X1"] + dn + ["--channels", "1", "--bench_metric", "y"], "--channels 1"),
                      (["--scale", "X1", "--task", "dn", "--dn_sigma", "300"], "sigma"), (["--scale", "X1", "--task", "car", "--jpeg_quality", "101"], "quality"),
                      (["--scale", "X2", "--channels", "1"], "--task dn | car"), (["--scale", "X2", "--dn_sigma", "25"], "--task dn | car")):
        with pytest.raises(SystemExit):
            E.parse_args(["--ckpt", "c.pt"] + (bad if "--arch" in bad else ["--arch", "swinir"] + bad))
        assert word in capsys.readouterr().err, bad


@pytest.mark.parametrize("task,channels", [("dn", 3), ("dn", 1), ("car", 3), ("car", 1)])
def test_build_restoration_model(task, channels):
    m = T.build_restoration_model(task, channels, 0.0)
    sd = m.state_dict()
    ws, size, rng = {"dn": (8, 128, 1.0), "car": (7, 126, 255.0)}[task]
    assert (m.upscale, m.upsampler, m.window_size, m.img_range, m.in_chans, m.embed_dim) == (1, "", ws, rng, channels, 180)
    assert sd["conv_first.weight"].shape == (180, channels, 3, 3) and sd["conv_last.weight"].shape == (channels, 180, 3, 3)
    assert sd["conv_last.bias"].shape == (channels,)
    assert not [k for k in sd if k.startswith(("upsample", "conv_before_upsample", "conv_up", "conv_hr"))]
    assert len([k for k in sd if k.endswith("attn.relative_position_bias_table")]) == 36          # six groups of six blocks
    assert sd["layers.0.residual_group.blocks.0.attn.relative_position_bias_table"].shape == ((2 * ws - 1) ** 2, 6)
    assert sd["layers.0.residual_group.blocks.1.attn_mask"].shape == ((size // ws) ** 2, ws * ws, ws * ws)
    assert sd["layers.0.residual_group.blocks.0.mlp.fc1.weight"].shape == (360, 180) and sd["layers.5.conv.weight"].shape == (180, 180, 3, 3)
    # a window given explicitly rounds img_size down to its multiple
    m4 = T.build_restoration_model(task, channels, 0.0, 4)
    assert m4.window_size == 4 and m4.state_dict()["layers.0.residual_group.blocks.1.attn_mask"].shape[0] == (size // 4) ** 2
    # strict loading of a state dict with the same keys and shapes, as the authors' checkpoints are
    T.build_restoration_model(task, channels, 0.1).load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)
    for bad in (dict(task="sr"), dict(channels=2), dict(window_size=9)):
        with pytest.raises(ValueError):
            T.build_restoration_model(**{"task": task, "channels": channels, **bad})


def test_saved_args_are_unchanged_at_the_defaults():
    a = T.parse_args(BASE + ["--scale", "X4"])
    saved = T.saved_args(a)
    assert not {"task", "channels", "dn_sigma", "dn_bits"} & set(saved)
    assert saved["window_size"] == 8 and saved["scale"] == "X4" and saved["gpu_data"] is False
    a = T.parse_args(BASE + ["--scale", "X1", "--task", "car", "--jpeg_quality", "10", "40", "--channels", "1", "--dn_sigma", "0", "5", "--dn_bits", "8"])
    saved = T.saved_args(a)
    assert (saved["task"], saved["channels"], saved["dn_sigma"], saved["dn_bits"], saved["window_size"]) == ("car", 1, [0.0, 5.0], 8, 7)
    assert saved["jpeg_quality"] == [10, 40]
