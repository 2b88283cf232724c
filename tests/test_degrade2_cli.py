"""The command lines of --degrade second_order: what the parsers accept, what they refuse, and that no new flag reaches a checkpoint's
saved arguments at its default.  No GPU."""
import pytest

TRAIN = ["--data_root", "D", "--scale", "X2"]
ON = TRAIN + ["--gpu_data", "--synth_lr", "--degrade", "second_order"]


def test_finetune_accepts_and_maps_the_flags():
    from tpu_superresolution_amd import finetune_swinir as F
    a = F.parse_args(ON + ["--arch", "hat", "--graph", "--ema_decay", "0.999", "--augment", "d4", "--loss", "mse", "--val_tile", "64",
                           "--blur_kernel", "mixed", "--blur_ksize", "7", "15", "--jpeg_quality", "40", "90", "--jpeg2_quality", "50", "70",
                           "--jpeg_subsample", "420", "--noise2_sigma", "2", "20", "--blur2_sigma", "0.3", "1.0", "--blur2_p", "0.5",
                           "--resize_range", "0.5", "1.25", "--resize_prob", "0.1", "0.8", "0.1", "--resize2_range", "0.4", "1.1",
                           "--resize2_prob", "0.2", "0.2", "0.6", "--sinc_p", "0.2", "--final_sinc_p", "0.6", "--degrade_margin", "4",
                           "--degrade_seed", "9", "--gray_noise_p", "0.3"])
    s = F.second_order_spec(a)
    assert s.jpeg_quality == (40, 90) and s.jpeg2_quality == (50, 70) and s.ksize == (7, 15) and s.seed == 9 and s.gray_noise_p == 0.3
    assert s.noise2_sigma == (2 / 255.0, 20 / 255.0) and s.blur2_sigma == (0.3, 1.0) and s.blur2_p == 0.5 and s.sinc_p == 0.2 and s.final_sinc_p == 0.6
    assert s.resize_range == (0.5, 1.25) and s.resize_prob == (0.1, 0.8, 0.1) and s.resize2_range == (0.4, 1.1) and s.resize2_prob == (0.2, 0.2, 0.6)
    assert F.jpeg_spec(a) is None and F.degrade_spec(a) is not None and F.psf_spec(a).mode == "mixed"
    for arch in (["--arch", "dat"], ["--arch", "swinir"], ["--arch", "swinir", "--window_size", "4", "--graph"]):
        assert F.second_order_spec(F.parse_args(ON + arch)) == __import__("tpu_superresolution_amd.sr_datasets", fromlist=["x"]).SecondOrderSpec()


def test_saved_args_keep_no_new_flag_at_its_default():
    from tpu_superresolution_amd import finetune_swinir as F
    plain = F.saved_args(F.parse_args(TRAIN))
    assert not [k for k in F.SECOND_ORDER_FLAGS if k in plain] and "degrade" not in plain
    on = F.saved_args(F.parse_args(ON + ["--sinc_p", "0.2"]))
    assert on["degrade"] == "second_order" and on["sinc_p"] == 0.2 and [k for k in F.SECOND_ORDER_FLAGS if k in on] == ["sinc_p"]
    assert F.second_order_spec(F.parse_args(TRAIN)) is None and F.second_order_spec(F.parse_args(TRAIN + ["--gpu_data", "--synth_lr", "--degrade", "blind"])) is None


@pytest.mark.parametrize("bad", [
    TRAIN + ["--degrade", "second_order"],                                          # no --synth_lr
    TRAIN + ["--synth_lr", "--degrade", "second_order"],                            # no --gpu_data
    ON + ["--synth_lr_bits", "0"],
    ON + ["--jpeg_quality", "30", "90", "--jpeg_p", "0.5"],
    ON + ["--jpeg_quality", "0", "90"],
    ON + ["--jpeg2_quality", "90", "30"],
    ON + ["--resize_range", "0.05", "1.5"],
    ON + ["--resize_range", "0.5", "0.9"],
    ON + ["--resize_prob", "0.5", "0.6", "0.1"],
    ON + ["--resize2_range", "0.3", "3"],
    ON + ["--sinc_p", "1.5"],
    ON + ["--final_sinc_p", "-0.1"],
    ON + ["--blur2_p", "2"],
    ON + ["--blur2_sigma", "0", "1"],
    ON + ["--noise2_sigma", "20", "2"],
    ON + ["--degrade_margin", "-1"],
    ON + ["--degrade_margin", "65"],
    ON + ["--blur_sigma", "0.2", "3.0"],
    ON + ["--blur_psf", "F.npy", "--blur_kernel", "mixed"],
    ON + ["--task", "dn", "--scale", "X1", "--dn_sigma", "25", "25"],
] + [TRAIN + ["--gpu_data", "--synth_lr", "--degrade", d] + f for d in ("bicubic", "blind") for f in (
    ["--sinc_p", "0.2"], ["--final_sinc_p", "0.5"], ["--blur2_p", "0.5"], ["--blur2_sigma", "0.2", "1"], ["--noise2_sigma", "1", "2"],
    ["--jpeg2_quality", "30", "90"], ["--resize_range", "0.5", "1.5"], ["--resize_prob", "0.2", "0.7", "0.1"], ["--resize2_range", "0.5", "1.2"],
    ["--resize2_prob", "0.3", "0.4", "0.3"], ["--degrade_margin", "8"])])
def test_finetune_refuses(bad, capsys):
    from tpu_superresolution_amd import finetune_swinir as F
    with pytest.raises(SystemExit) as e:
        F.parse_args(bad)
    assert e.value.code == 2 and "error:" in capsys.readouterr().err


def test_evaluate_parser():
    from tpu_superresolution_amd import evaluate as E
    base = ["--scale", "X2", "--ckpt", "F", "--arch", "swinir", "--synth_lr"]
    a = E.parse_args(base + ["--degrade", "second_order", "--tile", "64", "--self_ensemble", "--bench_metric", "y", "--jpeg_subsample", "420",
                             "--jpeg_quality", "50", "--blur_theta", "30"])
    assert a.degrade == "second_order" and a.jpeg_quality == 50
    for bad in (base + ["--degrade", "second_order", "--synth_lr_bits", "0"], ["--scale", "X2", "--ckpt", "F", "--arch", "swinir", "--degrade", "second_order"],
                base + ["--degrade", "second_order", "--blur_sigma", "3", "3"], base + ["--jpeg_subsample", "420"],
                base + ["--degrade", "second_order", "--arch", "ms_resunet"]):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
