"""tests/fft_loss_ref.py pinned to fp64 autograd of the torch.fft.rfft2 expression (CPU), with negative controls, and the host side of
the frequency-loss plumbing: training.make_loss / loss_name and the --fft_weight / --fft_norm flags of finetune_swinir."""
import argparse
import math

import pytest
import torch

import fft_loss_ref as R

# shapes on which torch's own spectrum is exactly zero at the self-conjugate bins (asserted below): there autograd's sign(0) = 0 is
# the definition, and the pin is meaningful to 1e-12.  Odd x odd shapes have the DC bin only.
PIN_SHAPES = [(1, 1, 4, 4), (2, 3, 12, 20), (1, 3, 9, 15), (1, 1, 7, 64)]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("shape", PIN_SHAPES, ids=["x".join(map(str, s)) for s in PIN_SHAPES])
@pytest.mark.parametrize("norm", R.NORMS)
def test_closed_form_matches_fp64_autograd(shape, norm):
    pred, target = R.random_inputs(shape, seed=0)
    v64, g64, spec = R.fft_loss_autograd(pred, target, norm)
    mask = R.structural_mask(*shape[2:])
    assert float(spec.imag[..., mask].abs().max()) == 0.0          # the premise of the pin
    v, g = R.fft_loss_ref(pred, target, norm)
    assert abs(float(v) - float(v64)) <= 1e-12 * float(v64)
    assert _rel(g, g64) <= 1e-12, (shape, norm)


def test_spectrum_matches_rfft2_and_masks_structural_bins():
    for shape in PIN_SHAPES + [(1, 2, 24, 10), (1, 1, 1, 1), (1, 1, 2, 1), (1, 1, 5, 2)]:
        pred, target = R.random_inputs(shape, seed=3)
        re, im = R.spectrum(pred.double() - target.double())
        want = torch.fft.rfft2(pred.double() - target.double())
        scale = float(want.abs().max())
        assert float((re - want.real).abs().max()) <= 1e-13 * scale
        assert float((im - want.imag).abs().max()) <= 1e-13 * scale
        mask = R.structural_mask(*shape[2:])
        assert float(im[..., mask].abs().max()) == 0.0
        H, W = shape[2:]
        assert int(mask.sum()) == (2 if H % 2 == 0 else 1) * (2 if W % 2 == 0 else 1)


def test_structural_sign_cannot_reach_the_gradient():
    """The fifth control, a non-zero sign of Im D at a self-conjugate bin, is one NO pin on value and gradient can catch: such a bin
    has u y / H and v x / W multiples of 1/2, so its term Re(i g exp(i theta)) = -g sin(theta) vanishes at every pixel.  What holds
    instead, and is asserted: the definition's sign there is 0, and putting 1 there moves the fp64 gradient by no more than the
    rounding of sin(pi) (1e-16 relative).  On the device the twiddles at these bins are exactly 0, +-1 and the bins are masked."""
    for shape in [(2, 3, 12, 20), (1, 3, 9, 15), (1, 1, 7, 64)]:
        pred, target = R.random_inputs(shape, seed=1)
        _, g = R.fft_loss_ref(pred, target)
        _, gf = R.fft_loss_ref(pred, target, flaw="structural_sign")
        assert _rel(gf, g) <= 1e-14
        _, im = R.spectrum(pred.double() - target.double())
        assert float(torch.sign(im)[..., R.structural_mask(*shape[2:])].abs().max()) == 0.0


@pytest.mark.parametrize("flaw", [f for f in R.FLAWS if f != "structural_sign"])
def test_negative_controls_are_caught(flaw):
    """Each mistake moves value or gradient by far more than the 1e-12 of the pin."""
    norm = "ortho" if flaw == "ortho_grad_unscaled" else "backward"
    for shape in [(2, 3, 12, 20), (1, 3, 9, 15)]:
        pred, target = R.random_inputs(shape, seed=1)
        v64, g64, _ = R.fft_loss_autograd(pred, target, norm)
        v, g = R.fft_loss_ref(pred, target, norm)
        assert _rel(g, g64) <= 1e-12 and abs(float(v) - float(v64)) <= 1e-12 * float(v64)
        vf, gf = R.fft_loss_ref(pred, target, norm, flaw=flaw)
        worst = max(_rel(gf, g64), abs(float(vf) - float(v64)) / float(v64))
        assert worst >= 1e-3, (flaw, shape, worst)


def test_impulse_known_answer():
    """d = a delta(0, 0): every bin is a (real), L = |a| / 2, d_x[y, x] = sign(a) / N * H [y == 0] sum_{v < Wh} cos(2 pi v x / W)"""
    for shape, a in (((1, 1, 12, 20), 0.75), ((1, 2, 9, 15), -1.5)):
        B, C, H, W = shape
        Wh = W // 2 + 1
        target = torch.zeros(shape)
        pred = torch.zeros(shape)
        pred[..., 0, 0] = a
        v, g = R.fft_loss_ref(pred, target)
        assert float(v) == pytest.approx(abs(a) / 2, rel=1e-14)
        n = 2 * B * C * H * Wh
        x = torch.arange(W, dtype=torch.float64)
        row = sum(torch.cos(2 * math.pi * vv * x / W) for vv in range(Wh)) * (math.copysign(1.0, a) * H / n)
        want = torch.zeros(shape, dtype=torch.float64)
        want[..., 0, :] = row
        assert float((g - want).abs().max()) <= 1e-14


def test_designed_inputs_keep_every_component_away_from_zero():
    for shape in [(1, 3, 96, 80), (1, 1, 65, 129), (1, 1, 24, 10)]:
        pred, target = R.designed_inputs(shape, seed=0)
        re, im = R.spectrum(pred.double() - target.double())
        free = ~R.structural_mask(*shape[2:])
        assert float(re.abs().min()) >= 0.999 and float(im[..., free].abs().min()) >= 0.999, shape
        assert float(re.abs().max()) <= 2.001 and float(im.abs().max()) <= 2.001


def test_make_loss_host_contract():
    from tpu_superresolution_amd import training as T
    assert T.make_loss() is T.l1_loss_checked
    assert T.make_loss("l1", fft_weight=0.0) is T.l1_loss_checked
    assert T.make_loss("l1", ssim_weight=0.0, fft_weight=0.0, fft_norm="ortho") is T.l1_loss_checked
    fn = T.make_loss("l1", fft_weight=0.05)
    assert callable(fn) and fn is not T.l1_loss_checked and fn.__name__ == "loss[l1+0.05*fft]"
    assert T.make_loss("charbonnier", ssim_weight=0.2, fft_weight=0.1, fft_norm="ortho").__name__ == "loss[charbonnier+0.2*(1-ssim)+0.1*fft]"
    assert T.make_loss("mse").__name__ == "loss[mse]" and T.make_loss("l1", ssim_weight=0.2).__name__ == "loss[l1+0.2*(1-ssim)]"
    assert T.loss_name("l1") == "l1" and T.loss_name("charbonnier", 0.2) == "charbonnier+0.2*(1-ssim)"
    assert T.loss_name("l1", 0.0, 0.05) == "l1+0.05*fft" and T.loss_name("mse", 0.2, fft_weight=0.1) == "mse+0.2*(1-ssim)+0.1*fft"
    for bad in (dict(fft_weight=-0.1), dict(fft_weight=float("nan")), dict(fft_weight=float("inf")), dict(fft_weight=0.1, fft_norm="forward"),
                dict(fft_norm="none")):
        with pytest.raises(ValueError):
            T.make_loss(**bad)
    # refused before any kernel is touched
    with pytest.raises(ValueError, match="target"):
        fn(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16, requires_grad=True))
    with pytest.raises(ValueError, match="512"):
        fn(torch.zeros(1, 1, 513, 16), torch.zeros(1, 1, 513, 16))
    with pytest.raises(ValueError, match="512"):
        fn(torch.zeros(1, 1, 16, 513), torch.zeros(1, 1, 16, 513))
    with pytest.raises(ValueError, match="512"):
        fn(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))


def test_ops_refuses_bad_arguments_on_the_host():
    from tpu_superresolution_amd import ops
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError, match="norm"):
        ops.fft_loss_fwd_bwd(x, x, norm="forward")
    with pytest.raises(ValueError, match="fp32"):
        ops.fft_loss_fwd_bwd(x.double(), x.double())
    with pytest.raises(ValueError, match="fp32"):
        ops.fft_loss_fwd_bwd(x[0], x[0])
    with pytest.raises(ValueError, match="accumulate"):
        ops.fft_loss_fwd_bwd(x, x, accumulate=True)


def test_finetune_flags():
    from tpu_superresolution_amd.finetune_swinir import parse_args, saved_args
    base = ["--data_root", "d", "--scale", "X4"]
    a = parse_args(base)
    assert (a.fft_weight, a.fft_norm) == (0.0, "backward")
    kept = saved_args(a)
    assert "fft_weight" not in kept and "fft_norm" not in kept
    a = parse_args(base + ["--fft_weight", "0.05"])
    kept = saved_args(a)
    assert kept["fft_weight"] == 0.05 and "fft_norm" not in kept
    a = parse_args(base + ["--fft_weight", "0.1", "--fft_norm", "ortho", "--loss", "charbonnier", "--ssim_weight", "0.2"])
    kept = saved_args(a)
    assert (kept["fft_weight"], kept["fft_norm"], kept["ssim_weight"], kept["loss"]) == (0.1, "ortho", 0.2, "charbonnier")
    assert "fft_norm" not in saved_args(parse_args(base + ["--fft_norm", "ortho"]))          # without the term the norm does nothing
    assert parse_args(base + ["--fft_weight", "0.05", "--lr_patch", "128"]).lr_patch == 128          # 128 * 4 = 512
    assert parse_args(base + ["--lr_patch", "129"]).lr_patch == 129                                  # no term: any patch
    for extra in (["--arch", "hat"], ["--arch", "dat"], ["--arch", "hat", "--graph"]):
        assert parse_args(base + ["--fft_weight", "0.05"] + extra).fft_weight == 0.05
    dn = ["--data_root", "d", "--scale", "X1", "--task", "dn", "--dn_sigma", "25", "25", "--channels", "1", "--fft_weight", "0.05"]
    assert parse_args(dn + ["--lr_patch", "512"]).fft_weight == 0.05          # scale 1: the patch itself
    with pytest.raises(SystemExit):
        parse_args(dn + ["--lr_patch", "513"])
    for bad in (["--fft_weight", "-0.1"], ["--fft_weight", "nan"], ["--fft_weight", "inf"], ["--fft_weight", "0.05", "--fft_norm", "forward"],
                ["--fft_weight", "0.05", "--lr_patch", "129"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    with pytest.raises(SystemExit):
        parse_args(["--data_root", "d", "--scale", "X2", "--fft_weight", "0.05", "--lr_patch", "257"])
    assert isinstance(a, argparse.Namespace)
