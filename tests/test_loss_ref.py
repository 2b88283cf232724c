"""tests/loss_ref.py pinned to torch (CPU, fp64), with negative controls, and the host side of the objective plumbing: training.make_loss
and the --loss / --charbonnier_eps / --ssim_weight flags of finetune_swinir."""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_ref as R


@pytest.mark.parametrize("kind", R.KINDS)
def test_pixel_losses_match_torch(kind):
    g = torch.Generator().manual_seed(1)
    pred = torch.rand(2, 3, 9, 7, generator=g, dtype=torch.float64)
    target = torch.rand(2, 3, 9, 7, generator=g, dtype=torch.float64)
    pred.view(-1)[5] = target.view(-1)[5]                      # d == 0: sign(0) = 0, Charbonnier's gradient 0
    leaf = pred.clone().requires_grad_(True)
    eps = 1e-3
    want = {"l1": lambda: F.l1_loss(leaf, target), "mse": lambda: F.mse_loss(leaf, target),
            "charbonnier": lambda: torch.sqrt((leaf - target) ** 2 + eps ** 2).mean()}[kind]()
    (gw,) = torch.autograd.grad(want, leaf)
    loss, grad = R.pixel_loss_ref(pred, target, kind, eps)
    assert abs(float(loss) - float(want.detach())) <= 1e-15
    assert float((grad - gw).abs().max()) <= 1e-15 * max(1.0, float(gw.abs().max()))
    assert R.pixel_terms_abs_sum(pred, target, kind, eps) == pytest.approx(float(want.detach()) * pred.numel(), rel=1e-12)


CASES = [(k, s) for k in R.SSIM_INPUTS for s in R.SSIM_SHAPES]


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in CASES])
def test_ssim_closed_form_matches_fp64_autograd(kind, shape):
    x, y = R.ssim_inputs(kind, shape)
    for data_range in (1.0, 255.0):
        s = data_range
        v64, g64 = R.ssim_autograd(x * s, y * s, data_range)
        v, g = R.ssim_value_grad_ref(x * s, y * s, data_range)
        assert abs(float(v) - float(v64)) <= 1e-14
        assert float((g - g64).abs().max()) <= 1e-12 * float(g64.abs().max()) + 1e-300, (kind, shape, data_range)


def test_ssim_negative_controls_are_caught():
    """A restatement whose a, b, c are not zero outside the valid domain, and one whose N misses the channel count, must differ from
    autograd by far more than the pin above allows."""
    for kind in R.SSIM_INPUTS:
        shape = (2, 3, 12, 45)
        x, y = R.ssim_inputs(kind, shape)
        v64, g64 = R.ssim_autograd(x, y, 1.0)
        ok = float((R.ssim_value_grad_ref(x, y, 1.0)[1] - g64).abs().max())
        halo = float((R.ssim_value_grad_ref(x, y, 1.0, wrong_halo=True)[1] - g64).abs().max())
        count = float((R.ssim_value_grad_ref(x, y, 1.0, wrong_count=True)[1] - g64).abs().max())
        scale = float(g64.abs().max())
        assert ok <= 1e-12 * scale
        assert halo >= 1e-2 * scale, (kind, halo, scale)
        assert count >= 0.5 * scale, (kind, count, scale)          # 3 channels: every entry is 3x too large


def test_ssim_inputs_are_the_documented_ones():
    p, t = R.ssim_inputs("flat", (1, 1, 11, 12))
    assert set(t.unique().tolist()) == {0.5, 0.8999999761581421} and float((p - t).abs().max()) < 0.01
    p, t = R.ssim_inputs("smooth", (2, 1, 12, 13))
    assert p.shape == t.shape == (2, 1, 12, 13) and 0.0 < float(t.min()) and float(t.max()) < 1.0
    a, b = R.ssim_inputs("random", (1, 1, 11, 11))
    a2, _ = R.ssim_inputs("random", (1, 1, 11, 11))
    assert torch.equal(a, a2) and not torch.equal(a, b)


def test_make_loss_host_contract():
    from tpu_superresolution_amd import training as T
    assert T.make_loss() is T.l1_loss_checked
    assert T.make_loss("l1", ssim_weight=0.0) is T.l1_loss_checked
    for kind in ("mse", "charbonnier"):
        assert callable(T.make_loss(kind)) and T.make_loss(kind) is not T.l1_loss_checked
    assert T.make_loss("l1", ssim_weight=0.2) is not T.l1_loss_checked
    assert T.loss_name("l1") == "l1" and T.loss_name("charbonnier", 0.2) == "charbonnier+0.2*(1-ssim)"
    for bad in (dict(kind="huber"), dict(kind="charbonnier", charbonnier_eps=0.0), dict(kind="charbonnier", charbonnier_eps=float("nan")),
                dict(ssim_weight=-0.1), dict(ssim_weight=float("nan")), dict(ssim_weight=float("inf")), dict(ssim_weight=0.1, data_range=0.0)):
        with pytest.raises(ValueError):
            T.make_loss(**bad)
    # refused before any kernel is touched: a target that wants a gradient, a batch the SSIM window does not fit
    fn = T.make_loss("charbonnier", ssim_weight=0.2)
    with pytest.raises(ValueError, match="target"):
        fn(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16, requires_grad=True))
    with pytest.raises(ValueError, match="11"):
        fn(torch.zeros(1, 3, 10, 16), torch.zeros(1, 3, 10, 16))
    import inspect
    assert inspect.signature(T.train_step).parameters["loss_fn"].default is None
    assert inspect.signature(T.GraphedTrainStep.__init__).parameters["loss_fn"].default is None


def test_finetune_flags():
    from tpu_superresolution_amd.finetune_swinir import parse_args
    base = ["--data_root", "d", "--scale", "X4"]
    a = parse_args(base)
    assert (a.loss, a.charbonnier_eps, a.ssim_weight) == ("l1", 1e-3, 0.0)
    a = parse_args(base + ["--loss", "charbonnier", "--charbonnier_eps", "1e-6", "--ssim_weight", "0.2"])
    assert (a.loss, a.charbonnier_eps, a.ssim_weight) == ("charbonnier", 1e-6, 0.2)
    assert parse_args(base + ["--loss", "mse"]).loss == "mse"
    assert parse_args(base + ["--ssim_weight", "0.5", "--lr_patch", "3"]).ssim_weight == 0.5          # 3 * 4 = 12 >= 11
    assert parse_args(base + ["--lr_patch", "2"]).lr_patch == 2                                       # no SSIM term: any patch
    for bad in (["--loss", "huber"], ["--ssim_weight", "-0.1"], ["--ssim_weight", "nan"], ["--ssim_weight", "inf"],
                ["--charbonnier_eps", "0"], ["--charbonnier_eps", "-1e-3"], ["--charbonnier_eps", "nan"],
                ["--ssim_weight", "0.2", "--lr_patch", "2"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    with pytest.raises(SystemExit):
        parse_args(["--data_root", "d", "--scale", "X2", "--ssim_weight", "0.2", "--lr_patch", "5"])      # 5 * 2 = 10 < 11
    assert math.isclose(parse_args(["--data_root", "d", "--scale", "X2", "--ssim_weight", "0.2", "--lr_patch", "6"]).ssim_weight, 0.2)
