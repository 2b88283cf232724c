"""The fp64 restatement of the benchmark-protocol PSNR / SSIM (tests/bench_metric_ref.py) against known answers, and the
torch-operator (CPU) form of metrics.bench_metrics against the restatement within the derived bounds.  No GPU."""
import math

import numpy as np
import pytest
import torch

import bench_metric_ref as R
from tpu_superresolution_amd import metrics


def _images(seed, B, C, H, W, noise=0.04):
    """target on the k / 255 grid, pred = target + noise, a few values outside [0, 1]."""
    rng = np.random.RandomState(seed)
    t = (rng.randint(0, 256, size=(B, C, H, W)) / 255.0).astype(np.float32)
    p = (t + noise * rng.standard_normal(t.shape)).astype(np.float32)
    return p, t


# ---- known answers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["y", "rgb"])
def test_identical_images_give_inf_and_one(mode):
    p, _ = _images(0, 2, 3, 19, 23)
    ref = R.bench_ref(p, p, 4, mode)
    assert np.all(np.isposinf(ref["psnr"])) and np.allclose(ref["ssim"], 1.0, rtol=0, atol=1e-12)
    ps, ss = metrics.bench_metrics(torch.from_numpy(p), torch.from_numpy(p.copy()), 4, mode)
    assert ps.dtype == torch.float32 and ps.shape == (2,) and ss.shape == (2,)
    assert bool(torch.isposinf(ps).all()) and float((ss - 1).abs().max()) <= 1e-6


def test_one_level_everywhere_is_mse_one():
    rng = np.random.RandomState(1)
    k = rng.randint(0, 255, size=(2, 3, 19, 23))
    t, p = (k / 255.0).astype(np.float32), ((k + 1) / 255.0).astype(np.float32)
    ref = R.bench_ref(p, t, 4, "rgb")
    assert np.array_equal(ref["sqsum"], np.full(2, 3 * 11 * 15.0))
    assert np.allclose(ref["psnr"], 20 * math.log10(255.0), rtol=0, atol=1e-12)
    ps, _ = metrics.bench_metrics(torch.from_numpy(p), torch.from_numpy(t), 4, "rgb")
    assert float((ps.double() - 20 * math.log10(255.0)).abs().max()) <= float(R.psnr_bound(ref["sqsum"], 3 * 11 * 15, "rgb", 3).max())


def test_grey_replicated_to_rgb_gains_the_luma_range_factor():
    p, t = _images(2, 2, 1, 19, 23)
    p3, t3 = np.repeat(p, 3, axis=1), np.repeat(t, 3, axis=1)
    y, rgb = R.bench_ref(p3, t3, 4, "y"), R.bench_ref(p3, t3, 4, "rgb")
    assert np.allclose(y["psnr"] - rgb["psnr"], 20 * math.log10(255.0 / 219.0), rtol=0, atol=1e-9)
    # a single-channel image is its own luma: the grey image itself scores like its RGB replication in mode rgb
    assert np.allclose(R.bench_ref(p, t, 4, "y")["psnr"], rgb["psnr"], rtol=0, atol=1e-12)


# ---- rounding ties -----------------------------------------------------------------------------------------------------------------
def test_every_half_level_has_an_fp32_tie_and_rounds_to_even():
    x, k = R.tie_inputs()
    assert x.size == 255 and np.array_equal(k, np.arange(255))
    assert int((k % 2 == 0).sum()) == 128 and int((k % 2 == 1).sum()) == 127
    assert np.array_equal(x.astype(np.float32) * np.float32(255.0), (k + 0.5).astype(np.float32))
    even = np.where(k % 2 == 0, k, k + 1).astype(np.float64)
    assert np.array_equal(R.quantise(x), even)
    got = metrics.bench_planes_torch(torch.from_numpy(x).view(1, 1, 15, 17), 0, "rgb")
    assert np.array_equal(got.numpy().reshape(-1).astype(np.float64), even)
    assert not np.array_equal(np.floor(x * np.float32(255.0)), even)          # the truncation of a PNG dump is another function


def test_a_nan_stays_and_values_outside_the_range_clamp():
    x = np.array([[[[-0.5, 1.5, float("nan"), 0.25]]]], dtype=np.float32)
    q = R.quantise(x).reshape(-1)
    assert q[0] == 0 and q[1] == 255 and np.isnan(q[2]) and q[3] == 64
    got = metrics.bench_planes_torch(torch.from_numpy(x), 0, "rgb").reshape(-1)
    assert got[0] == 0 and got[1] == 255 and bool(torch.isnan(got[2])) and got[3] == 64


# ---- negative controls: each departure from the protocol moves the PSNR beyond the bound ------------------------------------------------
B_, C_, H_, W_, BORDER = 3, 3, 24, 28, 4


@pytest.fixture(scope="module")
def case():
    p, t = _images(3, B_, C_, H_, W_)
    p[:, :, :BORDER] += 0.1                                    # the frame scores worse than the interior
    ref = R.bench_ref(p, t, BORDER, "y")
    bound = R.psnr_bound(ref["sqsum"], ref["pp"][0].size, "y", 3)
    return p, t, ref, bound


def _psnr_of(pp, pt, max_val=255.0):
    return R.psnr_from_sqsum(R.sqsum(pp, pt), pp[0].size, max_val)


def _crop(a, b):
    return a[:, :, b:a.shape[2] - b, b:a.shape[3] - b]


def _luma(x, border, coef=R.BT601, offset=16.0, quant=R.quantise):
    q = _crop(quant(x), border)
    return (offset + (coef[0] * q[:, 0] + coef[1] * q[:, 1] + coef[2] * q[:, 2]) / 255.0)[:, None]


def test_the_helpers_of_the_controls_restate_the_reference(case):
    p, t, ref, _ = case
    assert np.array_equal(_psnr_of(_luma(p, BORDER), _luma(t, BORDER)), ref["psnr"])


def _truncate(x):
    return np.floor(np.clip(np.asarray(x, dtype=np.float32), 0, 1) * np.float32(255.0)).astype(np.float64)


BT709 = (0.2126 * 219.0, 0.7152 * 219.0, 0.0722 * 219.0)
CONTROLS = {
    "truncation": lambda p, t: _psnr_of(_luma(p, BORDER, quant=_truncate), _luma(t, BORDER, quant=_truncate)),
    "no_crop": lambda p, t: _psnr_of(_luma(p, 0), _luma(t, 0)),
    "crop_one_less": lambda p, t: _psnr_of(_luma(p, BORDER - 1), _luma(t, BORDER - 1)),
    "bt709": lambda p, t: _psnr_of(_luma(p, BORDER, coef=BT709), _luma(t, BORDER, coef=BT709)),
    "offset_on_one_side": lambda p, t: _psnr_of(_luma(p, BORDER, offset=0.0), _luma(t, BORDER)),
    "max_val_one": lambda p, t: _psnr_of(_luma(p, BORDER), _luma(t, BORDER), max_val=1.0),
}


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_control(case, name):
    p, t, ref, bound = case
    moved = np.abs(CONTROLS[name](p, t) - ref["psnr"])
    assert np.all(moved > bound), (name, moved, bound)


def test_negative_control_mean_over_batches(case):
    _, _, ref, bound = case
    per_image = ref["psnr"]                                     # three images in batches of two: the last batch is short
    over_batches = (per_image[:2].mean() + per_image[2:].mean()) / 2
    assert abs(over_batches - per_image.mean()) > bound.max()


# ---- the torch-operator form of metrics.bench_metrics --------------------------------------------------------------------------------
CASES = [(1, 3, 9, 10, 4, "y"), (3, 3, 19, 23, 4, "y"), (3, 3, 19, 23, 4, "rgb"), (2, 1, 33, 37, 3, "y"), (2, 3, 70, 129, 0, "y"),
         (2, 3, 70, 129, 0, "rgb"), (2, 4, 19, 23, 2, "rgb")]


@pytest.mark.parametrize("B,C,H,W,border,mode", CASES)
def test_cpu_form_is_within_the_bounds_of_the_restatement(B, C, H, W, border, mode):
    p, t = _images(10 + H, B, C, H, W)
    p[0, 0, border, border], p[0, -1, H - border - 1, W - border - 1] = -0.25, 1.25
    ref = R.bench_ref(p, t, border, mode)
    with_ssim = ref["ssim"] is not None
    tp, tt = torch.from_numpy(p), torch.from_numpy(t)
    for x, want in ((tp, ref["pp"]), (tt, ref["pt"])):
        got = metrics.bench_planes_torch(x, border, mode)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        assert float(np.abs(got.numpy().astype(np.float64) - want).max()) <= R.plane_bound(mode, C)
    ps, ss = metrics.bench_metrics(tp, tt, border, mode, with_ssim=with_ssim)
    count = ref["pp"][0].size
    err = np.abs(ps.numpy().astype(np.float64) - ref["psnr"])
    assert np.all(err <= R.psnr_bound(ref["sqsum"], count, mode, C)), (err, R.psnr_bound(ref["sqsum"], count, mode, C))
    if with_ssim:
        assert float(np.abs(ss.numpy().astype(np.float64) - ref["ssim"]).max()) <= R.SSIM_BOUND
    else:
        assert ss is None


def test_bench_metrics_refuses_what_the_protocol_cannot_score():
    x = torch.rand(2, 3, 19, 23)
    with pytest.raises(ValueError, match="11 x 11"):
        metrics.bench_metrics(x, x, 5, "y")                   # 9 x 13 left
    assert metrics.bench_metrics(x, x, 5, "y", with_ssim=False)[1] is None
    for bad in (dict(crop_border=10), dict(crop_border=-1), dict(crop_border=4, mode="ycbcr"), dict(crop_border=1.0)):
        with pytest.raises(ValueError):
            metrics.bench_metrics(x, x, **bad)
    with pytest.raises(ValueError, match="C = 2"):
        metrics.bench_metrics(x[:, :2], x[:, :2], 4, "y")
    with pytest.raises(ValueError):
        metrics.bench_metrics(x, x[:, :, 1:], 4, "y")
