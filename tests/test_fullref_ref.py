"""Pins tests/fullref_ref.py, the fp64 restatement the PSNR-B / MS-SSIM kernels are held against: known answers, torch's avg_pool2d and the
SSIM pieces of metrics.py in fp64, the published count rule, the odd-extent pooling cell, and negative controls -- each wrong reading of
the definition that the pin must catch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fullref_ref as R


def _blocky(H, W, d, seed=0):
    """Constant 8 x 8 blocks on the grid anchored at (0, 0); neighbouring blocks differ by exactly d (a checkerboard of two levels)."""
    yy, xx = np.meshgrid(np.arange(H) // 8, np.arange(W) // 8, indexing="ij")
    return 100.0 + d * ((yy + xx) % 2)


def _ramp(H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return 20.0 + xx + yy                                        # every neighbour pair differs by 1: D_b = D_n


# ---- PSNR-B ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(32, 48), (64, 64)])
def test_constant_blocks_give_the_closed_form(H, W):
    d = 6.0
    p = _blocky(H, W, d)
    t = p + 2.0                                                  # mse = 4
    s = R.psnrb_sums(p, t)
    n_b, n_n = R.psnrb_counts(H, W)
    assert s[2] == 0 and s[4] == 0                                # D_n = 0
    assert s[1] == d * d * H * (W // 8 - 1) and s[3] == d * d * W * (H // 8 - 1)      # every boundary pair steps by d: D_b = d^2
    mse, bef, d_b, d_n = R.psnrb_parts(s, H, W)
    assert (mse, d_b, d_n) == (4.0, d * d, 0.0)
    want = 10.0 * math.log10(65025.0 / (4.0 + 3.0 / math.log2(min(H, W)) * d * d))
    assert R.psnrb_plane(p, t) == pytest.approx(want, rel=1e-14)
    assert R.psnrb(p[None, None], t[None, None])[0] == pytest.approx(want, rel=1e-14)


def test_a_smooth_ramp_has_no_blocking_effect_and_equals_psnr():
    p = _ramp(40, 56)
    t = p + np.where(np.arange(56) % 2 == 0, 1.0, -2.0)[None, :]
    mse, bef, d_b, d_n = R.psnrb_parts(R.psnrb_sums(p, t), 40, 56)
    assert bef == 0.0 and d_b <= d_n
    assert R.psnrb_plane(p, t) == pytest.approx(10.0 * math.log10(65025.0 / ((p - t) ** 2).mean()), rel=1e-14)


def test_cropping_four_pixels_moves_the_steps_off_the_grid():
    p = _blocky(48, 48, 10.0)
    t = p + 1.0
    assert R.psnrb_parts(R.psnrb_sums(p, t), 48, 48)[1] > 0
    pc, tc = p[4:-4, 4:-4], t[4:-4, 4:-4]
    mse, bef, d_b, d_n = R.psnrb_parts(R.psnrb_sums(pc, tc), 40, 40)
    assert d_b == 0.0 and d_n > 0 and bef == 0.0
    assert R.psnrb_plane(pc, tc) == pytest.approx(10.0 * math.log10(65025.0), rel=1e-14)


def test_equal_planes_without_blockiness_give_inf_and_a_nan_reaches_the_result():
    p = _ramp(16, 24)
    assert R.psnrb_plane(p, p) == float("inf")
    q = p.copy()
    q[5, 7] = np.nan
    assert math.isnan(R.psnrb_plane(q, p)) and math.isnan(R.psnrb_plane(p, q))


def test_the_published_counts_are_kept_at_an_extent_of_1_mod_8():
    """Wc = 17: boundary columns 7 and 15 (15 < Wc - 1), two lines of Hc pairs in Dh_b, but n_bh = Hc (17 // 8 - 1) = Hc."""
    H, W = 16, 17
    rng = np.random.RandomState(0)
    p = np.round(rng.rand(H, W) * 255)
    s = R.psnrb_sums(p, p)
    assert s[1] == sum(((p[:, x] - p[:, x + 1]) ** 2).sum() for x in (7, 15))
    n_b, n_n = R.psnrb_counts(H, W)
    assert n_b == H * 1 + W * 1 and n_n == H * 16 - H + W * 15 - W
    H, W = 25, 16                                                 # rows 7, 15, 23: three lines, n_bv = Wc (25 // 8 - 1) = 2 Wc
    p = np.round(rng.rand(H, W) * 255)
    assert R.psnrb_sums(p, p)[3] == sum(((p[y] - p[y + 1]) ** 2).sum() for y in (7, 15, 23))
    assert R.psnrb_counts(H, W)[0] == H * 1 + W * 2


def test_negative_controls_of_psnrb():
    """A boundary at x % 8 == 0 and a blocking effect taken from the target must each change the known answers."""
    p = _blocky(32, 48, 6.0)
    t = _ramp(32, 48)
    right = R.psnrb_plane(p, t)
    assert R.psnrb_sums(p, t, phase=0)[1] == 0.0 and R.psnrb_sums(p, t, phase=0)[2] > 0       # the steps land on the 'other' side
    assert R.psnrb_plane(p, t, phase=0) > right + 0.01            # ... and bef vanishes: the wrong phase reports plain PSNR
    assert R.psnrb_plane(p, t, bef_from="target") > right + 0.01  # the target is smooth: no bef
    assert R.psnrb_plane(t, p) == pytest.approx(R.psnrb_plane(p, t, bef_from="target"), rel=1e-14)      # the score is not symmetric


# ---- MS-SSIM ---------------------------------------------------------------------------------------------------------------------------
def _pair(H, W, sigma=12, seed=1):
    x = R.pink_image(seed, H, W)
    return x, R.noised(x, sigma, seed)


def _torch_msssim(x, y, weights=R.WEIGHTS, include_pad=True):
    """F.avg_pool2d + the SSIM pieces of metrics.py, in fp64.  The window is formed in fp64 here: metrics.gaussian_window rounds its taps to
    fp32 first, as the published package does, which moves the means by some 4e-7."""
    from tpu_superresolution_amd import metrics as M
    X, Y = torch.from_numpy(x)[None, None], torch.from_numpy(y)[None, None]
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5.0) ** 2 / 4.5)
    win = g / g.sum()
    vals, means = [], []
    for s in range(len(weights)):
        S, CS = M._ssim_channel_means(X, Y, win, 255.0, (0.01, 0.03))
        means.append((float(S), float(CS)))
        vals.append(max(float(CS if s < len(weights) - 1 else S), 0.0) ** weights[s])
        pad = [n % 2 for n in X.shape[2:]]
        X = F.avg_pool2d(X, 2, padding=pad, count_include_pad=include_pad)
        Y = F.avg_pool2d(Y, 2, padding=pad, count_include_pad=include_pad)
    return float(np.prod(vals)), np.array(means)


@pytest.mark.parametrize("H,W", [(161, 161), (176, 163)])
def test_msssim_equals_the_torch_pieces_in_fp64(H, W):
    x, y = _pair(H, W)
    want, want_means = _torch_msssim(x, y)
    means, pyr = R.msssim_levels(x, y)
    np.testing.assert_allclose(means, want_means, rtol=1e-10, atol=1e-12)
    assert R.msssim(x[None, None], y[None, None])[0] == pytest.approx(want, rel=1e-10)
    assert [a.shape for a, _ in pyr] == [tuple((n + (1 << s) - 1) >> s for n in (H, W)) for s in (1, 2, 3, 4)]


def test_pool_equals_avg_pool2d_and_the_odd_extent_cell_is_divided_by_four():
    rng = np.random.RandomState(3)
    for H, W in [(5, 6), (6, 5), (7, 9), (4, 4)]:
        a = np.round(rng.rand(H, W) * 255)
        want = F.avg_pool2d(torch.from_numpy(a)[None, None], 2, padding=[H % 2, W % 2])[0, 0].numpy()
        assert np.array_equal(R.pool(a), want), (H, W)
    a = np.arange(35, dtype=np.float64).reshape(5, 7) + 1.0
    o = R.pool(a)
    assert o.shape == (3, 4)
    assert o[0, 0] == a[0, 0] / 4 and o[0, 1] == (a[0, 1] + a[0, 2]) / 4 and o[1, 0] == (a[1, 0] + a[2, 0]) / 4
    assert o[2, 3] == (a[3, 5] + a[3, 6] + a[4, 5] + a[4, 6]) / 4


def test_identical_images_give_one_and_one_level_is_ssim():
    from tpu_superresolution_amd import metrics as M
    x, y = _pair(161, 170)
    assert R.msssim(x[None, None], x[None, None])[0] == pytest.approx(1.0, abs=1e-12)
    one = R.msssim(x[None, None], y[None, None], weights=(1.0,))[0]
    assert one == pytest.approx(R.ssim_means(x, y)[0], rel=1e-14)
    # ssim_torch's window holds fp32 taps
    assert one == pytest.approx(float(M.ssim_torch(torch.from_numpy(x)[None, None], torch.from_numpy(y)[None, None], 255.0)), rel=2e-6)


def test_negative_controls_of_msssim():
    """Pooling that leaves the pad out of the count and S in place of CS at the fine levels must each move the score."""
    x, y = _pair(161, 161, sigma=30)
    right = R.msssim(x[None, None], y[None, None])[0]
    assert right == pytest.approx(_torch_msssim(x, y)[0], rel=1e-10)
    no_pad = R.msssim(x[None, None], y[None, None], include_pad=False)[0]
    assert no_pad == pytest.approx(_torch_msssim(x, y, include_pad=False)[0], rel=1e-10)
    assert abs(no_pad - right) > 1e-4
    assert abs(R.msssim(x[None, None], y[None, None], cs_fine=False)[0] - right) > 1e-4
    a = np.full((5, 5), 8.0)
    assert R.pool(a)[0, 0] == 2.0 and R.pool(a, include_pad=False)[0, 0] == 8.0
