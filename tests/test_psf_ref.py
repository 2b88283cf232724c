"""Pins tests/psf_ref.py (the fp64 restatement the device tests of the 2-D blur compare against) and blur_kernels' generators: the blur
against F.conv2d on fp64 tensors, the three kernels against their closed forms, the axis-aligned Gaussian against degrade_ref's separable
operator in the interior; shows that each defining choice matters; and asserts, from the reference alone, the cap on undecided 8-bit levels
that tests/test_gpu_psf.py relies on.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import degrade_ref as D
import psf_ref as Pr
from tpu_superresolution_amd import blur_kernels as bk

ULP = 2.0 ** -23


def _asym(ks, seed=0):
    t = np.random.RandomState(seed).rand(ks, ks) + 0.05
    t[0, :] *= 3.0                     # heavy top row, light right column: no symmetry of the square survives
    t[:, -1] *= 0.2
    return (t / t.sum()).astype(np.float32)


def _conv_ref(x, K):
    """F.conv2d (a cross-correlation) on the zero-padded fp64 image, divided by the same of ones."""
    r = K.shape[0] // 2
    w = torch.from_numpy(np.asarray(K, dtype=np.float64))[None, None]
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))[:, None]
    num = F.conv2d(xt, w, padding=r)[:, 0]
    mass = F.conv2d(torch.ones_like(xt[:1]), w, padding=r)[0, 0]
    return (num / mass).numpy(), num.numpy()


@pytest.mark.parametrize("shape,ks", [((3, 45, 61), 7), ((1, 5, 7), 21), ((1, 1, 1), 3), ((2, 9, 4), 3)])
def test_blur2d_is_conv2d_over_conv2d_of_ones(shape, ks):
    x = np.random.RandomState(1).rand(*shape) * 2.0 - 0.5
    K = _asym(ks)
    want, num = _conv_ref(x, K)
    assert np.abs(Pr.blur2d(x, K) - want).max() <= 1e-13
    # a window of pixels has the bits of the same pixels of the whole image
    H, W = shape[-2:]
    rows, cols = (H // 3, H), (0, max(1, W // 2))
    assert np.array_equal(Pr.blur2d(x, K, rows, cols), Pr.blur2d(x, K)[..., rows[0]:rows[1], cols[0]:cols[1]])
    if min(H, W) > 1:
        # negative controls on the asymmetric table: a convolution, the transposed table, no renormalisation
        assert np.abs(Pr.blur2d(x, K, flip=True) - want).max() > 1e-3
        assert np.abs(Pr.blur2d(x, K.T) - want).max() > 1e-3
        raw = Pr.blur2d(x, K, renorm=False)
        assert np.abs(raw - num).max() <= 1e-13 and np.abs(raw - want).max() > 1e-2
        r = ks // 2
        if H > 2 * r and W > 2 * r:          # ... which only shows at the border
            assert np.abs(raw - want)[..., r:H - r, r:W - r].max() <= 1e-6 * 2          # the fp32 table sums to 1 within ks^2 2^-25


def test_zero_padding_and_delta_tables():
    x = np.random.RandomState(2).rand(2, 17, 23) - 0.3
    K = _asym(5)
    assert np.array_equal(Pr.blur2d(x, K), Pr.blur2d(x, Pr.pad_to(K, 21)))
    assert np.array_equal(bk.pad_to(K, 21), Pr.pad_to(K, 21)) and bk.pad_to(K, 21).shape == (21, 21) and bk.pad_to(K, 21)[10, 10] == K[2, 2]
    for ks in (1, 3, 21):
        assert np.array_equal(Pr.blur2d(x, Pr.delta(ks)), x)
    assert np.abs(Pr.blur2d(x, Pr.delta(7, 0.3)) - x).max() <= 1e-15
    with pytest.raises(ValueError):
        bk.pad_to(K, 3)
    with pytest.raises(ValueError):
        bk.pad_to(K, 8)


@pytest.mark.parametrize("ks,s1,s2,theta,beta", [(7, 2.0, 0.7, 0.5, 1.7), (21, 3.0, 1.5, -1.0, 0.6), (3, 0.4, 0.4, 0.0, 4.0), (13, 1.0, 2.5, 1.2, 1.0)])
def test_generators_against_their_closed_forms(ks, s1, s2, theta, beta):
    """blur_kernels inverts Sigma as a matrix; psf_ref writes the rotated quadratic form out element by element."""
    for kind, got in (("gaussian", bk.gaussian(ks, s1, s2, theta)), ("generalized", bk.generalized(ks, s1, s2, theta, beta)),
                      ("plateau", bk.plateau(ks, s1, s2, theta, beta))):
        want = Pr.kernel(kind, ks, s1, s2, theta, beta)
        assert got.dtype == np.float32 and got.shape == (ks, ks)
        assert np.abs(got.astype(np.float64) - want).max() <= ULP * want.max(), kind
        assert abs(got.astype(np.float64).sum() - 1.0) <= ks * ks * 2.0 ** -25
        bk.check_table(got)
        if s1 != s2 and theta != 0.0:          # negative control: the sign of theta
            assert np.abs(Pr.kernel(kind, ks, s1, s2, -theta, beta).astype(np.float64) - got).max() > 1e-4, kind
    # beta = 1: the generalized Gaussian is the Gaussian
    assert np.abs(bk.generalized(ks, s1, s2, theta, 1.0).astype(np.float64) - bk.gaussian(ks, s1, s2, theta)).max() <= ULP


def test_gaussian_at_theta_0_is_the_separable_one_and_90_degrees_swaps_the_sigmas():
    sy, sx = D.f32(1.7), D.f32(1.9)                     # both of radius 6
    assert D.radius(sy) == D.radius(sx) == 6
    want = np.outer(D.gauss(sy), D.gauss(sx))           # rows <-> y
    got = bk.gaussian(13, sx, sy, 0.0)                  # s1 runs along x (columns)
    assert np.abs(got.astype(np.float64) - want).max() <= ULP * want.max()
    assert np.abs(bk.gaussian(13, sy, sx, 0.0).astype(np.float64) - want).max() > 1e-4
    a, b = bk.gaussian(13, sx, sy, np.pi / 2).astype(np.float64), bk.gaussian(13, sy, sx, 0.0).astype(np.float64)
    assert np.abs(a - b).max() <= ULP * b.max()


def _gauss_table(sy, sx):
    """The fp64 outer product of degrade_ref's two normalised Gaussians, zero-padded to the larger radius."""
    r = max(D.radius(sy), D.radius(sx))
    gy, gx = (np.pad(D.gauss(v), r - D.radius(v)) if D.radius(v) else np.pad(np.ones(1), r) for v in (sy, sx))
    return np.outer(gy, gx), r


@pytest.mark.parametrize("s", Pr.SCALES)
def test_interior_agreement_with_the_separable_operator(s):
    """LR = resize(blur2d(HR)) against degrade_ref's composed tables: equal to fp64 rounding for outputs farther than (R + 2 s) / s from the
    border; nearer, the two border rules differ (one renormalisation per LR output against one per blurred pixel and one per cubic table)
    by an amount that is REPORTED here, not bounded."""
    rng = np.random.RandomState(40 + s)
    img = rng.rand(2, 30 * s + (s - 1), 37 * s)
    for sigma in ((1.7, 0.6), (2.5, 2.5), (0.0, 1.1)):
        K, r = _gauss_table(*sigma)
        sep = D.filtered(img, s, *sigma)
        two, _ = Pr.filtered(img, s, K)
        m = -(-(r + 2 * s) // s)
        diff = np.abs(sep - two)
        print(f"x{s} sigma {sigma}: interior max |diff| = {diff[..., m:-m, m:-m].max():.2e}, border max |diff| = {diff.max():.3e} "
              f"(within {m} LR pixels of the border)")
        assert diff[..., m:-m, m:-m].max() <= 1e-12
        assert diff.max() > 1e-6, "the two border rules are expected to differ"


@pytest.mark.parametrize("s", Pr.SCALES)
def test_patch_is_the_window_and_the_blur_is_bounded_by_the_region(s):
    rng = np.random.RandomState(50 + s)
    H, W = 20 * s + (s - 1), 26 * s
    img = rng.rand(1, H, W) * 0.2
    img[:, H - (s - 1):] = 1.0                          # the remainder rows, outside the region
    K = _asym(7, 3)
    whole, _ = Pr.filtered(img, s, K)
    P = 9
    for top, left in ((0, 0), (11 * s, 17 * s), (5 * s, 3 * s)):
        win, _ = Pr.filtered(img, s, K, top, left, P)
        assert np.array_equal(win, whole[..., top // s:top // s + P, left // s:left // s + P])
    # negative control: a blur bounded by the image reads the remainder rows and changes the bottom outputs, and only those
    loose, _ = Pr.filtered(img, s, K, region=False)
    d = np.abs(loose - whole)
    assert d[..., -1, :].min() > 1e-3 and d[..., :10, :].max() == 0.0
    # the NaN footprint: the cubic footprint dilated by the table
    x = img.copy()
    x[0, 7 * s, 9 * s] = np.nan
    got = np.isnan(Pr.filtered(x, s, K)[0])[0]
    assert np.array_equal(got, Pr.nan_footprint(H - H % s, W, s, 7, 7 * s, 9 * s)) and 0 < got.sum() < got.size


def test_bounds_are_formed_as_documented():
    x = np.random.RandomState(8).rand(1, 12, 15) - 0.5
    K = _asym(5, 4)
    n = 25
    num = _conv_ref(np.abs(x), K)[0]                    # S / m
    assert np.allclose(Pr.blur_bound(x, K), 2.0 * (2 * n + 2) * Pr.U * num, rtol=1e-12)
    assert np.array_equal(Pr.blur_bound(x, Pr.pad_to(K, 21)), Pr.blur_bound(x, K))          # n counts the table before padding
    # an fp32 emulation of the device's chains stays inside the bound
    Kf, xf = K.astype(np.float32), x.astype(np.float32)
    r, (H, W) = 2, x.shape[-2:]
    got = np.empty_like(xf)
    for p in range(H):
        for q in range(W):
            a0, m0 = np.float64(0), np.float64(0)
            for a in range(5):
                for b in range(5):
                    y, z = p + a - r, q + b - r
                    if 0 <= y < H and 0 <= z < W:          # fmaf: the exact product-sum (fp64 holds it), rounded once to fp32
                        a0 = np.float64(np.float32(np.float64(Kf[a, b]) * np.float64(xf[0, y, z]) + a0))
                        m0 = np.float64(np.float32(np.float64(Kf[a, b]) + m0))
            got[0, p, q] = np.float32(a0) / np.float32(m0)
    err = np.abs(got.astype(np.float64) - Pr.blur2d(xf, Kf))
    print(f"fp32 emulation: max |err| / bound = {(err / Pr.blur_bound(xf, Kf)).max():.3f}")
    assert (err <= Pr.blur_bound(xf, Kf)).all()


@pytest.mark.parametrize("s", Pr.SCALES)
def test_undecided_levels_stay_under_the_cap(s):
    """The condition of tests/test_gpu_psf.py's quantised comparisons, from the reference alone: at most 1 % of a sample lies within the
    bound of a half-integer level, noise off and on."""
    for k in range(len(Pr.SOURCES)):
        tabs = [smp[2] for smp in Pr.case_samples(s, k)]
        assert sorted({t.shape[0] for t in tabs}) == [3, 7, 21]
        assert all(np.abs(t - t.T).max() > 1e-4 and np.abs(t - t[::-1, ::-1]).max() > 1e-4 for t in tabs), "asymmetric tables"
        a = Pr.case_image(s, k)
        assert a.shape[0] % s != 0
        for noisy in (False, True):
            ref, bnd = Pr.case_reference(s, k, noisy)
            share = Pr.near_half(ref, bnd).reshape(len(ref), -1).mean(axis=1)
            print(f"x{s} {Pr.SOURCES[k]} noisy={noisy}: undecided per sample = {np.round(100 * share, 3).tolist()} %")
            assert share.max() <= 0.01
        assert all(n[0] > 0 for n in Pr.NOISES)
