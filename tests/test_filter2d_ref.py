"""Pins tests/filter2d_ref.py (the fp64 restatement of srk_filter2d_f32) against torch's own reflect padding and convolution, the sinc
tables and their Bessel function against published values, and the host side of the second-order degradation: SecondOrderSpec's
generator, the clamped window of DeviceHR2Pool, the parsers' refusals.  No GPU."""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import filter2d_ref as Fr
from tpu_superresolution_amd import blur_kernels as bk


def _asym_table(ks, seed=0):
    rng = np.random.RandomState(seed)
    K = rng.randn(ks, ks)
    K[0, -1] += 2.0          # neither symmetric nor point-symmetric
    return (K / K.sum()).astype(np.float32)


@pytest.mark.parametrize("ks", [1, 3, 7, 21])
def test_reference_is_conv2d_on_a_reflect_padded_input(ks):
    rng = np.random.RandomState(ks)
    x = rng.rand(3, 23, 31)
    K = _asym_table(ks, ks).astype(np.float64)
    R = ks // 2
    xp = F.pad(torch.from_numpy(x)[None], (R, R, R, R), mode="reflect") if R else torch.from_numpy(x)[None]
    want = F.conv2d(xp, torch.from_numpy(K)[None, None].repeat(3, 1, 1, 1), groups=3)[0].numpy()          # conv2d is a correlation
    assert np.abs(Fr.filter2d(x, K) - want).max() <= 1e-13
    assert np.array_equal(Fr.filter2d(x, Fr.delta(ks)), x)


def test_rho_is_reflect_101_and_clamps():
    assert Fr.rho(np.arange(-3, 8), 5).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert Fr.rho(np.arange(-4, 5), 1).tolist() == [0] * 9 and Fr.rho(np.array([-9, 9]), 3).tolist() == [2, 0]          # past one reflection: clamped


def test_negative_controls_are_told_apart():
    """What the kernel must NOT compute differs from the reference by far more than the tolerance."""
    x = np.random.RandomState(1).rand(2, 19, 26).astype(np.float32)
    K = _asym_table(7, 3)
    ref, bnd = Fr.filter2d(x, K), Fr.bound(x, K)
    for name, other in [("zero border", Fr.filter2d(x, K, border="zero")), ("replicate border", Fr.filter2d(x, K, border="replicate")),
                        ("flipped table (a convolution)", Fr.filter2d(x, K, flip=True)), ("mass-normalised", Fr.filter2d(x, K, border="mass")),
                        ("b as the outer index", Fr.filter2d(x, K, transpose=True))]:
        excess = np.abs(other - ref) / bnd
        assert excess.max() > 1e3, name
        if "border" in name or "mass" in name:          # the border rules agree in the interior and only there
            # (the mass of an fp32 table is 1 only to its rounding, so that rule is off by a relative 1e-7 in the interior)
            assert np.abs(other - ref)[:, 3:-3, 3:-3].max() <= (1e-6 if "mass" in name else 1e-12), name
            assert (excess[:, :3].max() > 1e3) and (excess[:, :, -3:].max() > 1e3), name


def test_bound_covers_an_fp32_chain_in_the_kernels_order():
    """The kernel's chain, restated in numpy fp32 (products rounded twice, so a little worse than fmaf): inside the bound."""
    rng = np.random.RandomState(2)
    x = (rng.rand(17, 21) * 1.5 - 0.25).astype(np.float32)
    for K in (bk.sinc(math.pi / 3, 7), bk.sinc(2.8, 13)):
        R = K.shape[0] // 2
        xp = x[Fr.rho(np.arange(-R, 17 + R), 17)][:, Fr.rho(np.arange(-R, 21 + R), 21)]
        acc = np.zeros((17, 21), dtype=np.float32)
        for a in range(K.shape[0]):
            for b in range(K.shape[0]):
                acc = (acc + K[a, b] * xp[a:a + 17, b:b + 21]).astype(np.float32)
        assert (np.abs(acc - Fr.filter2d(x, K)) <= Fr.bound(x, K)).all()


def test_j1_values():
    assert abs(float(bk.j1(1.0)) - 0.44005058574493355) <= 1e-15
    assert abs(float(bk.j1(2.0)) - 0.5767248077568734) <= 1e-15
    assert abs(float(bk.j1(3.8317059702075125))) <= 1e-15          # its first zero
    assert abs(float(bk.j1(0.0))) <= 1e-15 and abs(float(bk.j1(-1.0)) + 0.44005058574493355) <= 1e-15
    with pytest.raises(ValueError):
        bk.j1(float("nan"))
    with pytest.raises(ValueError):
        bk.j1(250.0)


def test_j1_against_scipy():
    special = pytest.importorskip("scipy.special")
    z = np.linspace(-60.0, 60.0, 2401)
    assert np.abs(bk.j1(z) - special.j1(z)).max() <= 5e-15


@pytest.mark.parametrize("ks", [7, 13, 21])
@pytest.mark.parametrize("cutoff", [math.pi / 5, 1.0, math.pi])
def test_sinc_tables(ks, cutoff):
    K = bk.sinc(cutoff, ks)
    assert K.dtype == np.float32 and K.shape == (ks, ks)
    assert np.array_equal(K, K.T) and np.array_equal(K, K[::-1]) and np.array_equal(K, K[:, ::-1])
    assert abs(float(K.astype(np.float64).sum()) - 1.0) <= ks * ks * 2.0 ** -25 * float(np.abs(K).sum())
    assert (K < 0).any() or cutoff * ks < 8, "a sinc table has negative lobes"
    # the formula, tap by tap
    R = ks // 2
    raw = np.empty((ks, ks))
    for a in range(ks):
        for b in range(ks):
            r = math.hypot(a - R, b - R)
            raw[a, b] = cutoff * cutoff / (4 * math.pi) if r == 0 else cutoff * float(bk.j1(cutoff * r)) / (2 * math.pi * r)
    assert np.array_equal(K, (raw / raw.sum()).astype(np.float32))
    assert bk.check_filter_table(K) is not None
    if (K < 0).any():
        with pytest.raises(ValueError):
            bk.check_table(K)          # the rule of blur2d: no negative taps


def test_sinc_and_table_refusals():
    for bad in (0.0, -1.0, 3.2, float("nan")):
        with pytest.raises(ValueError):
            bk.sinc(bad, 7)
    for ks in (0, 4, 23):
        with pytest.raises(ValueError):
            bk.sinc(1.0, ks)
    ok = bk.sinc(1.0, 7)
    for bad in (ok * 1.01, np.where(np.arange(49).reshape(7, 7) == 3, np.nan, ok), ok[:6], ok[:, :6], np.zeros((23, 23))):
        with pytest.raises(ValueError):
            bk.check_filter_table(bad)
    assert np.array_equal(bk.delta(5), Fr.delta(5)) and bk.check_filter_table(-ok + 2 * bk.delta(7)) is not None          # signs are free


@pytest.mark.parametrize("ks", [7, 13, 21])
def test_quantised_levels_are_decided_by_the_reference_on_dim_images(ks):
    """The 1 % cap of tests/test_gpu_degrade2.py, from the reference alone: on levels 0..31 a sinc table leaves under 1 % of a sample
    within the bound of a half-integer."""
    for b, cutoff in enumerate((math.pi / 3, 2.5)):
        x, K = Fr.dim_image(40 + b, channels=3), bk.sinc(cutoff, ks)
        share = Fr.near_half(Fr.filter2d(x, K), Fr.bound(x, K)).mean()
        print(f"ks {ks} cutoff {cutoff:.3f}: {100 * share:.3f} % undecided")
        assert share <= 0.01


# ---- SecondOrderSpec ----------------------------------------------------------------------------------------------------------------------
class _Counting(random.Random):
    calls = 0

    def random(self):
        type(self).calls += 1
        return super().random()


def _draws(spec, rng, n, E=96, s=4):
    from tpu_superresolution_amd.sr_datasets import stage1_table
    t = stage1_table((1.0, 1.5))
    return [spec.draw(rng, t, (0.01, 0.0), i, False, True, E, s) for i in range(n)]


def test_spec_takes_a_fixed_number_of_variates():
    from tpu_superresolution_amd.sr_datasets import SECOND_ORDER_VARIATES, SecondOrderSpec
    for spec in (SecondOrderSpec(), SecondOrderSpec(blur2_p=0.0, sinc_p=1.0, final_sinc_p=0.0), SecondOrderSpec(resize_prob=(0, 0, 1), sinc_p=0.0)):
        rng = _Counting("x")
        for k in range(1, 40):
            _Counting.calls = 0
            _draws(spec, rng, 1)
            assert _Counting.calls == SECOND_ORDER_VARIATES == 23


def test_spec_is_deterministic_per_seed_and_rank_and_leaves_random_alone():
    from tpu_superresolution_amd.sr_datasets import SecondOrderSpec

    def key(ps):
        return [(p.r1, p.r2, p.q1, p.q2, p.jpeg_last, p.noise2, p.gray2, p.k1.tobytes(), p.k2.tobytes(), p.k3.tobytes()) for p in ps]

    random.seed(1234)
    state = random.getstate()
    a = key(_draws(SecondOrderSpec(seed=5), SecondOrderSpec(seed=5).rng(1), 20))
    assert random.getstate() == state
    assert a == key(_draws(SecondOrderSpec(seed=5), SecondOrderSpec(seed=5).rng(1), 20))
    assert a == key(_draws(SecondOrderSpec(seed=6), SecondOrderSpec(seed=6).rng(0), 20))          # seed + rank
    assert a != key(_draws(SecondOrderSpec(seed=5), SecondOrderSpec(seed=5).rng(0), 20))
    assert SecondOrderSpec(seed=5).rng(1).random() == random.Random("degrade2:6").random()


def test_spec_draws_stay_in_their_ranges_and_fit_the_kernels():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import SecondOrderSpec
    spec = SecondOrderSpec()
    seen = {"up": 0, "down": 0, "keep": 0, "sinc1": 0, "delta2": 0, "sinc3": 0, "A": 0, "B": 0}
    for E, s in ((48, 2), (96, 3), (288, 4), (40, 4)):
        for p in _draws(spec, spec.rng(E), 600, E, s):
            (h1, _), (h2, _), (ho, _) = ops.second_order_sizes(E, E, s, p)
            assert 0.15 <= p.r1 <= 1.5 and p.r2 <= 1.2 and 30 <= p.q1 <= 95 and 30 <= p.q2 <= 95
            assert E <= 8 * h1 and h1 <= 8 * h2 and h2 <= 8 * ho, "a resize of the chain would shrink by more than 8x"
            assert p.k2.shape[0] // 2 < h1 and p.k1.shape[0] // 2 < E and p.k3.shape[0] // 2 < ho, "a table does not fit the size it filters"
            for k in (p.k1, p.k2, p.k3):
                bk.check_filter_table(k)
            seen["up" if p.r1 > 1 else "down" if p.r1 < 1 else "keep"] += 1
            seen["sinc1"] += bool((p.k1 < 0).any())
            seen["delta2"] += p.k2.shape[0] == 1
            seen["sinc3"] += p.k3.shape[0] > 1
            seen["B" if p.jpeg_last else "A"] += 1
    n = 2400
    assert abs(seen["up"] / n - 0.2) < 0.05 and abs(seen["down"] / n - 0.7) < 0.05 and abs(seen["keep"] / n - 0.1) < 0.05
    assert 0.03 < seen["sinc1"] / n < 0.2 and 0.15 < seen["delta2"] / n < 0.35 and abs(seen["sinc3"] / n - 0.8) < 0.05
    assert abs(seen["A"] / n - 0.5) < 0.05


def test_spec_fixed_is_the_documented_midpoints():
    from tpu_superresolution_amd.sr_datasets import SecondOrderSpec, stage1_table
    t = stage1_table((1.1, 1.1))
    p = SecondOrderSpec().fixed(t, (0.02, 0.0), True, 7)
    assert p.k1 is t and p.r1 == 0.575 and p.r2 == 0.65 and p.q1 == 62 and p.q2 == 62 and p.jpeg_last is False and p.noise_id == 7
    assert p.noise1 == (0.02, 0.0) and p.gray1 is True and p.gray2 is False and abs(p.noise2[0] - 13.0 / 255.0) < 1e-12 and p.noise2[1] == 0.0
    assert np.array_equal(p.k2, bk.gaussian(13, 0.85, 0.85)) and np.array_equal(p.k3, bk.sinc(0.5 * (math.pi / 5 + math.pi), 13))
    q = SecondOrderSpec(blur2_p=0.2, final_sinc_p=0.1).fixed(t, (0.0, 0.0))
    assert q.k2.shape == (1, 1) and q.k3.shape == (1, 1)


def test_spec_refusals():
    from tpu_superresolution_amd.sr_datasets import SecondOrderSpec
    for kw in (dict(resize_prob=(0.5, 0.6, 0.1)), dict(resize_prob=(1.0, 0.0)), dict(resize_range=(0.1, 1.5)), dict(resize_range=(0.5, 0.9)),
               dict(resize2_range=(0.3, 2.5)), dict(blur2_p=1.5), dict(sinc_p=float("nan")), dict(final_sinc_p=-0.1), dict(ksize=(8, 21)),
               dict(ksize=(9, 7)), dict(blur2_sigma=(0.0, 1.0)), dict(noise2_sigma=(0.5, 0.1)), dict(jpeg_quality=(0, 95)),
               dict(jpeg2_quality=(96, 95)), dict(gray_noise_p=2)):
        with pytest.raises(ValueError):
            SecondOrderSpec(**kw)


# ---- the clamped window -------------------------------------------------------------------------------------------------------------------
def test_window_arithmetic_in_the_corners_and_the_interior():
    from tpu_superresolution_amd.sr_datasets import second_order_window
    s, P, m = 2, 16, 4
    E = s * (P + 2 * m)
    Hr, Wr = 100, 130
    last_t, last_l = Hr - P * s, Wr - P * s
    cases = {(0, 0): (0, 0, 0, 0), (0, last_l): (0, Wr - E, 0, 2 * m), (last_t, 0): (Hr - E, 0, 2 * m, 0),
             (last_t, last_l): (Hr - E, Wr - E, 2 * m, 2 * m), (40, 50): (40 - s * m, 50 - s * m, m, m),
             (4, 50): (0, 50 - s * m, 2, m), (s * m, s * m): (0, 0, m, m)}
    for (top, left), want in cases.items():
        got = second_order_window(top, left, Hr, Wr, s, P, m)
        assert got == want == Fr.window_origin(top, left, Hr, Wr, s, P, m), (top, left)
        wt, wl, oy, ox = got
        assert 0 <= wt <= Hr - E and 0 <= wl <= Wr - E and wt + oy * s == top and wl + ox * s == left and 0 <= oy <= 2 * m and 0 <= ox <= 2 * m
    # a region of exactly E: every patch clamps to the one window
    for top in range(0, E - P * s + 1, s):
        assert second_order_window(top, 0, E, E, s, P, m) == (0, 0, top // s, 0)
