"""tests/usm_ref.py pinned: against F.conv2d of the reflect-padded input with outer(k, k) in fp64, against a from-the-formulas restatement
of the sharpening, and against negative controls -- what srk_usm_sharpen_f32 must NOT compute.  Also the undecided-pixel cap of the GPU
tests' images, a condition on the reference alone.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import usm_ref as Ur


def _x(seed=1, shape=(40, 72), C=3):
    return Ur.image(seed, shape, channels=C)


@pytest.mark.parametrize("ks", [51, 21, 3, 1])
def test_gauss_is_conv2d_of_the_reflect_padded_input(ks):
    x = _x(2, (33, 50))
    k = Ur.gaussian1d(ks).astype(np.float64)
    R = ks // 2
    xt = torch.from_numpy(x.astype(np.float64))[:, None]
    want = F.conv2d(F.pad(xt, (R, R, R, R), mode="reflect") if R else xt, torch.from_numpy(np.outer(k, k))[None, None])[:, 0].numpy()
    assert np.max(np.abs(Ur.gauss(x, k) - want)) < 1e-14


def test_usm_is_the_formulas():
    x = _x(3).astype(np.float64)
    k = Ur.gaussian1d(51).astype(np.float64)
    R = 25
    k2 = torch.from_numpy(np.outer(k, k))[None, None]
    blur = lambda v: F.conv2d(F.pad(torch.from_numpy(v)[:, None], (R,) * 4, mode="reflect"), k2)[:, 0].numpy()          # noqa: E731
    w, thr = float(np.float32(0.5)), 10.0
    res = x - blur(x)
    mask = (np.abs(res) * 255.0 > thr).astype(np.float64)
    soft = blur(mask)
    sharp = np.clip(x + w * res, 0.0, 1.0)
    want = soft * sharp + (1.0 - soft) * x
    r = Ur.usm(x, k, 0.5, 10.0)
    assert np.max(np.abs(r["out"] - want)) < 1e-13
    assert 0.02 < r["mask"].mean() < 0.98 and np.max(np.abs(r["out"] - x)) > 0.02          # the image exercises both branches


@pytest.mark.parametrize("control", [dict(border="zero"), dict(border="replicate"), dict(use_abs=False), dict(thr_scale=1.0), dict(clip=False),
                                     dict(hard=True), dict(swapped=True)], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_negative_controls_differ(control):
    x = _x(4)
    k = Ur.gaussian1d(51)
    iv = Ur.intervals(x, k, 1.5 if "clip" in control else 0.5, 10.0)
    wrong = Ur.usm(x, k, 1.5 if "clip" in control else 0.5, 10.0, **control)["out"]
    outside = (wrong < iv["lo"]) | (wrong > iv["hi"])
    assert outside.mean() > 0.01, f"the control {control} lies inside the derived hull: the GPU test could not tell it apart"


def test_sigma_rule_is_opencvs():
    assert np.isclose(0.3 * (25 - 1) + 0.8, 8.0)
    a, b = Ur.gaussian1d(51), Ur.gaussian1d(51, rule="ks/6")
    assert np.max(np.abs(a - b)) > 1e-4
    x = _x(5)
    iv = Ur.intervals(x, a)
    wrong = Ur.usm(x, b)["out"]
    assert ((wrong < iv["lo"]) | (wrong > iv["hi"])).mean() > 0.01


def test_reference_is_inside_its_own_hull_and_exact_cases():
    x = _x(6)
    for ks in (51, 3, 1):
        k = Ur.gaussian1d(ks)
        iv = Ur.intervals(x, k)
        assert ((iv["ref"]["out"] >= iv["lo"]) & (iv["ref"]["out"] <= iv["hi"])).all()
    assert np.array_equal(Ur.usm(x, np.ones(1, np.float32))["out"], x.astype(np.float64))
    assert np.array_equal(Ur.usm(x, Ur.gaussian1d(51), 0.5, 1e9)["out"], x.astype(np.float64))


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("shape", Ur.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ks", [51, 3])
def test_undecided_cap_of_the_gpu_images(ks, shape, C):
    """At most 1 % of the mask pixels of every image of tests/test_gpu_usm.py are undecided: from the reference alone."""
    x = Ur.image(7 + C, shape, channels=C, batch=2)
    for thr in (10.0, -1.0):
        iv = Ur.intervals(x, Ur.gaussian1d(ks), 0.5, thr)
        for b in range(2):
            assert iv["undecided"][b].mean() <= 0.01
