"""tests/niqe_ref.py (the fp64 restatement of BasicSR's calculate_niqe) pinned on cases with a known answer, its negative controls, and
the package's host fp64 chain (niqe_features / niqe_distance, the parameter file, the CPU form) held against it."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import niqe_ref as R


# ---- AGGD ------------------------------------------------------------------------------------------------------------------------------
def _gen_gaussian(alpha, n, rng, scale=1.0):
    """n samples of the generalised Gaussian exp(-(|x| / scale)^alpha): |x| = scale g^(1/alpha), g ~ Gamma(1/alpha)."""
    g = rng.gamma(1.0 / alpha, 1.0, size=n)
    return scale * g ** (1.0 / alpha) * rng.choice([-1.0, 1.0], size=n)


@pytest.mark.parametrize("alpha", [0.8, 2.0, 4.0])
def test_aggd_recovers_the_shape_of_a_generalised_gaussian(alpha):
    """One grid step (0.001) plus sampling error: the estimator's relative standard error at 1e6 samples is below 0.3 % for these shapes
    (delta method on r = E|x|^2 / E x^2), so 1.5 % of alpha is five standard errors."""
    x = _gen_gaussian(alpha, 10 ** 6, np.random.RandomState(int(alpha * 10)))
    a, bl, br = R.estimate_aggd(x)
    assert abs(a - alpha) <= 0.001 + 0.015 * alpha, (a, alpha)
    assert abs(bl - br) <= 0.01 * (bl + br)


def test_aggd_recovers_two_different_sides():
    rng = np.random.RandomState(7)
    n = 10 ** 6
    left, right = -np.abs(_gen_gaussian(2.0, n, rng, 1.0)), np.abs(_gen_gaussian(2.0, n, rng, 3.0))
    # an AGGD with beta_l = 1, beta_r = 3 draws the sides with probabilities beta / (beta_l + beta_r)
    x = np.concatenate([left[:n // 4], right[:3 * n // 4]])
    a, bl, br = R.estimate_aggd(x)
    assert abs(a - 2.0) <= 0.05 and abs(bl - 1.0) <= 0.03 and abs(br - 3.0) <= 0.09, (a, bl, br)


def test_mscn_of_gaussian_noise_is_gaussian():
    """In the limit of noise that is small against the constant 1 of the denominator, m is a linear filter of the noise (the divisor
    is 1 + O(0.05) here): Gaussian, alpha = 2 within three standard errors of 36864 correlated samples (3 x 0.03).  Strong noise is
    divided by its own local deviation -- an estimate from about 17 effective samples that contains the pixel itself -- which bounds m
    and lightens the tails: alpha is about 3 there (printed, not asserted)."""
    z = np.random.RandomState(3).standard_normal((192, 192))
    a, _, _ = R.estimate_aggd(R.mscn_naive(128.0 + 0.05 * z, R.window())[0])
    print("alpha at sigma 0.05:", a, "at sigma 40:", R.estimate_aggd(R.mscn_naive(128.0 + 40.0 * z, R.window())[0])[0])
    assert abs(a - 2.0) <= 0.1, a


# ---- half size -------------------------------------------------------------------------------------------------------------------------
def test_half_size_filter_is_torchs_antialiased_bicubic_in_the_interior_and_symmetric_at_the_border():
    p = np.random.RandomState(0).randint(0, 256, size=(40, 56)).astype(np.float64)
    got = R.half_ref(p)
    t = F.interpolate(torch.from_numpy(p)[None, None], scale_factor=0.5, mode="bicubic", antialias=True, align_corners=False)[0, 0].numpy()
    assert got.shape == t.shape == (20, 28)
    assert np.array_equal(got[2:-2, 2:-2], t[2:-2, 2:-2])          # exact: integers times 2^-16 in fp64 on both sides
    assert not np.array_equal(got, t)                               # the border rule differs (PIL's renormalised taps in torch)
    pad = np.pad(p, 3, mode="symmetric")                            # the explicit padded form
    want = np.zeros((20, 28))
    for i in range(20):
        for j in range(28):
            want[i, j] = R.TAPS @ pad[2 * i:2 * i + 8, 2 * j:2 * j + 8] @ R.TAPS
    assert np.array_equal(got, want)


def test_centred_form_equals_the_naive_form_in_fp64():
    v = np.rint(np.random.RandomState(1).rand(48, 48) * 255)
    m0, s0 = R.mscn_naive(v, R.window())
    m1, s1, *_ = R.mscn_centred(v, R.window())
    assert np.abs(m0 - m1).max() <= 1e-9 and np.abs(s0 - s1).max() <= 1e-8


# ---- the score orders images ---------------------------------------------------------------------------------------------------------------
def test_score_orders_clean_noised_and_blurred_images():
    s = R.suite()["scores"]
    print({k: round(v, 2) for k, v in s.items()})
    assert s["clean"] < s["noise10"] < s["noise25"] < s["noise50"]
    assert s["clean"] < s["blur0.8"] < s["blur1.5"] < s["blur3"]


CONTROLS = {"roll_wraps": False, "last_shift": (1, 1), "border_mode": "reflect"}


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_control_moves_the_score(name):
    S = R.suite()
    x = S["images"]["noise10"]
    changed = R.score(x, S["mu"], S["cov"], opt=dataclasses.replace(R.Opt(), **{name: CONTROLS[name]}))[0]
    assert abs(changed - S["scores"]["noise10"]) > 1e-6 * S["scores"]["noise10"], (name, changed, S["scores"]["noise10"])


def _rgb_case():
    """fp32 [1, 3, 200, 296] in [0, 1]: three different pink planes, so that the luma has fractional parts."""
    planes = [np.pad(R.pink_image(s), ((0, 0), (0, 8)), mode="edge")[:200] for s in (11, 12, 13)]
    return (np.stack(planes)[None] / 255.0).astype(np.float32)


def test_negative_controls_luma_rounding_and_border_crop_move_the_score():
    S = R.suite()
    x = _rgb_case()
    base = R.score(x, S["mu"], S["cov"], border=4)[0]
    unrounded = R.score(x, S["mu"], S["cov"], border=4, opt=R.Opt(round_luma=False))[0]
    uncropped = R.score(x, S["mu"], S["cov"], border=4, opt=R.Opt(crop=False))[0]
    assert abs(unrounded - base) > 1e-9 * base and abs(uncropped - base) > 1e-6 * base, (base, unrounded, uncropped)


def test_negative_control_a_nan_row_counted_into_the_mean():
    S = R.suite()
    rows, _ = R.plane_rows(R.plane_f32(S["images"]["clean"], 0, 96)[0], R.window(), 96)
    rows = rows.copy()
    rows[0, 5] = np.nan
    good = R.distance(rows, S["mu"], S["cov"])
    bad = R.distance(rows, S["mu"], S["cov"], opt=R.Opt(nan_rows_in_mean=True))
    assert np.isfinite(good) and not np.isfinite(bad)


# ---- the package's host chain ------------------------------------------------------------------------------------------------------------
def _ref_moments(m, bs):
    """fp64 block moments [nb, 5, 5] of one fp64 map, the layout of srk_niqe_moments_f32."""
    nbh, nbw = m.shape[0] // bs, m.shape[1] // bs
    out = np.zeros((nbh * nbw, 5, 5))
    for i in range(nbh):
        for j in range(nbw):
            blk = m[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs]
            for k, p in enumerate([blk] + [blk * np.roll(blk, s, axis=(0, 1)) for s in R.SHIFTS]):
                out[i * nbw + j, k] = [(p < 0).sum(), (p[p < 0] ** 2).sum(), (p > 0).sum(), (p[p > 0] ** 2).sum(), np.abs(p).sum()]
    return out


def test_package_features_and_distance_equal_the_restatement_on_its_own_moments():
    from tpu_superresolution_amd import metrics
    S = R.suite()
    plane = R.plane_f32(S["images"]["noise25"], 0, 96)[0]
    rows_ref, _ = R.plane_rows(plane, R.window(), 96)
    m1, _ = R.mscn_naive(plane, R.window())
    m2, _ = R.mscn_naive(R.half_ref(plane), R.window())
    got = np.concatenate([metrics.niqe_features(_ref_moments(m1, 96), 96 * 96), metrics.niqe_features(_ref_moments(m2, 48), 48 * 48)], axis=1)
    assert got.shape == rows_ref.shape == (9, 36)
    assert np.abs(got - rows_ref).max() <= 1e-12 * max(1.0, np.abs(rows_ref).max())
    d_ref, d_got = R.distance(rows_ref, S["mu"], S["cov"]), metrics.niqe_distance(rows_ref, S["mu"], S["cov"])
    assert abs(d_ref - d_got) <= 1e-12 * d_ref


def test_package_features_give_nan_for_an_empty_side_and_distance_needs_two_rows():
    from tpu_superresolution_amd import metrics
    mom = np.zeros((1, 5, 5))
    mom[0, :, 2:] = [50.0, 10.0, 20.0]          # nothing below zero
    assert np.isnan(metrics.niqe_features(mom, 100)).any()
    with pytest.raises(ValueError, match="at least 2"):
        metrics.niqe_distance(np.full((3, 36), np.nan), np.zeros(36), np.eye(36))


def test_cpu_form_scores_within_the_fp32_map_of_the_restatement():
    """The CPU form holds the MSCN maps in fp32 (as the device does): scores agree with the fp64 restatement far inside the 5e-3 the
    feature is built for."""
    from tpu_superresolution_amd import metrics
    S = R.suite()
    for name in ("clean", "noise25", "blur1.5"):
        got = float(metrics.niqe(torch.from_numpy(S["images"][name]), (S["mu"], S["cov"], R.window()))[0])
        assert abs(got - S["scores"][name]) <= 5e-3, (name, got, S["scores"][name])


def test_cpu_fit_equals_the_restatements_fit():
    from tpu_superresolution_amd import metrics
    S = R.suite()
    mu, cov = metrics.niqe_fit([torch.from_numpy(R.as_batch(R.pink_image(s))) for s in range(6)])
    assert np.abs(mu - S["mu"]).max() <= 2e-3 * np.abs(S["mu"]).max() and np.abs(cov - S["cov"]).max() <= 2e-2 * np.abs(S["cov"]).max()


def test_parameter_file_round_trips_and_bad_files_are_refused(tmp_path):
    from tpu_superresolution_amd import metrics
    S = R.suite()
    path = tmp_path / "p.npz"
    metrics.save_niqe_params(path, S["mu"], S["cov"], R.window())
    with np.load(path) as f:
        assert sorted(f.files) == ["cov_pris_param", "gaussian_window", "mu_pris_param"]
        assert f["mu_pris_param"].shape == (1, 36) and f["cov_pris_param"].shape == (36, 36) and f["gaussian_window"].shape == (7, 7)
    p = metrics.load_niqe_params(path)
    assert np.array_equal(p["mu"], S["mu"]) and np.array_equal(p["cov"], S["cov"]) and np.array_equal(p["window"], R.window())
    np.savez(tmp_path / "nokey.npz", mu_pris_param=np.zeros((1, 36)))
    with pytest.raises(ValueError, match="lacks"):
        metrics.load_niqe_params(tmp_path / "nokey.npz")
    for name, kw, msg in (("shape", dict(mu=np.zeros((1, 35))), "expected"), ("nan", dict(cov=np.full((36, 36), np.nan)), "non-finite"),
                          ("asym", dict(cov=np.triu(np.ones((36, 36)))), "symmetric")):
        full = dict(mu=np.zeros((1, 36)), cov=np.eye(36), win=R.window())
        full.update(kw)
        np.savez(tmp_path / f"{name}.npz", mu_pris_param=full["mu"], cov_pris_param=full["cov"], gaussian_window=full["win"])
        with pytest.raises(ValueError, match=msg):
            metrics.load_niqe_params(tmp_path / f"{name}.npz")
    (tmp_path / "junk.npz").write_bytes(b"not an archive")
    with pytest.raises(ValueError, match="cannot be read"):
        metrics.load_niqe_params(tmp_path / "junk.npz")
