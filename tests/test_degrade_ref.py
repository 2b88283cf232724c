"""Pins tests/degrade_ref.py (the fp64 restatement the device tests of the blind degradation compare against): Philox4x32-10 against
known-answer vectors, the statistics of its normals, the composed tables against F.conv2d + F.interpolate(antialias=True) on fp64
tensors, the window property; shows that each defining choice matters; and checks the host logic of --degrade blind.  No GPU."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import degrade_ref as D
import resize_ref as R

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key -> output.  The round function and the constants were compared
# line by line with rocRAND's rocrand_philox4x32_10.h (single_round / bumpkey / ten_rounds), which D.philox_int restates.
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    assert D.philox_int(ctr, key) == want
    assert tuple(int(v) for v in D.philox(*ctr, *key)) == want


def test_philox_array_form_equals_the_integer_form():
    rng = np.random.RandomState(0)
    w = rng.randint(0, 2 ** 32, (200, 6), dtype=np.uint64)
    got = np.stack(D.philox(*(w[:, i] for i in range(6))), axis=1)
    assert all(tuple(int(v) for v in got[n]) == D.philox_int(w[n, :4], w[n, 4:]) for n in range(200))


def test_normal_statistics_and_no_duplicated_draws():
    n_side = 512                                        # N = 2^18
    z, r = D.normal_field(1, 3, 5, n_side, n_side, D.NOISE_ID0, False)
    N = z.size
    print(f"N = {N}: mean = {z.mean():.3e} (limit {5 / np.sqrt(N):.3e}), var - 1 = {z.var() - 1:.3e} (limit {5 * np.sqrt(2 / N):.3e})")
    assert abs(z.mean()) <= 5.0 / np.sqrt(N) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2)) + 1e-12          # u1 >= 2^-24
    # the raw 64 bits behind every draw: distinct across x, y, ch and id
    xs, ys = np.meshgrid(np.arange(64), np.arange(64))
    words = []
    for ch in range(3):
        for nid in (0, 1, 1 << 32, D.NOISE_ID0):
            r0, r1, _, _ = D.philox(xs, ys, ch, 0, nid & D.MASK, nid >> 32)
            words.append((r0 << np.uint64(32) | r1).ravel())
    words = np.concatenate(words)
    assert np.unique(words).size == words.size
    # x and y are not interchangeable, and the id's high word matters
    assert D.normal(1, 2, 0, 7)[0] != D.normal(2, 1, 0, 7)[0] and D.normal(1, 2, 0, 7)[0] != D.normal(1, 2, 0, 7 + (1 << 32))[0]


def test_gauss_and_radius():
    assert [D.radius(s) for s in (0.0, 0.2, 1 / 3, 0.34, 1.7, 2.5)] == [0, 1, 2, 2, 6, 8]          # fp32(1/3) is just above 1/3
    for s in (0.2, 1.7, 2.5):
        g = D.gauss(s)
        assert len(g) == 2 * D.radius(s) + 1 and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    for s in D.SCALES:
        for sigma in (0.3, 1.7, 2.5):
            _, _, ws = D.tables(40 * s, 40, sigma)
            assert max(len(w) for w in ws) <= {2: 8, 3: 12, 4: 16}[s] + 2 * D.radius(sigma) <= 33
            assert all(abs(w.sum() - 1) < 1e-14 for w in ws)
    lo, hi, ws = D.tables(40, 20, 0.0)
    lo0, hi0, ws0 = R.tables(40, 20)
    assert np.array_equal(lo, lo0) and np.array_equal(hi, hi0) and all(np.array_equal(a, b) for a, b in zip(ws, ws0))


@pytest.mark.parametrize("s", D.SCALES)
@pytest.mark.parametrize("sigma", [(0.0, 1.7), (0.3, 2.5), (2.5, 2.5), (1.1, 0.0)], ids=str)
def test_interior_agrees_with_conv2d_then_interpolate_fp64(s, sigma):
    """Away from the border the composed operator is the Gaussian followed by the antialiased bicubic resize.  Both sides are short fp64
    sums: the composed one errs by at most D.bound(u = 2^-53); the sequential one runs a (2 Ry + 1)- and a (2 Rx + 1)-tap pass
    (weights >= 0, sum 1) and then the Kcy- and Kcx-tap cubic passes (sum |w| = Lcy, Lcx): 2 (2 Ry + 2 Rx + 2 + Kcy + Kcx + 8) u Lcy Lcx
    max|x| by the same 2 K u S rule with one extra rounding per weight."""
    H, W = 30 * s, 34 * s
    x = np.random.RandomState(7 * s).rand(1, 2, H, W)
    ry, rx = D.radius(sigma[0]), D.radius(sigma[1])
    t = torch.from_numpy(np.pad(x, ((0, 0), (0, 0), (ry, ry), (rx, rx)), mode="edge"))
    gy, gx = (torch.from_numpy(D.gauss(v)) if D.radius(v) else torch.ones(1, dtype=torch.float64) for v in sigma)
    t = F.conv2d(t.reshape(2, 1, H + 2 * ry, W + 2 * rx), gy.reshape(1, 1, -1, 1))
    t = F.conv2d(t, gx.reshape(1, 1, 1, -1)).reshape(1, 2, H, W)
    seq = F.interpolate(t, size=(H // s, W // s), mode="bicubic", antialias=True, align_corners=False).numpy()
    got = D.filtered(x[0], s, *sigma)
    (loy, hiy, wy), (lox, hix, wx) = R.tables(H, H // s), R.tables(W, W // s)
    iy = np.nonzero((loy - ry >= 0) & (hiy + ry <= H))[0]
    ix = np.nonzero((lox - rx >= 0) & (hix + rx <= W))[0]
    assert len(iy) >= 10 and len(ix) >= 10
    u = 2.0 ** -53
    kc = max(len(w) for w in wy) + max(len(w) for w in wx)
    lc = max(np.abs(w).sum() for w in wy) * max(np.abs(w).sum() for w in wx)
    bnd = D.bound(H, W, s, sigma, 1.0, u=u) + 2.0 * (2 * ry + 2 * rx + 2 + kc + 8) * u * lc
    err = np.abs(got - seq[0])[:, iy[0]:iy[-1] + 1, ix[0]:ix[-1] + 1].max()
    print(f"/{s} sigma {sigma}: max |composed - sequential| = {err:.3e}, bound = {bnd:.3e}")
    assert err <= bnd
    # at the border the two differ (the composed table drops mass outside the image; edge padding keeps it)
    assert np.abs(got - seq[0]).max() > 1e-6


@pytest.mark.parametrize("s", D.SCALES)
def test_patch_is_the_window_of_the_whole_image(s):
    img = D.to_unit3(D.case_image(s, 1))
    P = 16
    for top, left, sigma, noise, nid, gray in D.case_samples(s, 1)[1:]:
        whole, wb = D.degrade(img, s, sigma, noise, nid, gray)
        for tp, lf in ((0, 0), (top // s // 2 * s, left // s // 3 * s), (img.shape[1] // s * s - P * s, img.shape[2] // s * s - P * s)):
            part, pb = D.degrade(img, s, sigma, noise, nid, gray, tp, lf, P)
            assert np.array_equal(part, whole[:, tp // s:tp // s + P, lf // s:lf // s + P])
            assert np.array_equal(pb, wb[:, tp // s:tp // s + P, lf // s:lf // s + P])


def test_negative_controls_fail_their_comparison():
    """Each departure from the semantics is far outside the device tests' bound (a few 1e-6) or moves quantised levels."""
    s, P = 2, 24
    img = D.to_unit3(D.case_image(s, 1))
    sigma, noise, nid = (0.3, 2.5), (0.04, 0.01), 12345
    top, left = 10 * s, 14 * s
    ref, nb = D.degrade(img, s, sigma, noise, nid, False, top, left, P)
    tol = float((D.bound(img.shape[1] // s * s, img.shape[2] // s * s, s, sigma, 1.0) + nb).max())
    # sigma_x and sigma_y swapped
    assert np.abs(D.degrade(img, s, sigma[::-1], noise, nid, False, top, left, P)[0] - ref).max() > 1e3 * tol
    # noise keyed by the coordinates inside the patch
    assert np.abs(D.degrade(img, s, sigma, noise, nid, False, top, left, P, patch_keyed=True)[0] - ref).max() > 1e3 * tol
    # the blur applied to the HR target: the target is the unblurred crop, bit for bit
    hr = img[:, top:top + P * s, left:left + P * s]
    assert np.abs(D.blur(img, *sigma)[:, top:top + P * s, left:left + P * s] - hr).max() > 0.05
    # noise added after the quantisation: not on the 8-bit grid any more, and other levels where it lands on one
    clean = D.filtered(img, s, *sigma, top, left, P)
    z, _ = D.normal_field(3, top // s, left // s, P, P, nid, False)
    late = D.add_noise(D.quant8(clean)[0].astype(np.float64), z, *noise)
    assert np.abs(late * 255 - np.rint(late * 255)).max() > 0.1
    assert (D.quant8(late)[1] != D.quant8(ref)[1]).mean() > 0.05
    # and the blur itself matters
    assert np.abs(D.degrade(img, s, (0.0, 0.0), noise, nid, False, top, left, P)[0] - ref).max() > 1e3 * tol


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("k", range(3), ids=D.SOURCES)
@pytest.mark.parametrize("s", D.SCALES)
def test_skip_cap_of_the_quantised_device_cases(s, k, noisy):
    """At most 1 % of a quantised device case lies so close to a half-integer level that either neighbour must be accepted."""
    ref, bnd = D.case_reference(s, k, noisy)
    share = D.near_half(ref, bnd).reshape(len(ref), -1).mean(axis=1)
    print(f"/{s} {D.SOURCES[k]} {'noisy' if noisy else 'clean'}: near a half-integer per sample = {np.round(100 * share, 3).tolist()} %")
    assert share.max() <= 0.01


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
def test_packing_round_trip_and_ranges():
    from tpu_superresolution_amd.ops import pack_degrade_params
    for sigma, noise, nid, gray in [((0.0, 0.0), (0.0, 0.0), 0, False), ((0.3, 2.5), (0.04, 0.01), D.NOISE_ID0, True),
                                    ((2.5, 0.2), (1.0, 1.0), (1 << 64) - 1, False), ((1.7, 1.7), (10 / 255, 0.0), -5, True)]:
        row = pack_degrade_params(sigma, noise, nid, gray)
        assert row == D.pack(sigma, noise, nid, gray)
        assert all(-(1 << 63) <= v < (1 << 63) for v in row)
        a = np.array(row, dtype=np.int64)          # fits an int64 tensor
        f = a[:2].view(np.float32)
        assert (f[0], f[1], f[2], f[3]) == tuple(np.float32(v) for v in (*sigma, *noise))
        assert int(a[2:3].view(np.uint64)[0]) == nid & 0xFFFFFFFFFFFFFFFF and a[3] == int(gray)
    for bad in [((2.6, 0.0), (0, 0)), ((0.0, -0.1), (0, 0)), ((float("nan"), 0.0), (0, 0)), ((1.0, 1.0), (-1e-3, 0)), ((1.0, 1.0), (0, 1.5)),
                ((1.0, 1.0), (float("inf"), 0))]:
        with pytest.raises(ValueError):
            pack_degrade_params(*bad, 0, False)
    with pytest.raises(ValueError):
        pack_degrade_params((1.0, 1.0), (0, 0), 1 << 64, False)


def test_degrade_spec_draws_from_its_own_generator():
    from tpu_superresolution_amd.sr_datasets import DegradeSpec
    spec = DegradeSpec(blur_sigma=(0.5, 2.5), blur_aniso_p=0.5, noise_sigma=(0.01, 0.05), noise_gain=(0.0, 0.02), gray_noise_p=0.5, seed=3)
    state = random.getstate()
    a, b, other = spec.rng(1), spec.rng(1), spec.rng(2)
    draws = [spec.draw(a, True) for _ in range(400)]
    assert random.getstate() == state
    assert draws == [spec.draw(b, True) for _ in range(400)] and draws[:5] != [spec.draw(other, True) for _ in range(5)]
    sy, sx = np.array([d[0] for d in draws]).T
    assert 0.5 <= sy.min() and sy.max() <= 2.5 and 0.5 <= sx.min() and sx.max() <= 2.5
    assert 0.3 < (sy != sx).mean() < 0.7 and 0.3 < np.mean([d[3] for d in draws]) < 0.7
    assert all(0.01 <= d[1][0] <= 0.05 and 0.0 <= d[1][1] <= 0.02 for d in draws)
    assert len({d[2] for d in draws}) == 400 and max(d[2] for d in draws) >= 1 << 63
    assert all(spec.draw(a, False)[3] for _ in range(20))          # a one-channel source always gets gray noise
    fx = spec.fixed()
    assert fx.blur == (1.5, 1.5) and fx.noise == pytest.approx((0.03, 0.01), abs=1e-15) and fx.gray_noise is True
    assert DegradeSpec(blur_aniso_p=0.0).draw(random.Random(0), True)[0][0] == DegradeSpec(blur_aniso_p=0.0).draw(random.Random(0), True)[0][1]
    for bad in (dict(blur_sigma=(0.0, 2.6)), dict(blur_sigma=(2.0, 1.0)), dict(noise_sigma=(-0.1, 0.1)), dict(noise_gain=(0.0, 2.0)),
                dict(blur_aniso_p=1.5), dict(gray_noise_p=-0.1), dict(blur_sigma=(1.0,)), dict(noise_sigma=(float("nan"), 0.1))):
        with pytest.raises(ValueError):
            DegradeSpec(**bad)


def test_pool_draw_and_global_random_are_the_same_with_and_without_a_spec():
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool
    rng = np.random.RandomState(1)
    hrs = [rng.randint(0, 256, (37, 45)).astype(np.uint8), rng.randint(0, 256, (40, 32, 3)).astype(np.uint8),
           rng.randint(0, 65536, (33, 33)).astype(np.uint16)]
    plain = DeviceHRPool(hrs, 8, 2, device="cpu", augment="d4")
    blind = DeviceHRPool(hrs, 8, 2, device="cpu", augment="d4", degrade=DegradeSpec(seed=5), rank=1)
    batch = [0, 1, 2, 1, 0]
    random.seed(3)
    want = plain.draw(batch)
    state = random.getstate()
    random.seed(3)
    got = blind.draw(batch)
    rows = blind.draw_degrade(got[0])
    assert got == want and random.getstate() == state
    ref_rng = DegradeSpec(seed=5).rng(1)
    for d, row, i in zip(want[0], rows, batch):
        assert row[:6] == d and len(row) == 10
        assert list(row[6:]) == D.pack(*DegradeSpec(seed=5).draw(ref_rng, colour=(i == 1)))
        assert row[9] == 1 or i == 1          # gray sources carry the gray flag
    assert blind.draw_degrade(got[0]) != rows          # the spec's generator moves on; the global one does not
    assert random.getstate() == state
    with pytest.raises(ValueError):
        DeviceHRPool(hrs, 8, 2, device="cpu", degrade=(0.2, 2.0))


def test_argparse_degrade_blind(capsys):
    from tpu_superresolution_amd import evaluate as E
    from tpu_superresolution_amd import finetune_swinir as T
    base = ["--data_root", "x", "--scale", "X2"]
    a = T.parse_args(base)
    assert a.degrade == "bicubic" and T.degrade_spec(a) is None
    a = T.parse_args(base + ["--gpu_data", "--synth_lr", "--degrade", "blind"])
    spec = T.degrade_spec(a)
    assert (spec.blur_sigma, spec.blur_aniso_p, spec.noise_sigma, spec.noise_gain, spec.gray_noise_p, spec.seed) == \
        ((0.2, 2.0), 0.5, (0.0, 10.0 / 255.0), (0.0, 0.0), 0.4, 0)
    a = T.parse_args(base + ["--gpu_data", "--synth_lr", "--degrade", "blind", "--blur_sigma", "0", "2.5", "--blur_aniso_p", "1", "--noise_sigma",
                             "2", "20", "--noise_gain", "0", "0.01", "--gray_noise_p", "0", "--degrade_seed", "9"])
    spec = T.degrade_spec(a)
    assert spec.blur_sigma == (0.0, 2.5) and spec.noise_sigma == (2 / 255.0, 20 / 255.0) and spec.noise_gain == (0.0, 0.01) and spec.seed == 9
    for bad in (["--degrade", "blind"], ["--gpu_data", "--degrade", "blind"], ["--gpu_data", "--synth_lr", "--degrade", "jpeg"],
                ["--gpu_data", "--synth_lr", "--degrade", "blind", "--blur_sigma", "0", "3"],
                ["--gpu_data", "--synth_lr", "--degrade", "blind", "--blur_sigma", "2", "1"],
                ["--gpu_data", "--synth_lr", "--degrade", "blind", "--noise_sigma", "0", "300"],
                ["--gpu_data", "--synth_lr", "--degrade", "blind", "--gray_noise_p", "2"],
                ["--gpu_data", "--synth_lr", "--degrade", "blind", "--blur_sigma", "1"]):
        with pytest.raises(SystemExit):
            T.parse_args(base + bad)
    assert "--synth_lr" in capsys.readouterr().err
    ev = ["--scale", "X2", "--ckpt", "c", "--arch", "swinir"]
    a = E.parse_args(ev + ["--synth_lr", "--degrade", "blind", "--blur_sigma", "0.5", "2.0", "--noise_sigma", "8", "--noise_gain", "0.01"])
    assert a.degrade == "blind" and a.blur_sigma == [0.5, 2.0] and a.noise_sigma == 8.0 and a.noise_gain == 0.01
    assert E.parse_args(ev + ["--synth_lr"]).degrade == "bicubic"
    for bad in (["--degrade", "blind"], ["--synth_lr", "--degrade", "blind", "--blur_sigma", "0", "2.6"],
                ["--synth_lr", "--degrade", "blind", "--noise_sigma", "-1"], ["--synth_lr", "--degrade", "blind", "--noise_gain", "2"]):
        with pytest.raises(SystemExit):
            E.parse_args(ev + bad)


def test_synth_lr_batches_refuses_bad_fixed_parameters():
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, FixedDegrade, SynthLRBatches
    assert SynthLRBatches([], 2, 8, "cpu").degrade is None
    assert SynthLRBatches([], 2, 8, "cpu", degrade=DegradeSpec()).degrade == DegradeSpec().fixed()
    with pytest.raises(ValueError):
        SynthLRBatches([], 2, 8, "cpu", degrade=FixedDegrade((3.0, 1.0), (0.0, 0.0)))
