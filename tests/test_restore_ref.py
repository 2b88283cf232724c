"""Pins tests/restore_ref.py, the reference of tests/test_gpu_restore.py (CPU only): the integer luma by known answers, the window
rule by what it equals and what it differs from, and -- from the reference alone -- the cap the device test relies on."""
import numpy as np
import pytest

import degrade_ref as D
import restore_ref as R
from tpu_superresolution_amd import ops


def test_luma_known_answers():
    px = lambda r, g, b, dt=np.uint8: np.array([[[r, g, b]]], dtype=dt)          # noqa: E731
    assert int(R.luma(px(255, 0, 0))[0, 0]) == (4899 * 255 + 8192) >> 14 == 76
    assert int(R.luma(px(0, 255, 0))[0, 0]) == (9617 * 255 + 8192) >> 14 == 150
    assert int(R.luma(px(0, 0, 255))[0, 0]) == (1868 * 255 + 8192) >> 14 == 29
    assert int(R.luma(px(255, 255, 255))[0, 0]) == 255
    assert int(R.luma(px(0, 0, 0))[0, 0]) == 0
    assert int(R.luma(px(65535, 65535, 65535, np.uint16))[0, 0]) == 65535
    assert int(R.luma(px(65535, 0, 0, np.uint16))[0, 0]) == (4899 * 65535 + 8192) >> 14 == 19596
    assert sum(R.LUMA) == 16384 and 16384 * 65535 + 8192 < 2 ** 32
    for k in (0, 2):          # a gray pixel keeps its value: the coefficients sum to 1
        g = np.arange(256 if k == 0 else 65536, dtype=np.uint8 if k == 0 else np.uint16)
        assert np.array_equal(R.luma(np.stack([g, g, g], axis=-1)), g)


def test_to_gray_is_the_reference_luma():
    rng = np.random.default_rng(0)
    for dt, hi in ((np.uint8, 256), (np.uint16, 65536)):
        a = rng.integers(0, hi, (2, 9, 7, 3)).astype(dt)
        assert np.array_equal(ops.to_gray(a), R.luma(a)) and ops.to_gray(a).dtype == dt
    import torch
    t = torch.from_numpy(rng.integers(0, 256, (5, 4, 3)).astype(np.uint8))
    assert ops.to_gray(t).dtype == torch.uint8 and np.array_equal(ops.to_gray(t).numpy(), R.luma(t.numpy()))
    with pytest.raises(ValueError):
        ops.to_gray(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        ops.to_gray(np.zeros((4, 4, 3), np.float32))
    assert not np.array_equal(R.luma(a, "float_luma"), R.luma(a))          # rounded float coefficients are another function


@pytest.mark.parametrize("out_chans,sub", [(3, False), (3, True), (1, False)])
def test_window_rule(out_chans, sub):
    """The window of the whole-image chain equals the chain on an MCU-aligned crop that ends on the grid or on the image's border, and
    differs from the chain on an off-grid crop."""
    a = R.case_image(0)          # 45 x 61 RGB
    nid, q = R.NOISE_ID0, 50
    whole = R.chain(a, out_chans, R.SIGMA, nid, False, q, sub, 8)
    assert whole.shape == (out_chans, 45, 61)
    for top, left, P in ((16, 32, 16), (0, 16, 32)):
        win = R.chain(a, out_chans, R.SIGMA, nid, False, q, sub, 8, window=(top, left, P))
        assert np.array_equal(win, whole[:, top:top + P, left:left + P])
        assert np.array_equal(win, R.chain(a, out_chans, R.SIGMA, nid, False, q, sub, 8, "patch_blocks", (top, left, P)))
    off = (3, 5, 32)
    win = R.chain(a, out_chans, R.SIGMA, nid, False, q, sub, 8, window=off)
    assert not np.array_equal(win, R.chain(a, out_chans, R.SIGMA, nid, False, q, sub, 8, "patch_blocks", off))


def test_negative_controls():
    a, nid = R.case_image(0), R.NOISE_ID0
    w = (13, 29, 32)          # the far corner of the ragged 45 x 61 image: the replicated edge is inside the last blocks
    good = R.chain(a, 3, R.SIGMA, nid, False, 50, True, 8, window=w)
    assert not np.array_equal(good, R.chain(a, 3, R.SIGMA, nid, False, 50, True, 8, "patch_blocks", w))
    assert not np.array_equal(good, R.chain(a, 3, R.SIGMA, nid, False, 50, True, 8, "zero_pad", w))
    assert not np.array_equal(good, R.chain(a, 3, R.SIGMA, nid, False, 50, True, 8, "noise_after_jpeg", w))
    assert np.array_equal(R.chain(a, 3, 0.0, nid, False, 50, True, 8, "noise_after_jpeg", w), R.chain(a, 3, 0.0, nid, False, 50, True, 8, window=w))
    # noise keyed on patch coordinates, without a JPEG stage so that nothing else differs; at (0, 0) the two keys coincide
    plain = R.chain(a, 3, R.SIGMA, nid, False, 0, False, 0, window=w)
    assert not np.array_equal(plain, R.chain(a, 3, R.SIGMA, nid, False, 0, False, 0, "patch_noise", w))
    assert np.array_equal(R.chain(a, 3, R.SIGMA, nid, False, 0, False, 0, window=(0, 0, 32)),
                          R.chain(a, 3, R.SIGMA, nid, False, 0, False, 0, "patch_noise", (0, 0, 32)))
    g1 = R.chain(a, 1, 0.0, nid, True, 0, window=w)
    assert not np.array_equal(g1, R.chain(a, 1, 0.0, nid, True, 0, variant="float_luma", window=w))
    # gray noise is one draw for the three channels; colour noise is three
    d = R.chain(a, 3, R.SIGMA, nid, True, 0) - R.convert(a, 3)
    assert np.allclose(d[0], d[1], atol=1e-6) and np.allclose(d[0], d[2], atol=1e-6)
    d = R.chain(a, 3, R.SIGMA, nid, False, 0) - R.convert(a, 3)
    assert not np.allclose(d[0], d[1], atol=1e-3)


def test_noise_is_the_degrade_reference():
    """`noised` adds exactly degrade_ref's draw for the pixel's image coordinates, and nothing at sigma 0."""
    x = R.convert(R.case_image(1), 1)
    v, b = R.noised(x, R.SIGMA, 5, True)
    z, _ = D.normal(np.array(7), np.array(3), 0, 5)
    assert v[0, 3, 7] == x[0, 3, 7] + np.sqrt(D.f32(R.SIGMA) ** 2) * z
    sub, _ = R.noised(x[:, 3:9, 7:20], R.SIGMA, 5, True, 3, 7)
    assert np.array_equal(sub, v[:, 3:9, 7:20])
    v0, b0 = R.noised(x, 0.0, 5, True)
    assert np.array_equal(v0, x) and not b0.any() and (b > 0).all()


@pytest.mark.parametrize("k", range(len(R.SOURCES)))
@pytest.mark.parametrize("out_chans", [1, 3])
def test_quantised_noise_cap(k, out_chans):
    """What tests/test_gpu_restore.py relies on for its quantised noise cases: at most 1 % of a sample's pixels lie within the noise
    bound of a half-integer level (there either neighbouring level passes)."""
    for gray in (False, True):
        v, b = R.noise_reference(k, out_chans, gray)
        share = D.near_half(v, b).reshape(len(v), -1).mean(axis=1)
        print(f"image {k} out_chans {out_chans} gray {gray}: near a half-integer per sample {np.round(100 * share, 4).tolist()} %, "
              f"largest bound {b.max():.3e}")
        assert share.max() <= 0.01
