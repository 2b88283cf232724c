"""CPU pins of tests/jpeg_ref.py (the fp64 restatement of srk_jpeg_roundtrip_f32) and of the host logic of the JPEG stage."""
import io
import random

import numpy as np
import pytest

import jpeg_ref as R

from PIL import Image as PIL_Image  # noqa: E402


def pillow_tables(q):
    buf = io.BytesIO()
    PIL_Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, "JPEG", quality=q)
    buf.seek(0)
    qt = PIL_Image.open(buf).quantization
    return np.array(qt[0]).reshape(8, 8), np.array(qt[1]).reshape(8, 8)


def tables_pin(variant=""):
    for q in range(1, 101):
        want, got = pillow_tables(q), R.tables(q, variant)
        if not (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])):
            return False
    return True


def pillow_decode(lev, q):
    """lev uint8 [C][H][W] -> Pillow's decode of its baseline 4:4:4 file, fp64 [C][H][W]"""
    img = PIL_Image.fromarray(lev[0] if lev.shape[0] == 1 else lev.transpose(1, 2, 0))
    buf = io.BytesIO()
    img.save(buf, "JPEG", quality=q, subsampling=0)
    buf.seek(0)
    a = np.asarray(PIL_Image.open(buf)).astype(np.float64)
    return a[None] if a.ndim == 2 else a.transpose(2, 0, 1)


PIXEL_CASES = [(C, H, W, q) for (C, H, W) in ((1, 72, 72), (3, 72, 72), (1, 61, 45), (3, 61, 45)) for q in (10, 50, 75, 90)]


def pixel_gap_db(C, H, W, q, variant=""):
    """10 log10 of mse(Pillow's decode, source) / mse(reference, Pillow's decode): > 0 = the reference is closer to Pillow's decode
    than the source is, i.e. the same codec up to libjpeg's integer arithmetic."""
    lev = R.smooth_u8(np.random.default_rng(7 * H + C), C, H, W).astype(np.uint8)
    pil = pillow_decode(lev, q)
    ref = R.roundtrip(lev.astype(np.float32) / np.float32(255), q, False, None, variant).out.astype(np.float64) * 255.0
    return 10.0 * np.log10(np.mean((pil - lev) ** 2) / np.mean((ref - pil) ** 2))


def pixels_pin(variant=""):
    return all(pixel_gap_db(C, H, W, q, variant) > 0.0 for C, H, W, q in PIXEL_CASES)


def test_tables_equal_pillows_for_every_quality():
    assert tables_pin()


def test_dct_is_orthonormal_and_a_delta_gives_its_basis_image():
    d = R.dct_matrix64()
    assert np.abs(d @ d.T - np.eye(8)).max() < 8 * 2.0 ** -52
    assert np.abs(R.D - d).max() <= 2.0 ** -25 * 0.5          # rounded once to fp32, |d| <= 1/2
    for u, v in ((0, 0), (1, 0), (0, 1), (3, 5), (7, 7)):
        k = np.zeros((8, 8), np.int64)
        k[u, v] = 1
        c = np.einsum("uy,uv,vx->yx", R.D, k.astype(np.float64), R.D)
        assert np.abs(c - np.outer(d[u], d[v])).max() < 1e-7
        # and through inverse(): Q = 1 everywhere, the block scaled so that the rounding to levels keeps its shape
        vals, _ = R.inverse(k * 400, np.ones((8, 8), np.int64))
        assert np.array_equal(vals, np.clip(np.rint(400 * np.einsum("uy,uv,vx->yx", R.D, k.astype(np.float64), R.D) + 128), 0, 255))


@pytest.mark.parametrize("C,H,W,q", PIXEL_CASES)
def test_reference_is_closer_to_pillows_decode_than_the_source_is(C, H, W, q):
    gap = pixel_gap_db(C, H, W, q)
    print(f"C={C} {H}x{W} q={q}: gap {gap:.1f} dB")
    assert gap > 0.0


def test_420_chroma_equals_444_on_the_half_size_planes():
    rng = np.random.default_rng(3)
    small = R.smooth_u8(rng, 3, 24, 40)
    big = small.repeat(2, axis=1).repeat(2, axis=2)          # uniform 2 x 2 cells, 48 x 80: a whole number of 16 x 16 MCUs
    x = big.astype(np.float32) / np.float32(255)
    for q in (20, 75):
        sub = R.roundtrip(x, q, True)
        ycc_small = R.rgb_to_ycc(*small.astype(np.float32))          # conversion is per pixel: the half-size planes of the same colours
        for i in (1, 2):
            want, _ = R.forward(ycc_small[i].astype(np.float64), R.tables(q)[1])
            assert np.array_equal(sub.coef[i, :24, :40], want)
            assert not sub.coef_valid[i, 24:].any() and not sub.coef_valid[i, :, 40:].any()
        full = R.roundtrip(x, q, False)
        assert np.array_equal(sub.coef[0], full.coef[0])          # Y does not see the subsampling


def test_each_negative_control_breaks_a_pin():
    assert tables_pin() and pixels_pin()
    broken = {v: (not tables_pin(v)) or (not pixels_pin(v)) for v in R.VARIANTS}
    assert all(broken.values()), broken
    assert not tables_pin("transposed_table") and not tables_pin("zigzag_table") and not tables_pin("chroma_table_on_y")
    for v in ("no_level_shift", "swap_cbcr", "anchor_1_0", "zero_pad"):          # the tables cannot see these
        assert tables_pin(v) and not pixels_pin(v)


def test_pass_through_level_and_colour_steps():
    x = np.array([[[np.nan, -1.0, 0.0, 0.5, 1.0, 7.0, 3 / 255, 0.0019607844]]], np.float32)
    assert R.level(x).tolist() == [[[0.0, 0.0, 0.0, 128.0, 255.0, 255.0, 3.0, 0.0]]]          # 127.5 rounds to even
    r = R.roundtrip(x, 0)
    assert np.array_equal(r.out.view(np.uint32), x.view(np.uint32)) and r.pix_decided.all()
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(R.level(k / np.float32(255)), k)
    y, cb, cr = R.rgb_to_ycc(k, k, k)
    assert np.array_equal(y, k) and (cb == 128).all() and (cr == 128).all()          # gray stays gray
    assert all(np.array_equal(c, k) for c in R.ycc_to_rgb(k, np.full(256, 128.0), np.full(256, 128.0)))


@pytest.mark.parametrize("C,H,W,sub", list(R.cases()))
def test_caps_of_the_device_cases(C, H, W, sub):
    """From the reference alone: at most 2 % of a case's coefficients and 1 % of its pixels lie so close to a half-integer that the
    device may round them the other way."""
    x = R.make_batch(C, H, W)
    nc = uc = npx = upx = 0
    for b, q in enumerate(R.QUALITIES):
        if q == 0:
            continue
        r = R.roundtrip(x[b], q, sub)
        nc += int(r.coef_valid.sum())
        uc += int((r.coef_valid & ~r.coef_decided).sum())
        npx += r.pix_decided.size
        upx += int((~r.pix_decided).sum())
    print(f"C={C} {H}x{W} sub={sub}: undecided coefficients {uc}/{nc} = {100.0 * uc / nc:.2f} %, pixels {upx}/{npx} = {100.0 * upx / npx:.2f} %")
    assert uc <= 0.02 * nc and upx <= 0.01 * npx


# ---- host logic ---------------------------------------------------------------------------------------------------------------------

def test_jpeg_spec_ranges_and_draws():
    from tpu_superresolution_amd.sr_datasets import JpegSpec
    for bad in (dict(quality=(0, 50)), dict(quality=(50, 101)), dict(quality=(60, 40)), dict(quality=(50,)), dict(quality=(10.5, 50)),
                dict(quality=50), dict(p=1.5), dict(p=-0.1), dict(p=float("nan")), dict(quality=(True, 50))):
        with pytest.raises(ValueError):
            JpegSpec(**bad)
    spec = JpegSpec(quality=(30, 95), p=0.5, seed=4)
    assert spec.fixed() == round((30 + 95) / 2) and JpegSpec(quality=(40, 40)).fixed() == 40
    state = random.getstate()
    a = [spec.draw(r) for r in [spec.rng(1)] for _ in range(400)]
    assert a == [spec.draw(r) for r in [spec.rng(1)] for _ in range(400)]          # per seed and rank
    assert a != [spec.draw(r) for r in [spec.rng(2)] for _ in range(400)]
    assert a == [JpegSpec(quality=(30, 95), p=0.5, seed=5).draw(r) for r in [JpegSpec(seed=5).rng(0)] for _ in range(400)]          # seed + rank
    assert random.getstate() == state          # the global generator is not touched
    assert set(a) <= {0, *range(30, 96)} and 0 in a and 30 in a and 95 in a and 120 < a.count(0) < 280
    # two variates per draw whatever they decide: the generator ends where two plain draws per sample leave it
    for p in (0.0, 0.5, 1.0):
        s, r, plain = JpegSpec(quality=(1, 100), p=p, seed=0), JpegSpec(seed=0).rng(0), JpegSpec(seed=0).rng(0)
        got = [s.draw(r) for _ in range(50)]
        for _ in range(100):
            plain.random()
        assert r.getstate() == plain.getstate()
        assert (p != 0.0 or set(got) == {0}) and (p != 1.0 or 0 not in got)
    assert JpegSpec(seed=0).rng(0).getstate() != random.Random(0).getstate()          # not the DegradeSpec stream of the same seed


def test_pool_draws_are_the_same_with_and_without_jpeg():
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool, JpegSpec
    rng = np.random.RandomState(1)
    hrs = [rng.randint(0, 256, (37, 45)).astype(np.uint8), rng.randint(0, 256, (40, 32, 3)).astype(np.uint8)]
    batch = [0, 1, 1, 0]
    for degrade in (None, DegradeSpec(seed=5)):
        plain = DeviceHRPool(hrs, 8, 2, device="cpu", augment="d4", degrade=degrade, rank=1)
        with_jpeg = DeviceHRPool(hrs, 8, 2, device="cpu", augment="d4", degrade=degrade, rank=1, jpeg=JpegSpec(quality=(10, 90), seed=5))
        random.seed(3)
        want = plain.draw(batch)
        state = random.getstate()
        random.seed(3)
        got = with_jpeg.draw(batch)
        assert got == want and random.getstate() == state          # HR patches, D4 codes, the global generator
        if degrade is not None:
            assert with_jpeg.draw_degrade(got[0]) == plain.draw_degrade(want[0]) and len(plain.draw_degrade(want[0])[0]) == 10
    for bad in (dict(jpeg=(10, 90)), dict(jpeg=50), dict(jpeg=JpegSpec(), quant_bits=0)):
        with pytest.raises(ValueError):
            DeviceHRPool(hrs, 8, 2, device="cpu", **bad)
    assert DeviceHRPool(hrs, 8, 2, device="cpu").jpeg is None


def test_synth_lr_batches_jpeg_argument():
    from tpu_superresolution_amd.sr_datasets import JpegSpec, SynthLRBatches
    s = SynthLRBatches([], 2, 8, "cpu")
    assert s.jpeg is None and s.jpeg_subsample is False
    s = SynthLRBatches([], 2, 8, "cpu", jpeg=40, jpeg_subsample=True)
    assert (s.jpeg, s.jpeg_subsample) == (40, True)
    s = SynthLRBatches([], 2, 8, "cpu", jpeg=JpegSpec(quality=(30, 95), subsample=True))
    assert (s.jpeg, s.jpeg_subsample) == (62, True)
    for bad in (dict(jpeg=0), dict(jpeg=101), dict(jpeg=50.5), dict(jpeg=(30, 95))):
        with pytest.raises(ValueError):
            SynthLRBatches([], 2, 8, "cpu", **bad)
    with pytest.raises(ValueError):
        SynthLRBatches([], 2, 0, "cpu", jpeg=50)


def test_argparse_jpeg_flags(capsys):
    from tpu_superresolution_amd import evaluate as E
    from tpu_superresolution_amd import finetune_swinir as T
    base = ["--data_root", "x", "--scale", "X2"]
    plain = T.parse_args(base)
    assert plain.jpeg_quality is None and T.jpeg_spec(plain) is None
    assert not {"jpeg_quality", "jpeg_p", "jpeg_subsample"} & set(T.saved_args(plain))          # no trace at the defaults
    on = ["--gpu_data", "--synth_lr"]
    assert not {"jpeg_quality", "jpeg_p", "jpeg_subsample"} & set(T.saved_args(T.parse_args(base + on + ["--degrade", "blind"])))
    a = T.parse_args(base + on + ["--jpeg_quality", "30", "95"])
    spec = T.jpeg_spec(a)
    assert (spec.quality, spec.p, spec.subsample, spec.seed) == ((30, 95), 1.0, False, 0)
    assert T.saved_args(a)["jpeg_quality"] == [30, 95] and not {"jpeg_p", "jpeg_subsample"} & set(T.saved_args(a))
    a = T.parse_args(base + on + ["--degrade", "blind", "--jpeg_quality", "10", "10", "--jpeg_p", "0.25", "--jpeg_subsample", "420",
                                  "--degrade_seed", "9"])
    spec = T.jpeg_spec(a)
    assert (spec.quality, spec.p, spec.subsample, spec.seed) == ((10, 10), 0.25, True, 9) and T.degrade_spec(a).seed == 9
    assert {"jpeg_quality", "jpeg_p", "jpeg_subsample"} <= set(T.saved_args(a))
    assert T.parse_args(base + on + ["--degrade", "bicubic", "--jpeg_quality", "5", "100"]).degrade == "bicubic"
    for bad, word in ((["--jpeg_quality", "30", "95"], "--gpu_data --synth_lr"), (["--gpu_data", "--jpeg_quality", "30", "95"], "--synth_lr"),
                      (on + ["--synth_lr_bits", "0", "--jpeg_quality", "30", "95"], "--synth_lr_bits 8"),
                      (on + ["--jpeg_p", "0.5"], "--jpeg_quality"), (on + ["--jpeg_subsample", "420"], "--jpeg_quality"),
                      (on + ["--jpeg_quality", "0", "95"], "1..100"), (on + ["--jpeg_quality", "30", "101"], "1..100"),
                      (on + ["--jpeg_quality", "95", "30"], "LO <= HI"), (on + ["--jpeg_quality", "30", "95", "--jpeg_p", "1.5"], "probability"),
                      (on + ["--jpeg_quality", "30"], "expected 2 arguments"), (on + ["--jpeg_quality", "30", "95", "--jpeg_subsample", "422"], "422"),
                      (on + ["--degrade", "jpeg"], "jpeg")):
        with pytest.raises(SystemExit):
            T.parse_args(base + bad)
        assert word in capsys.readouterr().err, (bad, word)
    ev = ["--scale", "X2", "--ckpt", "c", "--arch", "swinir"]
    a = E.parse_args(ev + ["--synth_lr"])
    assert a.jpeg_quality is None and a.jpeg_subsample == "444"
    a = E.parse_args(ev + ["--synth_lr", "--jpeg_quality", "40", "--jpeg_subsample", "420", "--tile", "64", "--self_ensemble"])
    assert a.jpeg_quality == 40 and a.jpeg_subsample == "420" and a.tile == 64
    assert E.parse_args(ev + ["--synth_lr", "--degrade", "blind", "--jpeg_quality", "75"]).jpeg_quality == 75
    for bad, word in ((["--jpeg_quality", "40"], "--synth_lr"), (["--synth_lr", "--synth_lr_bits", "0", "--jpeg_quality", "40"], "--synth_lr_bits 8"),
                      (["--synth_lr", "--jpeg_quality", "0"], "1..100"), (["--synth_lr", "--jpeg_quality", "101"], "1..100"),
                      (["--synth_lr", "--jpeg_subsample", "420"], "--jpeg_quality"), (["--synth_lr", "--jpeg_quality", "40", "60"], "unrecognized")):
        with pytest.raises(SystemExit):
            E.parse_args(ev + bad)
        assert word in capsys.readouterr().err, (bad, word)


def test_ops_jpeg_roundtrip_refuses_before_any_launch():
    import torch
    from tpu_superresolution_amd import ops
    assert [ops.check_jpeg_quality(q) for q in (1, 50, 100, 75.0)] == [1, 50, 100, 75]
    for bad in (0, 101, -3, 50.5, True, "50", None, float("nan")):
        with pytest.raises(ValueError):
            ops.check_jpeg_quality(bad)
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip(torch.zeros(1, 3, 8, 8), 50)          # not on the device
