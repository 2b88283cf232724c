"""The host logic of the 2-D blur (sr_datasets.PsfSpec, DeviceHRPool(psf=), blur_kernels' table rule and file loader, ops.pack_psf, the
--blur_kernel / --blur_psf / --blur_theta command lines).  No GPU."""
import math
import random

import numpy as np
import pytest

from tpu_superresolution_amd import blur_kernels as bk
from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool, PsfSpec, SynthLRBatches


class CountingRandom(random.Random):
    """Counts the variates a draw takes."""
    calls = 0

    def random(self):
        self.calls += 1
        return super().random()


def _psf_file(tmp_path, tables, name="psf.npy"):
    path = str(tmp_path / name)
    np.save(path, np.asarray(tables))
    return path


def test_psf_spec_validation():
    spec = PsfSpec()
    assert (spec.mode, spec.kernel_prob, spec.beta_g, spec.beta_p, spec.ksize, spec.file, spec.seed) == \
        ("rotated", (0.45, 0.25, 0.12, 0.03, 0.12, 0.03), (0.5, 4.0), (1.0, 2.0), (7, 21), None, 0)
    assert spec.fixed() is None and spec.tables is None
    for bad in (dict(mode="axis"), dict(mode="mixed", kernel_prob=(0.5, 0.5)), dict(mode="mixed", kernel_prob=(0.5, 0.5, 0.1, 0, 0, 0)),
                dict(mode="mixed", kernel_prob=(1.5, -0.5, 0, 0, 0, 0)), dict(mode="mixed", beta_g=(0.0, 1.0)), dict(mode="mixed", beta_g=(2.0, 1.0)),
                dict(mode="mixed", beta_p=(1.0, float("nan"))), dict(mode="mixed", beta_p=(1.0,)), dict(mode="mixed", ksize=(6, 21)),
                dict(mode="mixed", ksize=(7, 23)), dict(mode="mixed", ksize=(9, 7)), dict(mode="mixed", ksize=(7.5, 9)), dict(mode="file"),
                dict(mode="rotated", file="x.npy")):
        with pytest.raises(ValueError):
            PsfSpec(**bad)
    with pytest.raises(ValueError):
        DeviceHRPool([np.zeros((40, 40), np.uint8)], 8, 2, device="cpu", psf=PsfSpec())                          # needs degrade=
    with pytest.raises(ValueError):
        DeviceHRPool([np.zeros((40, 40), np.uint8)], 8, 2, device="cpu", degrade=DegradeSpec(), psf="rotated")
    with pytest.raises(ValueError):
        SynthLRBatches([], 2, 8, "cpu", psf=bk.gaussian(5, 1.0, 1.0))                                            # needs degrade=


@pytest.mark.parametrize("mode", ["rotated", "mixed", "file"])
def test_psf_spec_draws_a_fixed_number_of_variates(mode, tmp_path):
    file = _psf_file(tmp_path, [bk.gaussian(5, 1.0, 2.0, 0.3), bk.plateau(5, 2.0, 1.0, 0.1, 1.5), bk.gaussian(5, 0.7, 0.7)]) if mode == "file" else None
    spec = PsfSpec(mode=mode, file=file, seed=4)
    assert spec.rng(3).random() == random.Random("psf:7").random() and spec.rng(0).random() != DegradeSpec(seed=4).rng(0).random()
    rng = CountingRandom("x")
    seen = set()
    for i in range(200):
        before = rng.calls
        K = spec.draw(rng, (0.2 + 0.01 * i, 2.3 - 0.01 * i) if i % 3 else (0.0, 0.0))
        assert rng.calls - before == 6
        bk.check_table(K)
        assert K.dtype == np.float32
        seen.add(K.shape[0])
    if mode == "rotated":
        assert seen <= set(range(1, 22, 2)) and max(seen) == 2 * math.ceil(3 * 2.29) + 1
        K = spec.draw(rng, (0.0, 0.0))
        assert K.shape == (1, 1) and K[0, 0] == 1.0                                   # no blur at all: the 1 x 1 delta
        assert spec.draw(rng, (2.5, 2.5)).shape == (17, 17) and spec.draw(rng, (2.5, 0.1)).shape == (17, 17)          # the separable path's support
    elif mode == "mixed":
        assert seen == {7, 9, 11, 13, 15, 17, 19, 21}
        only = PsfSpec(mode="mixed", kernel_prob=(0, 0, 0, 0, 1, 0), ksize=(9, 9), beta_p=(1.5, 1.5))
        K = only.draw(random.Random(1), (2.0, 1.0))                                   # plateau iso: s2 = s1, so theta is moot
        assert K.shape == (9, 9) and np.abs(K.astype(np.float64) - bk.plateau(9, 1.0, 1.0, 0.0, 1.5)).max() < 1e-7
    else:
        assert seen == {5} and np.array_equal(spec.fixed(), bk.gaussian(5, 1.0, 2.0, 0.3)) and spec.tables.shape == (3, 5, 5)
        picks = {spec.draw(rng, (1.0, 1.0)).tobytes() for _ in range(100)}
        assert len(picks) == 3


def test_rotated_at_theta_0_is_the_separable_gaussian():
    import degrade_ref as D

    class Zero(random.Random):
        def random(self):
            return 0.5                                                               # theta = pi (0.5 - 0.5) = 0

    sy, sx = D.f32(1.7), D.f32(1.9)
    K = PsfSpec().draw(Zero(), (sy, sx))
    want = np.outer(D.gauss(sy), D.gauss(sx))
    assert K.shape == (13, 13) and np.abs(K.astype(np.float64) - want).max() <= 2.0 ** -23 * want.max()


def test_pool_and_spec_draws_are_the_same_with_and_without_a_psf_spec():
    rng = np.random.RandomState(1)
    hrs = [rng.randint(0, 256, (37, 45)).astype(np.uint8), rng.randint(0, 256, (40, 32, 3)).astype(np.uint8),
           rng.randint(0, 65536, (33, 33)).astype(np.uint16)]
    spec = DegradeSpec(seed=5)
    blind = DeviceHRPool(hrs, 8, 2, device="cpu", augment="d4", degrade=spec, rank=1)
    psf = DeviceHRPool(hrs, 8, 2, device="cpu", augment="d4", degrade=spec, rank=1, psf=PsfSpec(mode="mixed", seed=5))
    batch = [0, 1, 2, 1, 0]
    for _ in range(3):
        random.seed(3)
        want = blind.draw(batch)
        state = random.getstate()
        random.seed(3)
        got = psf.draw(batch)
        assert got == want and random.getstate() == state
        rows = blind.draw_degrade(want[0])
        rows2, tabs, ks = psf.draw_psf(got[0])
        assert rows2 == rows and random.getstate() == state          # the DegradeSpec's sequence, the global `random` untouched
        assert tabs.shape == (5, ks, ks) and tabs.dtype == np.float32 and ks in range(7, 22, 2)
        assert blind._degrade_rng.getstate() == psf._degrade_rng.getstate()
    # a DegradeSpec's own draws do not depend on what a PsfSpec took in between
    a, b = spec.rng(0), spec.rng(0)
    p = PsfSpec(seed=5)
    pr = p.rng(0)
    for _ in range(5):
        da = spec.draw(a, True)
        p.draw(pr, da[0])
        assert da == spec.draw(b, True)


def test_pack_psf_pads_to_the_common_size_and_applies_the_host_rule():
    from tpu_superresolution_amd.ops import pack_psf
    a, b = bk.gaussian(3, 0.8, 0.5, 0.2), bk.plateau(7, 2.0, 1.0, 0.4, 1.2)
    tabs, ks = pack_psf([a, b], 2)
    assert ks == 7 and tabs.shape == (2, 7, 7) and np.array_equal(tabs[0], bk.pad_to(a, 7)) and np.array_equal(tabs[1], b)
    tabs, ks = pack_psf(a, 3)
    assert ks == 3 and tabs.shape == (3, 3, 3) and all(np.array_equal(t, a) for t in tabs)
    assert pack_psf(np.stack([b, b]), 2)[1] == 7
    with pytest.raises(ValueError):
        pack_psf([a, b], 3)


def test_table_rule_and_psf_files(tmp_path):
    good = bk.gaussian(5, 1.0, 2.0, 0.3)
    assert np.array_equal(bk.check_table(good), good)
    one = bk.load_psf_file(_psf_file(tmp_path, good))
    many = bk.load_psf_file(_psf_file(tmp_path, [good, good[::-1].copy()], "n.npy"))
    assert one.shape == (1, 5, 5) and many.shape == (2, 5, 5) and one.dtype == np.float32 and np.array_equal(many[0], good)
    assert bk.load_psf_file(_psf_file(tmp_path, good.astype(np.float64), "f64.npy")).dtype == np.float32
    neg = good.copy()
    neg[0, 0] = -1e-6
    zero_centre = good.copy()
    zero_centre[2, 2] = 0.0
    zero_centre /= zero_centre.sum()
    nan = good.copy()
    nan[1, 1] = np.nan
    bad = {"negative tap": neg, "zero centre": zero_centre, "even size": np.full((4, 4), 1 / 16), "ks > 21": np.full((23, 23), 1 / 529),
           "not square": np.full((3, 5), 1 / 15), "sum": good * 1.01, "nan": nan, "rank": np.full((2, 2, 3, 3), 1 / 9), "empty": np.zeros((0, 3, 3))}
    for what, t in bad.items():
        with pytest.raises(ValueError):
            bk.load_psf_file(_psf_file(tmp_path, t, "bad.npy"))
        if np.ndim(t) == 2:
            with pytest.raises(ValueError):
                bk.check_table(t)
    with pytest.raises(ValueError):
        bk.load_psf_file(_psf_file(tmp_path, [good, neg], "second_bad.npy"))          # every table of the file is checked
    assert abs(float(bk.check_table(good * 1.0009).sum()) - 1.0009) < 1e-6            # within 1e-3 of 1 passes
    for args in ((4, 1.0, 1.0), (23, 1.0, 1.0), (5, 0.0, 1.0), (5, 1.0, float("nan")), (5, 1.0, 1.0, float("inf"))):
        with pytest.raises(ValueError):
            bk.gaussian(*args)
    with pytest.raises(ValueError):
        bk.plateau(5, 1.0, 1.0, 0.0, 0.0)


def test_argparse_finetune(tmp_path, capsys):
    from tpu_superresolution_amd import finetune_swinir as T
    base = ["--data_root", "x", "--scale", "X2"]
    blind = base + ["--gpu_data", "--synth_lr", "--degrade", "blind"]
    a = T.parse_args(blind)
    assert a.blur_kernel == "axis" and T.psf_spec(a) is None
    saved = T.saved_args(a)
    assert not {"blur_kernel", "blur_kernel_prob", "blur_beta_g", "blur_beta_p", "blur_ksize", "blur_psf"} & set(saved) and saved["degrade"] == "blind"
    assert not {"blur_kernel", "blur_psf"} & set(T.saved_args(T.parse_args(base)))
    a = T.parse_args(blind + ["--blur_kernel", "rotated", "--degrade_seed", "9"])
    spec = T.psf_spec(a)
    assert (spec.mode, spec.seed, spec.ksize) == ("rotated", 9, (7, 21)) and T.saved_args(a)["blur_kernel"] == "rotated"
    a = T.parse_args(blind + ["--blur_kernel", "mixed", "--blur_kernel_prob", "0.5", "0.5", "0", "0", "0", "0", "--blur_beta_g", "1", "2",
                              "--blur_beta_p", "1.5", "1.5", "--blur_ksize", "9", "13"])
    spec = T.psf_spec(a)
    assert (spec.mode, spec.kernel_prob, spec.beta_g, spec.beta_p, spec.ksize) == ("mixed", (0.5, 0.5, 0, 0, 0, 0), (1.0, 2.0), (1.5, 1.5), (9, 13))
    assert T.saved_args(a)["blur_ksize"] == [9, 13]
    file = _psf_file(tmp_path, [bk.gaussian(5, 1.0, 2.0, 0.3), bk.gaussian(5, 2.0, 1.0)])
    a = T.parse_args(blind + ["--blur_psf", file])
    assert T.psf_spec(a).mode == "file" and T.psf_spec(a).tables.shape == (2, 5, 5) and T.saved_args(a)["blur_psf"] == file
    even = _psf_file(tmp_path, np.full((4, 4), 1 / 16), "even.npy")
    for bad in (base + ["--blur_kernel", "rotated"], base + ["--gpu_data", "--synth_lr", "--blur_psf", file],
                blind + ["--blur_kernel", "rotated", "--blur_psf", file], blind + ["--blur_ksize", "7", "9"],
                blind + ["--blur_kernel", "rotated", "--blur_beta_g", "1", "2"], blind + ["--blur_kernel", "mixed", "--blur_ksize", "8", "9"],
                blind + ["--blur_kernel", "mixed", "--blur_kernel_prob", "1", "1", "0", "0", "0", "0"], blind + ["--blur_kernel", "diag"],
                blind + ["--blur_psf", even], blind + ["--blur_psf", str(tmp_path / "missing.npy")]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    assert "--blur_psf" in capsys.readouterr().err


def test_argparse_evaluate(tmp_path, capsys):
    from tpu_superresolution_amd import evaluate as E
    ev = ["--scale", "X2", "--ckpt", "c", "--arch", "swinir", "--synth_lr", "--degrade", "blind"]
    a = E.parse_args(ev)
    assert a.blur_theta is None and a.blur_psf is None and E.eval_psf(a) is None
    a = E.parse_args(ev + ["--blur_sigma", "1.7", "0.6", "--blur_theta", "30", "--tile", "24", "--tile_overlap", "8", "--self_ensemble", "--jpeg_quality", "60",
                           "--bench_metric", "y"])
    K = E.eval_psf(a)
    assert K.shape == (13, 13) and np.abs(K.astype(np.float64) - bk.gaussian(13, 0.6, 1.7, math.radians(30))).max() < 1e-7
    assert E.eval_psf(E.parse_args(ev + ["--blur_sigma", "0", "0", "--blur_theta", "10"])).shape == (1, 1)
    file = _psf_file(tmp_path, [bk.gaussian(5, 1.0, 2.0, 0.3), bk.gaussian(5, 2.0, 1.0)])
    assert np.array_equal(E.eval_psf(E.parse_args(ev + ["--blur_psf", file])), bk.gaussian(5, 1.0, 2.0, 0.3))          # table 0
    big = _psf_file(tmp_path, np.full((23, 23), 1 / 529), "big.npy")
    for bad in (["--scale", "X2", "--ckpt", "c", "--arch", "swinir", "--synth_lr", "--blur_theta", "30"],
                ["--scale", "X2", "--ckpt", "c", "--arch", "swinir", "--synth_lr", "--blur_psf", file],
                ev + ["--blur_theta", "30", "--blur_psf", file], ev + ["--blur_theta", "nan"], ev + ["--blur_psf", big],
                ev + ["--blur_psf", str(tmp_path / "missing.npy")]):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    assert "--blur_psf" in capsys.readouterr().err
