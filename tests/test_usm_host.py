"""Host logic of the USM target and the resize rules: the taps, the specs' refusals, the mode generator next to the
23-variate stream, the trailing field of ops.SecondOrder, and the command lines.  No GPU."""
import random

import numpy as np
import pytest

TRAIN = ["--data_root", "D", "--scale", "X2"]
ON = TRAIN + ["--gpu_data", "--synth_lr", "--degrade", "second_order"]


def test_gaussian1d_is_the_closed_form():
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd import ops
    for ks, sigma in ((51, 8.0), (3, 0.8), (1, 1.0), (21, 2.5)):
        r = ks // 2
        d = np.arange(-r, r + 1, dtype=np.float64)
        e = np.exp(-d * d / (2.0 * sigma * sigma))
        k = bk.gaussian1d(ks, sigma)
        assert k.dtype == np.float32 and k.shape == (ks,) and np.array_equal(k, (e / e.sum()).astype(np.float32))
        assert np.array_equal(k, k[::-1]) and abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6
    assert bk.gaussian1d(1, 3.0)[0] == 1.0
    for bad in ((0, 1.0), (2, 1.0), (53, 1.0), (True, 1.0), (5, 0.0), (5, -1.0), (5, float("nan")), (5, float("inf"))):
        with pytest.raises(ValueError):
            bk.gaussian1d(*bad)
    assert [ops.usm_ks(r) for r in (50, 51, 1, 2, 3)] == [51, 51, 1, 3, 3]
    for bad in (0, 52, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            ops.usm_ks(bad)


def test_usm_spec_refusals():
    from tpu_superresolution_amd.sr_datasets import UsmSpec
    s = UsmSpec()
    assert (s.radius, s.sigma, s.weight, s.threshold, s.ks) == (50, 0.0, 0.5, 10.0, 51)
    assert UsmSpec(radius=3, weight=1, threshold=0).ks == 3
    for bad in (dict(radius=0), dict(radius=52), dict(radius=2.5), dict(weight=-0.1), dict(weight=11), dict(weight=float("nan")),
                dict(threshold=-1), dict(threshold=256), dict(threshold=float("nan")), dict(sigma=float("nan")), dict(sigma=101),
                dict(sigma=float("-inf")), dict(weight="x")):
        with pytest.raises(ValueError):
            UsmSpec(**bad)


def test_resize_mode_prob_refusals():
    from tpu_superresolution_amd.sr_datasets import SecondOrderSpec
    assert SecondOrderSpec().resize_mode_prob == (0.0, 0.0, 1.0)
    assert SecondOrderSpec(resize_mode_prob=[0.3, 0.3, 0.4]).resize_mode_prob == (0.3, 0.3, 0.4)
    for bad in ((0.5, 0.6, 0.1), (1.0, 0.0), (-0.1, 0.6, 0.5), (float("nan"), 0.5, 0.5), "abc", None, (0.2, 0.2, 0.2)):
        with pytest.raises(ValueError, match="resize_mode_prob"):
            SecondOrderSpec(resize_mode_prob=bad)


def test_mode_generator_leaves_the_23_variate_stream():
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd.sr_datasets import SECOND_ORDER_VARIATES, SecondOrderSpec
    assert SECOND_ORDER_VARIATES == 23
    a, b = SecondOrderSpec(seed=5), SecondOrderSpec(seed=5, resize_mode_prob=(0.3, 0.3, 0.4))
    ra, rb, ma, mb = a.rng(1), b.rng(1), a.mode_rng(1), b.mode_rng(1)
    t1 = bk.gaussian(7, 1.0, 2.0, 0.3)
    seen = set()
    for i in range(64):
        pa = a.draw(ra, t1, (0.01, 0.0), i, False, True, 96, 2, mode_rng=ma)
        pb = b.draw(rb, t1, (0.01, 0.0), i, False, True, 96, 2, mode_rng=mb)
        po = b.draw(SecondOrderSpec(seed=5).rng(1), t1, (0.01, 0.0), i, False, True, 96, 2) if i == 0 else None
        assert pa.modes == (0, 0, 0) and len(pb.modes) == 3 and set(pb.modes) <= {0, 1, 2}
        seen |= set(pb.modes)
        for f in pa._fields:
            if f == "modes":
                continue
            va, vb = getattr(pa, f), getattr(pb, f)
            assert np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb, f"draw {i}: field {f} moved with resize_mode_prob"
        if po is not None:
            assert po.modes == (0, 0, 0)          # no mode generator: the cubic
    assert seen == {0, 1, 2}
    assert ra.getstate() == rb.getstate() == _advanced(a.rng(1), 64 * 23).getstate()
    assert ma.getstate() == mb.getstate() == _advanced(a.mode_rng(1), 64 * 3).getstate()
    # the order is AREA BILINEAR BICUBIC
    assert SecondOrderSpec(resize_mode_prob=(1, 0, 0)).draw_modes(random.Random(0)) == (2, 2, 2)
    assert SecondOrderSpec(resize_mode_prob=(0, 1, 0)).draw_modes(random.Random(0)) == (1, 1, 1)
    assert SecondOrderSpec(resize_mode_prob=(0, 0, 1)).draw_modes(random.Random(0)) == (0, 0, 0)
    fx = b.fixed(t1, (0.01, 0.0))
    assert fx.modes == (0, 0, 0)


def _advanced(rng, n):
    for _ in range(n):
        rng.random()
    return rng


def test_second_order_keeps_its_13_positional_fields():
    from tpu_superresolution_amd.ops import SecondOrder
    p = SecondOrder("k1", 1.0, (0.0, 0.0), False, 50, "k2", 1.0, (0.0, 0.0), False, 60, False, "k3", 7)
    assert p.modes == (0, 0, 0) and p.noise_id == 7 and len(p) == 14
    assert SecondOrder(*p[:13], (2, 1, 0)).modes == (2, 1, 0)


def test_finetune_flags_map_and_stay_out_of_saved_args():
    from tpu_superresolution_amd import finetune_swinir as F
    from tpu_superresolution_amd.sr_datasets import UsmSpec
    plain = F.saved_args(F.parse_args(ON))
    assert not [k for k in ("gt_usm", "usm_radius", "usm_weight", "usm_threshold", "resize_mode_prob") if k in plain]
    assert F.usm_spec(F.parse_args(ON)) is None and F.second_order_spec(F.parse_args(ON)).resize_mode_prob == (0.0, 0.0, 1.0)
    a = F.parse_args(ON + ["--gt_usm", "--resize_mode_prob", "0.3", "0.3", "0.4", "--arch", "hat", "--graph", "--ema_decay", "0.999", "--augment", "d4",
                           "--loss", "mse", "--val_tile", "64", "--degrade_tables", "device", "--degrade_margin", "25"])
    assert F.usm_spec(a) == UsmSpec() and F.second_order_spec(a).resize_mode_prob == (0.3, 0.3, 0.4)
    on = F.saved_args(a)
    assert on["gt_usm"] is True and on["resize_mode_prob"] == [0.3, 0.3, 0.4] and "usm_weight" not in on
    b = F.parse_args(ON + ["--gt_usm", "--usm_weight", "0.8", "--usm_threshold", "4", "--usm_radius", "21"])
    assert F.usm_spec(b) == UsmSpec(radius=21, weight=0.8, threshold=4.0) and F.saved_args(b)["usm_radius"] == 21


@pytest.mark.parametrize("bad", [
    TRAIN + ["--gt_usm"],
    TRAIN + ["--gpu_data", "--synth_lr", "--degrade", "blind", "--gt_usm"],
    TRAIN + ["--gpu_data", "--synth_lr", "--gt_usm"],
    TRAIN + ["--gpu_data", "--synth_lr", "--degrade", "blind", "--resize_mode_prob", "0.3", "0.3", "0.4"],
    TRAIN + ["--resize_mode_prob", "0", "0", "1"],
    ON + ["--usm_weight", "0.5"],
    ON + ["--usm_threshold", "10"],
    ON + ["--usm_radius", "50"],
    ON + ["--gt_usm", "--usm_radius", "0"],
    ON + ["--gt_usm", "--usm_radius", "52"],
    ON + ["--gt_usm", "--usm_weight", "-1"],
    ON + ["--gt_usm", "--usm_threshold", "300"],
    ON + ["--resize_mode_prob", "0.5", "0.6", "0.1"],
    ON + ["--resize_mode_prob", "0.5", "0.5"],
])
def test_finetune_refuses(bad, capsys):
    from tpu_superresolution_amd import finetune_swinir as F
    with pytest.raises(SystemExit) as e:
        F.parse_args(bad)
    assert e.value.code == 2 and "error:" in capsys.readouterr().err


def test_evaluate_parser():
    from tpu_superresolution_amd import evaluate as E
    from tpu_superresolution_amd.sr_datasets import UsmSpec
    base = ["--scale", "X2", "--ckpt", "F", "--arch", "swinir", "--synth_lr"]
    a = E.parse_args(base + ["--degrade", "second_order", "--gt_usm", "--usm_weight", "0.7", "--tile", "64", "--self_ensemble", "--bench_metric", "y"])
    assert E.eval_usm(a) == UsmSpec(weight=0.7) and E.eval_usm(E.parse_args(base + ["--degrade", "second_order"])) is None
    for bad in (base + ["--gt_usm"], base + ["--degrade", "blind", "--gt_usm"], base + ["--degrade", "second_order", "--usm_weight", "0.5"],
                base + ["--degrade", "second_order", "--gt_usm", "--usm_radius", "99"], base + ["--degrade", "second_order", "--resize_mode_prob", "0", "0", "1"]):
        with pytest.raises(SystemExit):
            E.parse_args(bad)


def test_pool_and_batches_refuse_without_a_device():
    from tpu_superresolution_amd.sr_datasets import SecondOrderSpec, SynthLRBatches, UsmSpec
    with pytest.raises(ValueError, match="usm="):
        SynthLRBatches([], 2, 8, "cpu", usm=UsmSpec())
    with pytest.raises(ValueError, match="usm="):
        SynthLRBatches([], 2, 8, "cpu", degrade=None, second_order=None, usm="x")
    assert SecondOrderSpec().draw_modes(None) == (0, 0, 0)
