"""evaluate.py --bench_metric end to end on the CPU (--arch ms_resunet): the new lines and keys, their values against the fp64
restatement recomputed from the (pred, hr) arrays the script scored, and everything else unchanged by the flag."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import bench_metric_ref as R
from tpu_superresolution_amd import evaluate, metrics
from tpu_superresolution_amd.ms_resunet import MS_ResUNet


def _make_tree(root, n, hr_size, scale=2, seed=0):
    hr_dir = os.path.join(root, "shuffled2D", "shuffled2D_test_HR")
    lr_dir = os.path.join(root, "shuffled2D", f"shuffled2D_test_LR_default_X{scale}")
    os.makedirs(hr_dir), os.makedirs(lr_dir)
    rs = np.random.RandomState(seed)
    for i in range(n):
        base = rs.rand(hr_size // 4 + 1, hr_size // 4 + 1, 3)
        hr = np.asarray(Image.fromarray((base * 255).astype(np.uint8)).resize((hr_size, hr_size), Image.BICUBIC))
        Image.fromarray(hr).save(os.path.join(hr_dir, f"{i:04d}.png"))
        Image.fromarray(hr).resize((hr_size // scale, hr_size // scale), Image.BICUBIC).save(os.path.join(lr_dir, f"{i:04d}x{scale}.png"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_script")
    root = str(d / "data")
    _make_tree(root, 3, 32)
    torch.manual_seed(0)
    ck = str(d / "ck.pt")
    torch.save({"model": MS_ResUNet().state_dict()}, ck)
    return d, ["--scale", "X2", "--data_root", root, "--ckpt", ck, "--batch_size", "2", "--save_n", "1", "--device", "cpu"]


def _record(monkeypatch):
    calls = []
    real = metrics.bench_metrics

    def recording(pred, target, crop_border, mode="y", with_ssim=True):
        calls.append((pred.detach().clone().numpy(), target.detach().clone().numpy(), crop_border, mode))
        return real(pred, target, crop_border, mode, with_ssim)

    monkeypatch.setattr(metrics, "bench_metrics", recording)
    return calls


def _want(calls):
    """Per-image fp64 scores of the recorded batches -> (mean PSNR, mean SSIM, PSNR bound, images)."""
    ps, ss, bound = [], [], []
    for pred, target, border, mode in calls:
        ref = R.bench_ref(pred, target, border, mode)
        ps += list(ref["psnr"])
        ss += list(ref["ssim"])
        bound += list(R.psnr_bound(ref["sqsum"], ref["pp"][0].size, mode, pred.shape[1]))
    return float(np.mean(ps)), float(np.mean(ss)), float(np.max(bound)), len(ps)


@pytest.mark.parametrize("mode,border", [("y", None), ("rgb", 3)])
def test_evaluate_reports_the_benchmark_protocol_scores(tree, capsys, monkeypatch, mode, border):
    d, common = tree
    plain = evaluate.main(common + ["--save_dir", str(d / f"plain_{mode}")])
    plain_text = capsys.readouterr().out
    assert "[bench]" not in plain_text and not any(k.startswith("bench_") for k in plain)
    calls = _record(monkeypatch)
    flags = ["--bench_metric", mode] + ([] if border is None else ["--crop_border", str(border)])
    out = evaluate.main(common + ["--save_dir", str(d / f"bench_{mode}")] + flags)
    text = capsys.readouterr().out
    # everything the script reported before is unchanged by the flag
    for k in ("psnr", "ssim", "bicubic_psnr", "bicubic_ssim", "saved", "n"):
        assert out[k] == plain[k], k
    assert set(out) - set(plain) == {"bench_psnr", "bench_ssim", "bench_bicubic_psnr", "bench_bicubic_ssim"}
    strip = [ln for ln in text.splitlines() if not ln.startswith(("[bench]", "[done]", "[saved]"))]
    assert strip == [ln for ln in plain_text.splitlines() if not ln.startswith(("[done]", "[saved]"))]
    # two batches (2 + 1 images) for the baseline, then two for the model; the default border is the scale
    b = 2 if border is None else border
    assert [(c[0].shape[0], c[2], c[3]) for c in calls] == [(2, b, mode), (1, b, mode)] * 2
    tag = mode.upper()
    lines = [ln for ln in text.splitlines() if ln.startswith("[bench]")]
    for line, key, batches in ((lines[0], "bench_bicubic", calls[:2]), (lines[1], "bench", calls[2:])):
        want_p, want_s, bound, n = _want(batches)
        assert n == 3 and abs(out[key + "_psnr"] - want_p) <= bound and abs(out[key + "_ssim"] - want_s) <= R.SSIM_BOUND
        what = "Bicubic " if key == "bench_bicubic" else ""
        assert line == (f"[bench] {what}PSNR-{tag}: {out[key + '_psnr']:.2f} dB | SSIM-{tag}: {out[key + '_ssim']:.4f} "
                        f"(8-bit, border {b}, mean over 3 images)")
    assert len(lines) == 2 and text.index("[bench] Bicubic") < text.index("[ckpt]") < text.index("[done]") < text.index("[bench] PSNR-")
    # the mean is over images: with a short last batch the mean of the batch means is another number
    per = np.concatenate([R.bench_ref(*c)["psnr"] for c in calls[2:]])
    assert abs((per[:2].mean() + per[2]) / 2 - per.mean()) > 10 * _want(calls[2:])[2]
    # the protocol's number is not the script's own: another scale, another crop, 8 bits
    assert abs(out["bench_psnr"] - out["psnr"]) > 0.01


def test_argument_errors(tree, capsys):
    d, common = tree
    with pytest.raises(SystemExit):
        evaluate.main(common + ["--save_dir", str(d / "e1"), "--crop_border", "2"])
    assert "--crop_border" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        evaluate.main(common + ["--save_dir", str(d / "e2"), "--bench_metric", "y", "--crop_border", "-1"])
    with pytest.raises(SystemExit):
        evaluate.main(common + ["--save_dir", str(d / "e3"), "--bench_metric", "ycbcr"])
    capsys.readouterr()
    with pytest.raises(ValueError, match="border of 16 leaves nothing of 32 x 32"):
        evaluate.main(common + ["--save_dir", str(d / "e4"), "--bench_metric", "y", "--crop_border", "16"])
    with pytest.raises(ValueError, match="11 x 11"):          # 32 - 2 * 11 = 10: too small for the SSIM window
        evaluate.main(common + ["--save_dir", str(d / "e5"), "--bench_metric", "y", "--crop_border", "11"])


# ---- finetune_swinir: the flags (the validation loop itself needs the device: tests/test_gpu_bench_metric.py) -----------------------------
def test_finetune_flags():
    from tpu_superresolution_amd import finetune_swinir as F
    base = ["--data_root", "d", "--scale", "X4"]
    a = F.parse_args(base)
    assert a.val_bench_metric is None and a.val_crop_border is None
    assert "val_bench_metric" not in F.saved_args(a) and "val_crop_border" not in F.saved_args(a)          # no trace at the defaults
    a = F.parse_args(base + ["--val_bench_metric", "rgb", "--val_crop_border", "3"])
    assert (a.val_bench_metric, a.val_crop_border) == ("rgb", 3)
    assert F.saved_args(a)["val_bench_metric"] == "rgb" and F.saved_args(a)["val_crop_border"] == 3
    for bad in (["--val_crop_border", "2"], ["--val_bench_metric", "y", "--val_crop_border", "-1"], ["--val_bench_metric", "ycbcr"]):
        with pytest.raises(SystemExit):
            F.parse_args(base + bad)
