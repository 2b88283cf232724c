"""python -m tpu_superresolution_amd.score with --device cpu on generated files: pairing with and without the suffix, a missing partner,
--gt_modcrop, mixed sizes split into batches, the `-` of a pair too small for a metric, and the result dict against the library functions."""
import numpy as np
import pytest
import torch
from PIL import Image

import fullref_ref as R

ALL = ["--metrics", "psnr", "ssim", "psnrb", "ms_ssim"]


def _rgb(seed, H, W):
    return np.stack([R.pink_image(seed + k, H, W) for k in range(3)], axis=-1)


def _save(a, path):
    a = a.astype(np.uint8)
    Image.fromarray(a, mode="RGB" if a.ndim == 3 else "L").save(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """gt: a (RGB 170 x 165), b (gray 170 x 165), c (RGB 64 x 64), d (RGB 170 x 165), z (no SR file).  sr: a_sr, b_sr, c_sr, d_sr."""
    d = tmp_path_factory.mktemp("score_files")
    gt, sr = d / "gt", d / "sr"
    gt.mkdir()
    sr.mkdir()
    imgs = {"a": _rgb(1, 170, 165), "b": R.pink_image(5, 170, 165), "c": _rgb(7, 64, 64), "d": _rgb(11, 170, 165)}
    for k, (n, a) in enumerate(imgs.items()):
        _save(a, gt / f"{n}.png")
        _save(R.noised(a, 6 + 4 * k, k), sr / f"{n}_sr.png")
    _save(_rgb(20, 64, 64), gt / "z.png")
    (sr / "notes.txt").write_text("not an image")
    return d, imgs


def _t(a):
    a = a[:, :, None] if a.ndim == 2 else a
    return (torch.from_numpy(a.astype(np.uint8)).permute(2, 0, 1)[None].float() / 255.0)


def test_scores_equal_the_library_functions_and_small_pairs_print_a_dash(files):
    from tpu_superresolution_amd import metrics as M
    from tpu_superresolution_amd import score as S
    d, imgs = files
    lines = []
    r = S.main(["--sr", str(d / "sr"), "--gt", str(d / "gt"), "--device", "cpu", "--batch_size", "4", "--crop_border", "2"] + ALL, log=lines.append)
    assert r["n"] == 4 and list(r["scores"]) == ["a_sr.png", "b_sr.png", "c_sr.png", "d_sr.png"] and r["unmatched_gt"] == 1
    assert "[pair] 1 ground-truth files have no SR file" in lines and any(ln.startswith("[skip] notes.txt") for ln in lines)
    for k, n in enumerate("abd"):
        sr, gt = _t(R.noised(imgs[n], 6 + 4 * "abcd".index(n), "abcd".index(n))), _t(imgs[n])
        ps, ss = M.bench_metrics(sr, gt, 2, "y")
        pp, pt = M.bench_planes_pair(sr, gt, 2, "y")
        want = {"psnr": float(ps[0]), "ssim": float(ss[0]), "psnrb": float(M.psnrb(sr, gt, 2, "y")[0]),
                "ms_ssim": float(M.ms_ssim(pp, pt, size_average=False)[0])}
        assert r["scores"][f"{n}_sr.png"] == want
        assert float(want["psnrb"]) == pytest.approx(R.psnrb(pp.numpy(), pt.numpy())[0], rel=1e-6)
        assert float(want["ms_ssim"]) == pytest.approx(R.msssim(pp.numpy(), pt.numpy())[0], rel=1e-4)
    c = r["scores"]["c_sr.png"]
    assert c["ms_ssim"] is None and c["psnr"] is not None and c["ssim"] is not None and c["psnrb"] is not None
    line = next(ln for ln in lines if ln.startswith("[score] c_sr.png"))
    assert line.endswith(" ms_ssim=-") and f"psnr={c['psnr']:.4f} ssim={c['ssim']:.6f} psnrb={c['psnrb']:.4f}" in line
    a = r["scores"]["a_sr.png"]
    assert f"[score] a_sr.png psnr={a['psnr']:.4f} ssim={a['ssim']:.6f} psnrb={a['psnrb']:.4f} ms_ssim={a['ms_ssim']:.6f}" in lines
    assert r["mean"]["ms_ssim"] == float(np.mean([r["scores"][f"{n}_sr.png"]["ms_ssim"] for n in "abd"]))      # c stays out of this mean
    assert r["mean"]["psnr"] == float(np.mean([s["psnr"] for s in r["scores"].values()]))
    assert lines[-1] == "[done] 4 pairs | " + " ".join(f"{m}={r['mean'][m]:.4f}" if m in ("psnr", "psnrb") else f"{m}={r['mean'][m]:.6f}"
                                                       for m in ("psnr", "ssim", "psnrb", "ms_ssim"))


def test_mixed_sizes_split_into_batches_and_the_batch_size_does_not_change_a_score(files, monkeypatch):
    from tpu_superresolution_amd import score as S
    d, _ = files
    sizes = []
    real = S.score_batch
    monkeypatch.setattr(S, "score_batch", lambda sr, gt, *a: (sizes.append(tuple(sr.shape)), real(sr, gt, *a))[1])
    base = ["--sr", str(d / "sr"), "--gt", str(d / "gt"), "--device", "cpu", "--metrics", "psnr", "psnrb"]
    r4 = S.main(base + ["--batch_size", "4"], log=lambda s: None)
    assert sizes == [(1, 3, 170, 165), (1, 1, 170, 165), (1, 3, 64, 64), (1, 3, 170, 165)]      # a | b (gray) | c (small) | d: only neighbours join
    sizes.clear()
    r1 = S.main(base, log=lambda s: None)
    assert len(sizes) == 4 and r1["scores"] == r4["scores"]
    # two neighbours of one size and mode form a batch
    two = d / "two"
    (two / "sr").mkdir(parents=True)
    (two / "gt").mkdir()
    for n in "ad":
        (two / "sr" / f"{n}_sr.png").write_bytes((d / "sr" / f"{n}_sr.png").read_bytes())
        (two / "gt" / f"{n}.png").write_bytes((d / "gt" / f"{n}.png").read_bytes())
    sizes.clear()
    r2 = S.main(["--sr", str(two / "sr"), "--gt", str(two / "gt"), "--device", "cpu", "--metrics", "psnr", "psnrb", "--batch_size", "4"], log=lambda s: None)
    assert sizes == [(2, 3, 170, 165)] and r2["scores"] == {n: r1["scores"][n] for n in ("a_sr.png", "d_sr.png")}


def test_pairing_by_suffix_without_suffix_and_of_two_files(files, tmp_path):
    from tpu_superresolution_amd import score as S
    d, imgs = files
    plain = tmp_path / "plain"
    plain.mkdir()
    for n in "ac":
        (plain / f"{n}.png").write_bytes((d / "sr" / f"{n}_sr.png").read_bytes())
    r = S.main(["--sr", str(plain), "--gt", str(d / "gt"), "--device", "cpu"], log=lambda s: None)          # stems equal: the suffix is absent
    assert list(r["scores"]) == ["a.png", "c.png"] and r["unmatched_gt"] == 3 and list(r["mean"]) == ["psnr", "ssim"]
    other = tmp_path / "other"
    other.mkdir()
    (other / "a_x4.png").write_bytes((d / "sr" / "a_sr.png").read_bytes())
    r2 = S.main(["--sr", str(other), "--gt", str(d / "gt"), "--device", "cpu", "--suffix", "_x4"], log=lambda s: None)
    assert r2["scores"]["a_x4.png"] == r["scores"]["a.png"]
    one = S.main(["--sr", str(other / "a_x4.png"), "--gt", str(d / "gt" / "a.png"), "--device", "cpu"], log=lambda s: None)      # two files: one pair
    assert one["scores"]["a_x4.png"] == r["scores"]["a.png"] and one["n"] == 1
    with pytest.raises(SystemExit) as e:                         # the default suffix does not match: every orphan in one error, nothing scored
        S.main(["--sr", str(other), "--gt", str(d / "gt"), "--device", "cpu"], log=lambda s: None)
    assert "1 of 1 files have no partner" in str(e.value) and "a_x4.png" in str(e.value)


def test_every_missing_partner_is_reported_before_anything_runs(files, tmp_path):
    from tpu_superresolution_amd import score as S
    d, _ = files
    sr = tmp_path / "sr"
    sr.mkdir()
    for n in ("a_sr", "q_sr", "r"):
        (sr / f"{n}.png").write_bytes((d / "sr" / "a_sr.png").read_bytes())
    lines = []
    with pytest.raises(SystemExit) as e:
        S.main(["--sr", str(sr), "--gt", str(d / "gt"), "--device", "cpu"], log=lines.append)
    msg = str(e.value)
    assert "2 of 3 files have no partner" in msg and "q_sr.png" in msg and "r.png" in msg and "'q'" in msg and "a_sr.png" not in msg
    assert not any(ln.startswith("[score]") for ln in lines)


def test_gt_modcrop_and_the_size_error_that_names_both_files(files, tmp_path):
    from tpu_superresolution_amd import score as S
    d, imgs = files
    gt, sr = tmp_path / "gt", tmp_path / "sr"
    gt.mkdir()
    sr.mkdir()
    _save(imgs["a"], gt / "a.png")                                # 170 x 165; modcrop 4 -> 168 x 164
    _save(R.noised(imgs["a"][:168, :164], 8, 3), sr / "a_sr.png")
    argv = ["--sr", str(sr), "--gt", str(gt), "--device", "cpu", "--metrics", "psnr", "psnrb"]
    with pytest.raises(SystemExit) as e:
        S.main(argv, log=lambda s: None)
    assert "a_sr.png is 168 x 164" in str(e.value) and "a.png is 170 x 165" in str(e.value)
    r = S.main(argv + ["--gt_modcrop", "4"], log=lambda s: None)
    _save(imgs["a"][:168, :164], gt / "a.png")
    assert S.main(argv, log=lambda s: None)["scores"] == r["scores"]
    with pytest.raises(SystemExit) as e:
        S.main(argv + ["--gt_modcrop", "8"], log=lambda s: None)
    assert "after --gt_modcrop 8" in str(e.value)
    _save(imgs["b"][:168, :164], gt / "a.png")                    # gray against RGB
    with pytest.raises(SystemExit, match="3 colour channel.*with 1"):
        S.main(argv, log=lambda s: None)


def test_a_metric_that_no_pair_can_take_is_an_error_and_the_flags_are_checked(files, capsys):
    from tpu_superresolution_amd import score as S
    d, _ = files
    lines = []
    with pytest.raises(SystemExit, match="--metrics ms_ssim: no pair could be scored"):
        S.main(["--sr", str(d / "sr" / "c_sr.png"), "--gt", str(d / "gt" / "c.png"), "--device", "cpu", "--metrics", "psnr", "ms_ssim"], log=lines.append)
    assert any(ln.startswith("[score] c_sr.png psnr=") and ln.endswith("ms_ssim=-") for ln in lines)
    with pytest.raises(SystemExit, match="--metrics psnrb: no pair"):                            # a border that leaves 14 x 14
        S.main(["--sr", str(d / "sr" / "c_sr.png"), "--gt", str(d / "gt" / "c.png"), "--device", "cpu", "--metrics", "psnrb", "--crop_border", "25"],
               log=lines.append)
    with pytest.raises(SystemExit, match="does not exist"):
        S.main(["--sr", str(d / "nowhere"), "--gt", str(d / "gt"), "--device", "cpu"], log=lines.append)
    for argv, msg in [(["--sr", "x"], "--gt"), (["--sr", "x", "--gt", "y", "--metrics", "lpips"], "invalid choice"),
                      (["--sr", "x", "--gt", "y", "--crop_border", "-1"], "--crop_border must be >= 0"),
                      (["--sr", "x", "--gt", "y", "--gt_modcrop", "0"], "--gt_modcrop must be >= 1"),
                      (["--sr", "x", "--gt", "y", "--batch_size", "0"], "--batch_size must be >= 1"), (["--sr", "x", "--gt", "y", "--mode", "ycbcr"], "invalid choice")]:
        with pytest.raises(SystemExit) as e:
            S.parse_args(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    assert S.parse_args(["--sr", "x", "--gt", "y"]).suffix == "_sr"
    assert S.parse_args(["--sr", "x", "--gt", "y", "--metrics", "psnrb", "psnr", "psnrb"]).metrics == ["psnrb", "psnr"]
