"""python -m tpu_superresolution_amd.niqe fit | score with --device cpu on generated files -- lines, dicts, the skip line, every refusal with
its message -- and predict's --niqe flags: parsing and the validation of the parameter file before the checkpoint is opened."""
import numpy as np
import pytest
import torch
from PIL import Image

import niqe_ref as R


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("niqe_files")
    good = d / "good"
    good.mkdir()
    for s in (0, 1, 2):
        Image.fromarray(R.pink_image(s, 192).astype(np.uint8), mode="L").save(good / f"g{s}.png")
    mixed = d / "mixed"
    mixed.mkdir()
    Image.fromarray(R.noised(R.pink_image(3, 192), 25).astype(np.uint8), mode="L").save(mixed / "a_noisy.png")
    Image.fromarray(R.pink_image(4, 192).astype(np.uint8), mode="L").save(mixed / "b_clean.png")
    rgb = np.stack([R.pink_image(s, 192)[:100, :192] for s in (5, 6, 7)], axis=-1).astype(np.uint8)
    Image.fromarray(rgb, mode="RGB").save(mixed / "c_one_block_row.png")          # 100 x 192: 1 x 2 blocks
    Image.fromarray(R.pink_image(8, 64).astype(np.uint8), mode="L").save(mixed / "d_small.png")
    (mixed / "e_notes.txt").write_text("not an image")
    small = d / "small"
    small.mkdir()
    Image.fromarray(R.pink_image(8, 64).astype(np.uint8), mode="L").save(small / "d_small.png")
    return d


@pytest.fixture(scope="module")
def fitted(files):
    from tpu_superresolution_amd import niqe as N
    lines = []
    out = files / "fit.npz"
    r = N.main(["fit", "--input", str(files / "good"), "--out", str(out), "--sharpness", "0", "--device", "cpu", "--batch_size", "2"], log=lines.append)
    return out, r, lines


def test_fit_writes_the_basicsr_format_and_equals_the_library_fit(files, fitted):
    from tpu_superresolution_amd import metrics
    out, r, lines = fitted
    assert r["n"] == 3 and r["files"] == ["g0.png", "g1.png", "g2.png"] and lines[-1] == f"[done] fitted on 3 images -> {out}"
    p = metrics.load_niqe_params(out)
    mu, cov = metrics.niqe_fit([torch.from_numpy(R.as_batch(R.pink_image(s, 192))) for s in (0, 1, 2)], sharpness=0.0)
    assert np.array_equal(p["mu"], mu) and np.array_equal(p["cov"], cov) and np.array_equal(p["window"], R.window())


def test_score_prints_a_line_per_file_skips_small_files_and_returns_the_mean(files, fitted):
    from tpu_superresolution_amd import metrics
    from tpu_superresolution_amd import niqe as N
    out, _, _ = fitted
    lines = []
    r = N.main(["score", "--input", str(files / "mixed"), "--params", str(out), "--device", "cpu", "--batch_size", "4"], log=lines.append)
    assert list(r["scores"]) == ["a_noisy.png", "b_clean.png", "c_one_block_row.png"] and r["n"] == 3
    assert r["scores"]["b_clean.png"] < r["scores"]["a_noisy.png"]
    assert r["mean"] == float(np.mean(list(r["scores"].values())))
    for name, v in r["scores"].items():
        assert f"[niqe] {name} {v:.4f}" in lines
    assert any(ln.startswith("[niqe] d_small.png: skipped (") and "holds no block" in ln for ln in lines)
    assert any(ln.startswith("[skip] e_notes.txt") for ln in lines)
    assert lines[-1] == f"[done] 3 images | mean {r['mean']:.4f}"
    x = torch.from_numpy(R.as_batch(R.noised(R.pink_image(3, 192), 25)))
    assert r["scores"]["a_noisy.png"] == float(metrics.niqe(x, str(out))[0])
    one = N.main(["score", "--input", str(files / "mixed" / "b_clean.png"), "--params", str(out), "--device", "cpu"], log=lines.append)
    assert one["scores"] == {"b_clean.png": r["scores"]["b_clean.png"]}


def test_a_file_with_one_block_is_skipped_and_no_scored_file_is_an_error(files, fitted):
    from tpu_superresolution_amd import niqe as N
    out, _, _ = fitted
    lines = []
    with pytest.raises(SystemExit, match="no file could be scored"):
        N.main(["score", "--input", str(files / "mixed" / "c_one_block_row.png"), "--params", str(out), "--device", "cpu", "--crop_border", "50"], log=lines.append)
    assert any(ln.startswith("[niqe] c_one_block_row.png: skipped (") for ln in lines)
    lines.clear()
    Image.fromarray(R.pink_image(9, 150).astype(np.uint8)[:100, :150], mode="L").save(files / "one_block.png")
    with pytest.raises(SystemExit, match="no file could be scored"):
        N.main(["score", "--input", str(files / "one_block.png"), "--params", str(out), "--device", "cpu"], log=lines.append)
    assert any("holds 1 block" in ln and "at least 2" in ln for ln in lines)
    with pytest.raises(SystemExit, match="no file could be scored"):
        N.main(["score", "--input", str(files / "small"), "--params", str(out), "--device", "cpu"], log=lines.append)
    empty = files / "empty"
    empty.mkdir()
    with pytest.raises(SystemExit, match="no image that PIL can open"):
        N.main(["score", "--input", str(empty), "--params", str(out), "--device", "cpu"], log=lines.append)
    with pytest.raises(SystemExit, match="at least 2"):
        N.main(["fit", "--input", str(files / "small"), "--out", str(files / "never.npz"), "--device", "cpu"], log=lines.append)
    assert not (files / "never.npz").exists()


@pytest.mark.parametrize("argv,msg", [
    (["score", "--input", "x", "--params", "{missing}"], "cannot be read as a NIQE parameter file"),
    (["score", "--input", "x", "--params", "{nokey}"], "lacks"),
    (["score", "--input", "x", "--params", "{fit}", "--crop_border", "-1"], "--crop_border must be >= 0"),
    (["score", "--input", "x", "--params", "{fit}", "--batch_size", "0"], "--batch_size must be >= 1"),
    (["fit", "--input", "x", "--out", "y.npz", "--sharpness", "1.5"], "--sharpness must be in"),
    (["fit", "--input", "x"], "--out"),
    (["rank", "--input", "x"], "invalid choice"),
])
def test_command_line_refusals(files, fitted, capsys, argv, msg):
    from tpu_superresolution_amd import niqe as N
    np.savez(files / "nokey.npz", mu_pris_param=np.zeros((1, 36)))
    sub = {"{missing}": str(files / "missing.npz"), "{nokey}": str(files / "nokey.npz"), "{fit}": str(fitted[0])}
    with pytest.raises(SystemExit) as e:
        N.parse_args([sub.get(a, a) for a in argv])
    assert e.value.code == 2 and msg in capsys.readouterr().err


# ---- predict --niqe ----------------------------------------------------------------------------------------------------------------------
PREDICT = ["--input", "in", "--output", "out", "--arch", "swinir", "--scale", "X2", "--ckpt", "does_not_exist.pt"]


def test_predict_parses_the_niqe_flags_and_loads_the_file(fitted):
    from tpu_superresolution_amd import predict as P
    args = P.parse_args(PREDICT)
    assert args.niqe is None and args.niqe_params is None and args.niqe_crop_border == 0
    args = P.parse_args(PREDICT + ["--niqe", str(fitted[0]), "--niqe_crop_border", "4"])
    assert args.niqe_crop_border == 4 and args.niqe_params["mu"].shape == (36,) and args.niqe_params["cov"].shape == (36, 36)


@pytest.mark.parametrize("kind,msg", [("missing", "cannot be read"), ("nokey", "lacks"), ("shape", "expected mu_pris_param"), ("nan", "non-finite"),
                                      ("asym", "not symmetric"), ("border", "--niqe_crop_border"), ("border_alone", "--niqe_crop_border")])
def test_predict_refuses_a_bad_parameter_file_before_the_checkpoint_is_opened(tmp_path, fitted, capsys, kind, msg):
    """The checkpoint of PREDICT does not exist: a refusal that names --niqe came first."""
    from tpu_superresolution_amd import predict as P
    path = tmp_path / f"{kind}.npz"
    full = dict(mu_pris_param=np.zeros((1, 36)), cov_pris_param=np.eye(36), gaussian_window=R.window())
    if kind == "nokey":
        np.savez(path, mu_pris_param=full["mu_pris_param"])
    elif kind == "shape":
        np.savez(path, **dict(full, gaussian_window=np.ones((5, 5))))
    elif kind == "nan":
        np.savez(path, **dict(full, mu_pris_param=np.full((1, 36), np.inf)))
    elif kind == "asym":
        np.savez(path, **dict(full, cov_pris_param=np.triu(np.ones((36, 36)))))
    extra = {"border": ["--niqe", str(fitted[0]), "--niqe_crop_border", "-2"], "border_alone": ["--niqe_crop_border", "2"]}.get(kind, ["--niqe", str(path)])
    with pytest.raises(SystemExit) as e:
        P.parse_args(PREDICT + extra)
    err = capsys.readouterr().err
    assert e.value.code == 2 and msg in err and "--niqe" in err
