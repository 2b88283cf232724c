"""--degrade second_order from the command line, end to end on the device: finetune_swinir trains on DeviceHR2Pool's pairs (with --graph,
EMA weights, D4 augmentation, another loss, tiled validation) and writes a checkpoint that evaluate --synth_lr --degrade second_order
scores on the fixed chain; SynthLRBatches(second_order=) is ops.degrade_second_order on whole images, the same every epoch."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

SIZE = 96


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    """train / valid / test HR directories of four SIZE x SIZE RGB PNGs each; no LR directory."""
    r = str(tmp_path_factory.mktemp("degrade2_script") / "data")
    rs = np.random.RandomState(0)
    for split in ("train", "valid", "test"):
        d = os.path.join(r, "shuffled2D", f"shuffled2D_{split}_HR")
        os.makedirs(d)
        for i in range(4):
            base = (rs.rand(SIZE // 4 + 1, SIZE // 4 + 1, 3) * 255).astype(np.uint8)
            Image.fromarray(base).resize((SIZE, SIZE), Image.BICUBIC).save(os.path.join(d, f"{i:04d}.png"))
    return r


def test_finetune_with_graph_then_evaluate(root, tmp_path, capsys, monkeypatch):
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", root, "--scale", "X2", "--workers", "0", "--epochs", "1", "--batch_size", "2", "--lr_patch", "16", "--gpu_data",
            "--synth_lr", "--degrade", "second_order", "--blur_kernel", "mixed", "--jpeg_subsample", "420", "--sinc_p", "0.3",
            "--window_size", "4", "--graph", "--ema_decay", "0.999", "--augment", "d4", "--loss", "charbonnier", "--val_tile", "32",
            "--val_tile_overlap", "8"])
    out = capsys.readouterr().out
    assert "[degrade] second order: window 64 x 64 HR px (margin 8 LR px)" in out and "[done] best_val_loss=" in out
    m = re.search(r"\[X2\] epoch 001/1 .*train (?:L1|loss\[[a-z]+\])=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB", out)
    assert m and all(np.isfinite(float(v)) for v in m.groups())
    ck = tmp_path / "bestpsnr_swinir_finetune_X2.pt"
    saved = torch.load(ck, map_location="cpu", weights_only=False)["args"]
    assert saved["degrade"] == "second_order" and saved["sinc_p"] == 0.3 and "final_sinc_p" not in saved and "degrade_margin" not in saved
    ev = ["--scale", "X2", "--data_root", root, "--ckpt", str(ck), "--batch_size", "2", "--arch", "swinir", "--window_size", "4", "--device", "cuda",
          "--synth_lr", "--degrade", "second_order", "--jpeg_subsample", "420"]
    res = evaluate.main(ev)
    text = capsys.readouterr().out
    assert "[degrade] second order, fixed:" in text and re.search(r"\[done\] test PSNR: [0-9.]+ dB", text)
    assert np.isfinite(res["psnr"]) and np.isfinite(res["bicubic_psnr"]) and res["n"] == 4
    again = evaluate.main(ev + ["--tile", "32", "--tile_overlap", "8", "--self_ensemble", "--bench_metric", "y", "--param_key", "params_ema"])
    capsys.readouterr()
    assert np.isfinite(again["psnr"])
    clean = evaluate.main(ev[:-4])          # the plain bicubic LR: a better baseline than the degraded one
    capsys.readouterr()
    assert clean["bicubic_psnr"] > res["bicubic_psnr"]


def test_whole_images_get_the_fixed_chain_every_epoch():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, SecondOrderSpec, SynthLRBatches, stage1_table
    g = torch.Generator().manual_seed(0)
    hr = torch.randint(0, 256, (3, 3, 49, 66), generator=g).float() / 255.0
    hr[1, 1], hr[1, 2] = hr[1, 0], hr[1, 0]          # a gray image in three channels: gray noise
    loader = [hr[:2], hr[2:]]
    spec, deg = SecondOrderSpec(), DegradeSpec()
    a = list(SynthLRBatches(loader, 2, 8, "cuda", degrade=deg, second_order=spec))
    b = list(SynthLRBatches(loader, 2, 8, "cuda", degrade=deg, second_order=spec))
    fx = deg.fixed()
    for (l0, h0), (l1, h1), first in zip(a, b, (0, 2)):
        n = h0.shape[0]
        assert torch.equal(l0, l1) and torch.equal(h0, h1) and tuple(h0.shape) == (n, 3, 48, 66) and tuple(l0.shape) == (n, 3, 24, 33)
        ps = [spec.fixed(stage1_table(fx.blur), fx.noise, first + i == 1, first + i) for i in range(n)]
        assert torch.equal(l0, ops.degrade_second_order(h0, 2, ps))
    for kw in (dict(second_order=spec), dict(degrade=deg, second_order=spec, jpeg=50), dict(degrade=deg, second_order="x")):
        with pytest.raises(ValueError):
            SynthLRBatches(loader, 2, 8, "cuda", **kw)
    with pytest.raises(ValueError):
        SynthLRBatches(loader, 2, 0, "cuda", degrade=deg, second_order=spec)
