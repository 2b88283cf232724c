"""The scale-1 tasks from the command line, end to end on the device: finetune_swinir --task dn | car writes a checkpoint that
evaluate --task scores; DeviceRestorePool places its patches where DevicePairPool does; RestoreBatches is ops.restore_degrade."""
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

SIZE = 96


def _make_tree(root, n=4, seed=0):
    """train / valid / test HR directories of n random SIZE x SIZE RGB PNGs each; no LR directory."""
    rs = np.random.RandomState(seed)
    for split in ("train", "valid", "test"):
        d = os.path.join(root, "shuffled2D", f"shuffled2D_{split}_HR")
        os.makedirs(d)
        for i in range(n):
            base = (rs.rand(SIZE // 4 + 1, SIZE // 4 + 1, 3) * 255).astype(np.uint8)
            Image.fromarray(base).resize((SIZE, SIZE), Image.BICUBIC).save(os.path.join(d, f"{i:04d}.png"))


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("restore_script") / "data")
    _make_tree(r)
    return r


TASKS = {"dn": (["--task", "dn", "--dn_sigma", "25", "25", "--lr_patch", "48"], ["--task", "dn", "--dn_sigma", "25"], 8, 3),
         "car": (["--task", "car", "--jpeg_quality", "10", "40", "--channels", "1", "--lr_patch", "42"],
                 ["--task", "car", "--jpeg_quality", "25", "--channels", "1"], 7, 1),
         # the existing options on the new pairs: the graphed small-window step, EMA weights, D4 augmentation, another loss, tiled validation
         "car_opts": (["--task", "car", "--jpeg_quality", "10", "40", "--jpeg_subsample", "420", "--lr_patch", "42", "--graph", "--ema_decay", "0.999",
                       "--augment", "d4", "--loss", "charbonnier", "--val_tile", "64", "--val_tile_overlap", "16"],
                      ["--task", "car", "--jpeg_quality", "25", "--jpeg_subsample", "420", "--self_ensemble", "--param_key", "params_ema", "--tile", "64"], 7, 3)}


@pytest.mark.parametrize("case", list(TASKS))
def test_finetune_then_evaluate(root, case, tmp_path, capsys, monkeypatch):
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    train_flags, eval_flags, window, channels = TASKS[case]
    task = train_flags[1]
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", root, "--scale", "X1", "--workers", "0", "--epochs", "1", "--batch_size", "2"] + train_flags)
    out = capsys.readouterr().out
    assert f"[task {task}]" in out and "[done] best_val_loss=" in out
    m = re.search(r"\[X1\] epoch 001/1 .*train (?:L1|loss\[[a-z]+\])=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB", out)
    assert m and all(np.isfinite(float(v)) for v in m.groups())
    ck = tmp_path / "bestpsnr_swinir_finetune_X1.pt"
    assert ck.exists() and (tmp_path / "best_swinir_finetune_X1.pt").exists()
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert saved["args"]["task"] == task and saved["args"]["window_size"] == window and saved["args"]["gpu_data"] is True
    assert saved["model"]["conv_last.weight"].shape[0] == channels and not [k for k in saved["model"] if k.startswith("upsample")]
    ev = ["--scale", "X1", "--data_root", root, "--ckpt", str(ck), "--batch_size", "2", "--save_dir", str(tmp_path / "p"), "--save_n", "1",
          "--arch", "swinir", "--device", "cuda"] + eval_flags
    res = evaluate.main(ev)
    text = capsys.readouterr().out
    assert "[baseline] Degraded input PSNR" in text and "Bicubic" not in text and f"[task {task}]" in text
    assert re.search(r"\[done\] test PSNR: [0-9.]+ dB", text)
    assert np.isfinite(res["psnr"]) and np.isfinite(res["ssim"]) and np.isfinite(res["bicubic_psnr"]) and res["n"] == 4
    assert res["bicubic_psnr"] < 60.0          # the baseline is the degraded input, not the clean image (80 dB by the script's formula)
    again = evaluate.main(ev)          # noise id = image index: the same degraded images, the same scores
    capsys.readouterr()
    assert again["bicubic_psnr"] == res["bicubic_psnr"] and again["bicubic_ssim"] == res["bicubic_ssim"]
    if case == "dn":          # tiles at scale 1, merged: another prediction, a finite score
        tiled = evaluate.main(ev + ["--tile", "64"])
        assert "[tile] 64 overlap 32" in capsys.readouterr().out
        assert np.isfinite(tiled["psnr"]) and tiled["bicubic_psnr"] == res["bicubic_psnr"]


@pytest.mark.parametrize("augment", ["none", "d4"])
def test_restore_pool_cuts_where_the_pair_pool_cuts(augment):
    from tpu_superresolution_amd.sr_datasets import DevicePairPool, DeviceRestorePool, RestoreSpec
    rs = np.random.RandomState(5)
    imgs = [rs.randint(0, 256, (45, 61, 3)).astype(np.uint8), rs.randint(0, 256, (40, 72)).astype(np.uint8),
            rs.randint(0, 65536, (33, 50, 3)).astype(np.uint16)]
    P, batch = 20, [0, 1, 2, 2, 1, 0, 1]
    pairs = DevicePairPool([(a, a) for a in imgs], P, 1, augment=augment)
    quiet = DeviceRestorePool(imgs, P, 3, RestoreSpec(seed=4), augment=augment)
    noisy = DeviceRestorePool(imgs, P, 3, RestoreSpec(sigma=(0.02, 0.1), jpeg_quality=(10, 90), gray_noise_p=0.5, subsample=True, seed=4), augment=augment)
    random.seed(17)
    lr, hr = pairs.sample(batch)
    state = random.getstate()
    for pool in (quiet, noisy):
        random.seed(17)
        degraded, clean = pool.sample(batch)
        assert random.getstate() == state, "the pools must consume the global `random` alike"
        assert torch.equal(clean, hr) and torch.equal(clean, lr)
        assert torch.equal(degraded, clean) == (pool is quiet)
    gray = DeviceRestorePool(imgs, P, 1, RestoreSpec(seed=4), augment=augment)
    random.seed(17)
    d1, c1 = gray.sample(batch)
    assert random.getstate() == state and c1.shape == (len(batch), 1, P, P) and torch.equal(d1, c1)
    assert torch.equal(c1[1], hr[1, :1]) and torch.equal(c1[4], hr[4, :1])          # the gray source as is
    with pytest.raises(ValueError):
        DeviceRestorePool(imgs, 34, 3, RestoreSpec())          # the 33-row image is too small
    with pytest.raises(ValueError):
        DeviceRestorePool(imgs, P, 2, RestoreSpec())
    with pytest.raises(ValueError):
        DeviceRestorePool(imgs, P, 3, None)


def test_restore_pool_is_the_window_of_the_whole_image_degradation():
    """The pool's patch, D4 transform undone by construction (augment none), against ops.restore_degrade on the whole image with the
    parameters the spec's generator gives."""
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import DeviceRestorePool, RestoreSpec, clean_to_tensor
    rs = np.random.RandomState(6)
    imgs = [rs.randint(0, 256, (45, 61, 3)).astype(np.uint8), rs.randint(0, 256, (40, 72, 3)).astype(np.uint8)]
    spec = RestoreSpec(sigma=(0.02, 0.1), jpeg_quality=(10, 90), gray_noise_p=0.5, subsample=True, seed=9)
    for oc in (3, 1):
        pool = DeviceRestorePool(imgs, 32, oc, spec, rank=1)
        batch = [0, 1, 1, 0]
        random.seed(3)
        hd, _ = pool.draw(batch)
        g = spec.rng(1)
        drawn = [spec.draw(g, colour=oc == 3) for _ in batch]
        pool._spec_rng = spec.rng(1)
        random.seed(3)
        degraded, clean = pool.sample(batch)
        for b, (i, d, (sigma, q, nid, gr)) in enumerate(zip(batch, hd, drawn)):
            x = clean_to_tensor(Image.fromarray(imgs[i]), oc).cuda()[None]
            top, left = d[4], d[5]
            whole = ops.restore_degrade(x, (sigma, 0.0), [nid], gr, q, True, 0)
            assert torch.equal(clean[b], x[0, :, top:top + 32, left:left + 32])
            assert torch.equal(degraded[b], whole[0, :, top:top + 32, left:left + 32]), (oc, b, top, left, q)


def test_restore_batches_degrade_whole_images_the_same_every_epoch():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import FixedRestore, RestoreBatches, RestoreSpec
    g = torch.Generator().manual_seed(0)
    colour = (torch.randint(0, 256, (3, 3, 40, 56), generator=g).float() / 255.0)
    colour[1, 1], colour[1, 2] = colour[1, 0], colour[1, 0]          # a gray image in three channels: gray noise
    loader = [colour[:2], colour[2:]]
    spec = RestoreSpec(sigma=(0.04, 0.08), jpeg_quality=(30, 50), subsample=True)
    a = list(RestoreBatches(loader, 3, spec, 0, "cuda"))
    b = list(RestoreBatches(loader, 3, FixedRestore(0.06, 40, False, True), 0, "cuda"))
    assert len(a) == 2 and [tuple(d.shape) for d, _ in a] == [(2, 3, 40, 56), (1, 3, 40, 56)]
    for (d0, c0), (d1, c1), first in zip(a, b, (0, 2)):
        assert torch.equal(d0, d1) and torch.equal(c0, c1) and not torch.equal(d0, c0)
        n = c0.shape[0]
        grays = [first + i == 1 for i in range(n)]
        assert torch.equal(d0, ops.restore_degrade(c0, (0.06, 0.0), range(first, first + n), grays, 40, True, 0))
    one = list(RestoreBatches([colour[:, :1]], 1, FixedRestore(0.1), 8, "cuda"))[0][0]
    assert torch.equal(one, ops.noise(colour[:, :1].cuda().contiguous(), (0.1, 0.0), [0, 1, 2], True, 8))
    with pytest.raises(ValueError):
        list(RestoreBatches([colour], 1, spec, 0, "cuda"))
    with pytest.raises(ValueError):
        RestoreBatches(loader, 3, FixedRestore(2.0), 0, "cuda")
