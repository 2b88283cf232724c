"""--degrade_tables device from the command line, end to end on the device: finetune_swinir trains one epoch on pairs whose blur and sinc
tables the device built (DeviceHR2Pool / DeviceHRPool with tables="device"; csrc/tables.hip), and the flag reaches the
checkpoint's saved arguments only when it is given."""
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
    """train / valid HR directories of four SIZE x SIZE RGB PNGs each; no LR directory."""
    r = str(tmp_path_factory.mktemp("tables_script") / "data")
    rs = np.random.RandomState(0)
    for split in ("train", "valid"):
        d = os.path.join(r, "shuffled2D", f"shuffled2D_{split}_HR")
        os.makedirs(d)
        for i in range(4):
            base = (rs.rand(SIZE // 4 + 1, SIZE // 4 + 1, 3) * 255).astype(np.uint8)
            Image.fromarray(base).resize((SIZE, SIZE), Image.BICUBIC).save(os.path.join(d, f"{i:04d}.png"))
    return r


@pytest.mark.parametrize("degrade", [["--degrade", "second_order", "--blur_kernel", "mixed", "--sinc_p", "0.3", "--graph"],
                                     ["--degrade", "blind", "--blur_kernel", "mixed"]], ids=["second_order", "blind_mixed"])
def test_finetune_one_epoch_with_device_tables(root, tmp_path, capsys, monkeypatch, degrade):
    from tpu_superresolution_amd import finetune_swinir as F
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", root, "--scale", "X2", "--workers", "0", "--epochs", "1", "--batch_size", "2", "--lr_patch", "16", "--gpu_data",
            "--synth_lr", "--window_size", "4", "--degrade_tables", "device"] + degrade)
    out = capsys.readouterr().out
    assert "[degrade] tables: built on the device from descriptors" in out and "[done] best_val_loss=" in out
    m = re.search(r"\[X2\] epoch 001/1 .*train (?:L1|loss\[[a-z]+\])=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB", out)
    assert m and all(np.isfinite(float(v)) for v in m.groups())
    saved = torch.load(tmp_path / "bestpsnr_swinir_finetune_X2.pt", map_location="cpu", weights_only=False)["args"]
    assert saved["degrade_tables"] == "device" and saved["degrade"] == degrade[1]
