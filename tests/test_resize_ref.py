"""Pins tests/resize_ref.py (the fp64 restatement the device tests compare against) to the two public implementations of the convention,
shows that each of its three defining choices matters, and checks the host logic of --synth_lr.  No GPU."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import resize_ref as R

# (H, W, Ho, Wo): integer /2, /3 and /4, non-integer ratios, x2, x4, identity -- and the shapes of the device cases
TORCH_SHAPES = [(16, 24, 8, 12), (18, 27, 6, 9), (32, 40, 8, 10), (33, 47, 16, 23), (20, 20, 7, 3), (7, 5, 14, 10), (13, 9, 52, 36),
                (11, 11, 11, 11)] + [c[2:] for c in R.CASES]


def _torch_aa(x, Ho, Wo):
    return F.interpolate(torch.from_numpy(x), size=(Ho, Wo), mode="bicubic", antialias=True, align_corners=False).numpy()


@pytest.mark.parametrize("H,W,Ho,Wo", TORCH_SHAPES)
def test_matches_torch_antialias_fp64(H, W, Ho, Wo):
    x = np.random.RandomState(H * 1000 + W).rand(2, 3, H, W)
    err = np.abs(R.resize(x, Ho, Wo) - _torch_aa(x, Ho, Wo)).max()
    print(f"{H}x{W}->{Ho}x{Wo}: max |ref - torch| = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("kw", [dict(a=-0.75), dict(widen=False), dict(border="clamp")], ids=["a=-0.75", "narrow-support", "clamped-border"])
def test_negative_controls_fail_the_torch_comparison(kw):
    """Each departure from the convention is far outside the 1e-12 of the test above (on a downscale, where all three differ)."""
    x = np.random.RandomState(5).rand(1, 1, 33, 47)
    assert np.abs(R.resize(x, 16, 23, **kw) - _torch_aa(x, 16, 23)).max() > 1e-3


@pytest.mark.parametrize("s", [2, 3, 4])
def test_within_one_level_of_pil(s):
    """PIL rounds to 8 bits between its two passes, so its bits are not promised: at most one level apart.  PIL also CLIPS that 8-bit
    intermediate to [0, 255], which the formula does not (full-range noise then differs by 2 levels here and there).  The negative
    lobes weigh (max sum |w| - 1) / 2 <= 0.12 per pass, so on levels 32 .. 223 no pass can leave [32 - 0.12 * 191, 223 + 0.12 * 191],
    inside [0, 255]: nothing is clipped and the rounding between the passes is all that separates the two."""
    rng = np.random.RandomState(s)
    a = rng.randint(32, 224, (24 * s, 30 * s)).astype(np.uint8)
    ref = np.rint(np.clip(R.resize(a / 255.0, 24, 30), 0, 1) * 255).astype(np.int64)
    pil = np.asarray(Image.fromarray(a, "L").resize((30, 24), Image.BICUBIC)).astype(np.int64)
    d = np.abs(ref - pil)
    print(f"/{s}: differing pixels {100.0 * (d > 0).mean():.1f} %, max {d.max()}")
    assert d.max() <= 1


def test_identity_is_exact_and_taps_are_0100():
    lo, hi, ws = R.tables(11, 11)
    for i in range(1, 9):
        assert hi[i] - lo[i] == 4 and np.array_equal(ws[i], [0.0, 1.0, 0.0, 0.0])
    x = np.random.RandomState(0).rand(1, 3, 11, 11)
    assert np.array_equal(R.resize(x, 11, 11), x)


def test_tap_counts_and_weight_norms():
    """What the kernel's table sizes and the tolerance rest on: at most 9 taps at /2, 16 at /4, 33 at /8; max sum |w| about 1.17 .. 1.24 (1.168 at /2)."""
    for s, k in ((2, 9), (4, 16), (8, 33)):
        _, _, ws = R.tables(40 * s, 40)
        assert max(len(w) for w in ws) <= k
        assert 1.16 <= max(np.abs(w).sum() for w in ws) <= 1.25
    for n_in, n_out in ((799, 100), (33, 16), (700, 175), (5, 37)):
        assert max(len(w) for w in R.tables(n_in, n_out)[2]) <= 33


@pytest.mark.parametrize("s", R.SCALES)
def test_patch_is_the_window_of_the_whole_image_downscale(s):
    imgs = R.pool_images(s)
    for k, top, left in R.pool_positions(imgs, s):
        img = R.to_unit3(imgs[k])
        H, W = img.shape[-2:]
        whole = R.resize(img[:, :H - H % s, :W - W % s], H // s, W // s)
        win = whole[:, top // s:top // s + R.PATCH, left // s:left // s + R.PATCH]
        assert np.array_equal(R.patch(img, top, left, R.PATCH, s), win)


def test_quantisation_ties_stay_under_the_cap_on_the_chosen_seeds():
    """tests/test_gpu_resize.py lets either level pass where the reference lies within the bound of a half-integer, for at most 1 % of a
    case: the reference alone must stay under that cap on the inputs the device tests use."""
    for idx in R.QUANT_CASES:
        B, C, H, W, Ho, Wo = R.CASES[idx]
        ref = R.resize(R.case_input(idx), Ho, Wo)
        share = R.near_half(ref, R.bound(H, W, Ho, Wo, 1.0)).mean()
        print(f"{R.CASE_IDS[idx]}: {100 * share:.3f} % near a half-integer")
        assert share <= 0.01
    for s in R.SCALES:
        imgs = R.pool_images(s)
        near = []
        for k, top, left in R.pool_positions(imgs, s):
            H, W = imgs[k].shape[:2]
            ref = R.patch(R.to_unit3(imgs[k]), top, left, R.PATCH, s)
            near.append(R.near_half(ref, R.bound(H - H % s, W - W % s, H // s, W // s, 1.0)))
        share = np.mean(near)
        print(f"crop_degrade /{s}: {100 * share:.3f} % near a half-integer")
        assert share <= 0.01


def test_quant8_levels():
    v, k = R.quant8(np.array([-0.2, 0.0, 0.5 / 255 - 1e-4, 1.5 / 255 + 1e-4, 1.0, 1.7]))
    assert k.tolist() == [0, 0, 0, 2, 255, 255]
    assert v.dtype == np.float32 and np.array_equal(v, (k / np.float32(255)).astype(np.float32))


# ---- host logic ------------------------------------------------------------------------------------------------------------------------
def _hr_only_tree(root, sizes=((6, 24), (2, 24), (2, 20))):
    rng = np.random.RandomState(0)
    for (n, size), split in zip(sizes, ("train", "valid", "test")):
        d = os.path.join(root, "shuffled2D", f"shuffled2D_{split}_HR")
        os.makedirs(d)
        for i in range(n):
            Image.fromarray((rng.rand(size, size) * 255).astype(np.uint8), "L").save(os.path.join(d, f"{i:04d}.png"))


def test_argparse_synth_lr(capsys):
    from tpu_superresolution_amd import evaluate as E
    from tpu_superresolution_amd import finetune_swinir as T
    base = ["--data_root", "x", "--scale", "X2"]
    a = T.parse_args(base)
    assert a.synth_lr is False and a.synth_lr_bits == 8
    a = T.parse_args(base + ["--gpu_data", "--synth_lr", "--synth_lr_bits", "0", "--arch", "hat"])
    assert a.synth_lr and a.synth_lr_bits == 0
    for bad in (["--synth_lr"], ["--gpu_data", "--synth_lr", "--synth_lr_bits", "4"]):
        with pytest.raises(SystemExit):
            T.parse_args(base + bad)
    assert "--gpu_data" in capsys.readouterr().err
    ev = ["--scale", "X2", "--ckpt", "c"]
    assert E.parse_args(ev + ["--arch", "dat", "--synth_lr"]).synth_lr_bits == 8
    for bad in (["--synth_lr"], ["--arch", "swinir", "--synth_lr", "--synth_lr_bits", "16"]):          # ms_resunet is the default arch
        with pytest.raises(SystemExit):
            E.parse_args(ev + bad)


def test_shuffled2dhr_needs_no_lr_directory(tmp_path):
    from tpu_superresolution_amd.sr_datasets import Shuffled2DHR, Shuffled2DPaired, hr_to_tensor3
    root = str(tmp_path)
    _hr_only_tree(root)
    ds = Shuffled2DHR(root, split="train")
    assert len(ds) == 6 and ds[0].size == (24, 24)
    t = Shuffled2DHR(root, split="test", transform=hr_to_tensor3)[1]
    assert t.shape == (3, 20, 20) and t.dtype == torch.float32 and torch.equal(t[0], t[2])
    with pytest.raises(FileNotFoundError):
        Shuffled2DPaired(root, split="train", scale="X2")
    with pytest.raises(FileNotFoundError):
        Shuffled2DHR(root, split="extra")
    with pytest.raises(RuntimeError):
        Shuffled2DHR(root, split="train", exts=(".bmp",))


def test_device_hr_pool_host_side():
    """Up to the kernel call on device='cpu': packing, refusals, and crop corners / D4 codes drawn in DevicePairPool's order and ranges."""
    from tpu_superresolution_amd.sr_datasets import DeviceHRPool, DevicePairPool
    rng = np.random.RandomState(1)
    hrs = [rng.randint(0, 256, (37, 45)).astype(np.uint8), rng.randint(0, 256, (40, 32, 3)).astype(np.uint8),
           rng.randint(0, 65536, (33, 33)).astype(np.uint16)]
    s, P = 2, 8
    pool = DeviceHRPool(hrs, P, s, device="cpu", augment="d4")
    assert len(pool) == 3 and pool.num_shards == 1 and pool.shard_of(2) == 0
    assert pool.pool.numel() == 37 * 45 + 40 * 32 * 3 + 1 + 33 * 33 * 2          # HR bytes only; the u16 image starts at an even byte
    pairs = [(np.zeros((a.shape[0] // s, a.shape[1] // s), np.uint8), a) for a in hrs]
    pair_pool = DevicePairPool(pairs, P, s, device="cpu", augment="d4")
    random.seed(7)
    hd, codes = pool.draw([0, 1, 2, 1])
    random.seed(7)
    want = []
    for i in (0, 1, 2, 1):
        _, (_, lh, lw, _), _ = pair_pool.meta[i]
        top, left = random.randint(0, lh - P), random.randint(0, lw - P)
        want.append((top * s, left * s, random.randrange(8)))
    assert [(d[4], d[5], c) for d, c in zip(hd, codes)] == want
    assert [d[:4] for d in hd] == [pool.meta[i][1] for i in (0, 1, 2, 1)]
    two = DeviceHRPool(hrs, P, s, device="cpu", shard_bytes=6000)
    assert two.num_shards == 2 and [two.shard_of(i) for i in range(3)] == [0, 0, 1]
    with pytest.raises(ValueError):
        two._batch_pool([0, 2])
    for bad in (dict(scale=5), dict(scale=1), dict(quant_bits=4), dict(augment="rot")):
        with pytest.raises(ValueError):
            DeviceHRPool(hrs, P, **{"scale": s, "device": "cpu", **bad})
    with pytest.raises(ValueError):
        DeviceHRPool(hrs, 17, s, device="cpu")          # 33 // 2 = 16 < 17
    with pytest.raises(ValueError):
        DeviceHRPool([], P, s, device="cpu")
    with pytest.raises(ValueError):
        DeviceHRPool([np.zeros((20, 20), np.float32)], P, s, device="cpu")
