"""What is built on the two entries of DESIGN 7r: ops.degrade_second_order with resize rules per sample, DeviceHR2Pool(usm=) and
SynthLRBatches(usm=), and both command lines end to end.  Shapes: s 2, P 16, m 4, E 48, B 4.

Chain: torch.equal to the per-sample composition of the dense and ragged ops; with all-zero modes, to the function without the field.
Pool: the HR patch is the window of ops.usm_sharpen(window), the LR patch the window of the chain on it, clamped corners included;
usm=None and default modes give the bits of the pool without them from the same `random` state."""
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

S, P, M = 2, 16, 4
E = S * (P + 2 * M)


def _params(modes):
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd.ops import SecondOrder
    g = bk.gaussian(9, 1.4, 0.7, 0.4)
    ps = [SecondOrder(g, 1.3, (0.02, 0.0), False, 60, bk.sinc(1.8, 7), 0.9, (0.03, 0.01), True, 45, False, bk.sinc(2.2, 13), 11),
          SecondOrder(bk.sinc(1.5, 11), 0.4, (0.01, 0.02), True, 90, bk.delta(), 1.2, (0.05, 0.0), False, 30, True, bk.delta(), 12),
          SecondOrder(bk.plateau(7, 1.0, 2.0, 1.0, 1.5), 1.0, (0.0, 0.0), False, 35, g, 1.0, (0.02, 0.0), False, 95, True, bk.sinc(3.0, 21), 13),
          SecondOrder(g, 0.7, (0.04, 0.0), False, 75, bk.gaussian(5, 0.8, 0.8), 0.55, (0.0, 0.0), True, 50, False, bk.sinc(1.0, 7), 2 ** 63 + 5)]
    return [p._replace(modes=m) for p, m in zip(ps, modes)]


def _resize1(x1, size, mode, q=0):
    """One sample through the dense form of the rule."""
    from tpu_superresolution_amd import ops
    return ops.resize_aa(x1, size, q) if mode == 0 else ops.resize_ragged(x1, None, None, [mode], size, q)


def _compose(x1, s, p, sub=False):
    from tpu_superresolution_amd import ops
    H, W = x1.shape[-2:]
    z1, z2, zo = ops.second_order_sizes(H, W, s, p)
    i1, i2 = ops.second_order_noise_ids(p)
    a = ops.filter2d(x1, p.k1)
    a = _resize1(a, z1, p.modes[0])
    a = ops.noise(a, p.noise1, [i1], p.gray1)
    a = ops.jpeg_roundtrip(a, p.q1, sub)
    a = ops.filter2d(a, p.k2)
    a = _resize1(a, z2, p.modes[1])
    a = ops.noise(a, p.noise2, [i2], p.gray2)
    if not p.jpeg_last:
        a = ops.jpeg_roundtrip(a, p.q2, sub)
    a = _resize1(a, zo, p.modes[2])
    a = ops.filter2d(a, p.k3, quant_bits=8)
    return ops.jpeg_roundtrip(a, p.q2, sub) if p.jpeg_last else a


@pytest.mark.parametrize("C", [3, 1])
def test_chain_with_mixed_modes_is_the_composition(C):
    from tpu_superresolution_amd import ops
    x = torch.from_numpy(np.random.RandomState(60 + C).rand(4, C, E, E).astype(np.float32)).cuda()
    ps = _params([(1, 2, 0), (2, 0, 1), (0, 0, 0), (2, 1, 2)])
    got = ops.degrade_second_order(x, S, ps)
    for b, p in enumerate(ps):
        assert torch.equal(got[b:b + 1], _compose(x[b:b + 1], S, p)), f"C={C}: sample {b} differs from the composition"
        assert torch.equal(got[b:b + 1], ops.degrade_second_order(x[b:b + 1], S, [p]))
    zero = _params([(0, 0, 0)] * 4)
    legacy = [ops.SecondOrder(*p[:13]) for p in zero]
    want = ops.degrade_second_order(x, S, legacy)
    assert torch.equal(ops.degrade_second_order(x, S, zero), want)
    assert not torch.equal(got, want), "the modes changed nothing"
    for b in range(4):          # the all-cubic chain is the composition over ops.resize_aa alone, as before
        assert torch.equal(want[b:b + 1], _compose(x[b:b + 1], S, legacy[b]))
    with pytest.raises(ValueError):
        ops.degrade_second_order(x, S, _params([(0, 0, 3)] * 4))


def _images():
    rng = np.random.RandomState(70)
    return [rng.randint(0, 256, size=(E + 7, E + 20, 3), dtype=np.uint8), rng.randint(0, 256, size=(E + 1, E, 1), dtype=np.uint8),
            rng.randint(0, 65536, size=(2 * E, E + 33, 3)).astype(np.uint16)]


def _pool(images, seed=3, prob=None, **kw):
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHR2Pool, SecondOrderSpec
    spec = SecondOrderSpec(seed=seed) if prob is None else SecondOrderSpec(seed=seed, resize_mode_prob=prob)
    return DeviceHR2Pool(images, P, S, spec, DegradeSpec(seed=seed), margin=M, **kw)


def test_pool_with_usm_cuts_windows_of_the_sharpened_window():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.augment import dihedral
    from tpu_superresolution_amd.sr_datasets import UsmSpec
    images, idx = _images(), [0, 1, 2, 0]
    usm = UsmSpec(weight=0.8, threshold=4.0)
    a, b = _pool(images, prob=(0.3, 0.3, 0.4), usm=usm, augment="d4"), _pool(images, prob=(0.3, 0.3, 0.4), usm=usm, augment="d4")
    clamped, modes = 0, set()
    for step in range(3):
        random.seed(100 + step)
        lr, hr = a.sample(idx)
        random.seed(100 + step)
        hd, codes = b.draw(idx)
        wd, offs, params = b.draw_second_order(hd)
        clamped += sum(o != (M, M) for o in offs)
        modes |= {m for p in params for m in p.modes}
        win = ops.usm_sharpen(b._crop(b.pool, wd, E), 50, 0.0, 0.8, 4.0)
        whole = ops.degrade_second_order(win, S, params)
        want_lr = torch.stack([whole[k, :, oy:oy + P, ox:ox + P] for k, (oy, ox) in enumerate(offs)])
        want_hr = torch.stack([win[k, :, oy * S:(oy + P) * S, ox * S:(ox + P) * S] for k, (oy, ox) in enumerate(offs)])
        ops_t = torch.tensor(codes, dtype=torch.int32).cuda()
        assert torch.equal(hr, dihedral(want_hr, ops_t) if any(codes) else want_hr)
        assert torch.equal(lr, dihedral(want_lr, ops_t) if any(codes) else want_lr)
        assert not torch.equal(want_hr, torch.stack([b._crop(b.pool, wd, E)[k, :, oy * S:(oy + P) * S, ox * S:(ox + P) * S]
                                                     for k, (oy, ox) in enumerate(offs)])), "the sharpening changed nothing"
    assert clamped > 0, "no patch of this test clamped its window: the corner case is not covered"
    assert modes == {0, 1, 2}


def test_pool_without_the_options_is_the_pool_of_before():
    """usm=None and the default modes: the bits of a pool whose chain never sees the field, from the same `random` state."""
    from tpu_superresolution_amd import ops
    images, idx = _images(), [0, 1, 2, 0]
    a, b = _pool(images, augment="d4"), _pool(images, augment="d4")
    for step in range(2):
        random.seed(200 + step)
        lr, hr = a.sample(idx)
        random.seed(200 + step)
        hd, codes = b.draw(idx)
        wd, offs, params = b.draw_second_order(hd)
        assert all(p.modes == (0, 0, 0) for p in params)
        from tpu_superresolution_amd.augment import dihedral
        whole = ops.degrade_second_order(b._crop(b.pool, wd, E), S, [ops.SecondOrder(*p[:13]) for p in params])
        want_lr = torch.stack([whole[k, :, oy:oy + P, ox:ox + P] for k, (oy, ox) in enumerate(offs)])
        want_hr = b._crop(b.pool, hd, P * S)
        ops_t = torch.tensor(codes, dtype=torch.int32).cuda()
        assert torch.equal(lr, dihedral(want_lr, ops_t) if any(codes) else want_lr)
        assert torch.equal(hr, dihedral(want_hr, ops_t) if any(codes) else want_hr)
    # a non-default resize_mode_prob moves neither the crops nor the 23-variate stream
    random.seed(9)
    p0 = _pool(images).draw_second_order(_pool(images).draw(idx)[0])
    random.seed(9)
    p1 = _pool(images, prob=(0.5, 0.5, 0.0)).draw_second_order(_pool(images).draw(idx)[0])
    assert p0[0] == p1[0] and p0[1] == p1[1]
    for x, y in zip(p0[2], p1[2]):
        assert all((np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v) for u, v in zip(x[:13], y[:13])) and 0 not in y.modes


def test_pool_refuses_a_window_below_the_radius():
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHR2Pool, SecondOrderSpec, UsmSpec
    with pytest.raises(ValueError, match="unsharp mask"):
        DeviceHR2Pool([np.zeros((64, 64, 3), dtype=np.uint8)], 4, 2, SecondOrderSpec(), DegradeSpec(), margin=2, usm=UsmSpec())
    with pytest.raises(ValueError, match="UsmSpec"):
        DeviceHR2Pool([np.zeros((64, 64, 3), dtype=np.uint8)], 4, 2, SecondOrderSpec(), DegradeSpec(), margin=2, usm=0.5)


def test_whole_images_are_sharpened_then_degraded():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, SecondOrderSpec, SynthLRBatches, UsmSpec, stage1_table
    g = torch.Generator().manual_seed(0)
    hr = torch.randint(0, 256, (2, 3, 49, 66), generator=g).float() / 255.0
    spec, deg, usm = SecondOrderSpec(resize_mode_prob=(0.5, 0.5, 0.0)), DegradeSpec(), UsmSpec()
    (lr, sharp), = list(SynthLRBatches([hr], 2, 8, "cuda", degrade=deg, second_order=spec, usm=usm))
    want = ops.usm_sharpen(hr[..., :48, :66].contiguous().cuda())
    assert torch.equal(sharp, want) and not torch.equal(sharp.cpu(), hr[..., :48, :66])
    fx = deg.fixed()
    ps = [spec.fixed(stage1_table(fx.blur), fx.noise, False, i) for i in range(2)]
    assert all(p.modes == (0, 0, 0) for p in ps) and torch.equal(lr, ops.degrade_second_order(want, 2, ps))
    (lr0, hr0), = list(SynthLRBatches([hr], 2, 8, "cuda", degrade=deg, second_order=spec))
    assert torch.equal(hr0.cpu(), hr[..., :48, :66]) and not torch.equal(lr0, lr)


# ---- the command lines ------------------------------------------------------------------------------------------------------------------
SIZE = 96


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = str(tmp_path_factory.mktemp("usm_script") / "data")
    rs = np.random.RandomState(0)
    for split in ("train", "valid", "test"):
        d = os.path.join(r, "shuffled2D", f"shuffled2D_{split}_HR")
        os.makedirs(d)
        for i in range(4):
            base = (rs.rand(SIZE // 4 + 1, SIZE // 4 + 1, 3) * 255).astype(np.uint8)
            Image.fromarray(base).resize((SIZE, SIZE), Image.BICUBIC).save(os.path.join(d, f"{i:04d}.png"))
    return r


def test_finetune_with_gt_usm_then_evaluate(root, tmp_path, capsys, monkeypatch):
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", root, "--scale", "X2", "--workers", "0", "--epochs", "1", "--batch_size", "2", "--lr_patch", "16", "--gpu_data",
            "--synth_lr", "--degrade", "second_order", "--gt_usm", "--resize_mode_prob", "0.3", "0.3", "0.4", "--window_size", "4", "--graph"])
    out = capsys.readouterr().out
    assert "[degrade] gt_usm: the HR window is unsharp-masked (51 taps" in out and "[degrade] resize rules: area / bilinear / bicubic" in out
    m = re.search(r"\[X2\] epoch 001/1 .*train L1=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB \[against the USM-sharpened target\]", out)
    assert m and all(np.isfinite(float(v)) for v in m.groups())
    ck = tmp_path / "bestpsnr_swinir_finetune_X2.pt"
    saved = torch.load(ck, map_location="cpu", weights_only=False)["args"]
    assert saved["gt_usm"] is True and saved["resize_mode_prob"] == [0.3, 0.3, 0.4] and "usm_weight" not in saved and "usm_radius" not in saved
    ev = ["--scale", "X2", "--data_root", root, "--ckpt", str(ck), "--batch_size", "2", "--arch", "swinir", "--window_size", "4", "--device", "cuda",
          "--synth_lr", "--degrade", "second_order"]
    plain = evaluate.main(ev)
    capsys.readouterr()
    res = evaluate.main(ev + ["--gt_usm"])
    text = capsys.readouterr().out
    assert "[degrade] gt_usm: HR is unsharp-masked (51 taps" in text and re.search(r"\[done\] test PSNR: [0-9.]+ dB", text)
    assert np.isfinite(res["psnr"]) and res["n"] == 4 and res["bicubic_psnr"] != plain["bicubic_psnr"]
