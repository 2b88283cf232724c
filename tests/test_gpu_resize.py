"""srk_resize_aa_f32 / srk_crop_degrade_u8 (csrc/resize.hip) and what is built on them: ops.resize_aa, sr_datasets.DeviceHRPool and the
--synth_lr command lines.  The reference is tests/resize_ref.py (fp64 numpy, pinned against F.interpolate(antialias=True) and PIL in
tests/test_resize_ref.py).

Tolerance (resize_ref.bound, derived, not tuned): 2 (Ky + Kx + 4) u Ly Lx max|x| with u = 2^-24, K the largest tap count and L the
largest sum |w| of each axis from the reference's own tables -- the project's 2 K u S rule for a K-term fp32 dot product, plus one
rounding per weight (fp64 -> fp32).  Everything that can be exact is compared with torch.equal: identity, the HR patch against
srk_paired_crop_u8, a training patch against the window of the whole-image resize, the pool against DevicePairPool."""
import functools
import random

import numpy as np
import pytest
import torch

import resize_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _resize(x, out, B, C, H, W, Ho, Wo, q=0):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_resize_aa_f32(_ptr(x), _ptr(out), B, C, H, W, Ho, Wo, q, _stream())


def _degrade(pool, desc, lr, hr, B, P, s, q=0):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_crop_degrade_u8(_ptr(pool), _ptr(desc), _ptr(lr), _ptr(hr), B, P, s, q, _stream())


@functools.lru_cache(maxsize=None)
def _case(idx, lo=0.0, hi=1.0):
    """(input fp32, fp64 reference, bound) of R.CASES[idx]; computed once and shared."""
    B, C, H, W, Ho, Wo = R.CASES[idx]
    x = R.case_input(idx, lo, hi)
    return x, R.resize(x, Ho, Wo), R.bound(H, W, Ho, Wo, float(np.abs(x).max()))


def _run_resize(x, Ho, Wo, q=0):
    B, C, H, W = x.shape
    n = B * C * Ho * Wo
    out = Guarded("f32", 1, n, n)
    assert _resize(torch.from_numpy(x).cuda(), out.ptr, B, C, H, W, Ho, Wo, q) == 0
    torch.cuda.synchronize()
    out.assert_guards(f"resize_aa {x.shape} -> {(Ho, Wo)}")
    return out.data().reshape(B, C, Ho, Wo)


def _check_quantised(got, ref, bnd, what):
    """Every value is k / 255.0f exactly; k is the reference's level, except where 255 x the reference's unquantised value lies within
    255 x bound of a half-integer, where either neighbouring level passes -- for at most 1 % of the case."""
    got = np.asarray(got, dtype=np.float32)
    k = np.rint(got.astype(np.float64) * 255.0)
    assert np.array_equal(got, (k.astype(np.float32) / np.float32(255)).astype(np.float32)), f"{what}: values that are not k / 255.0f"
    level = R.quant8(ref)[1]
    near = R.near_half(ref, bnd)
    print(f"{what}: {int((k != level).sum())} levels differ from the reference, {100.0 * near.mean():.3f} % of the case near a half-integer")
    assert near.mean() <= 0.01, what
    wrong = (k != level) & ~(near & (np.abs(k - level) <= 1))
    assert not wrong.any(), f"{what}: {int(wrong.sum())} levels differ from the reference away from a half-integer"


# ---- srk_resize_aa_f32 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,lo,hi", [(i, 0.0, 1.0) for i in range(len(R.CASES))] + [(4, -3.0, 3.0)],
                         ids=R.CASE_IDS + [R.CASE_IDS[4] + "-in-3..3"])
def test_resize_direct(idx, lo, hi):
    B, C, H, W, Ho, Wo = R.CASES[idx]
    x, ref, bnd = _case(idx, lo, hi)
    got = _run_resize(x, Ho, Wo).numpy()
    err = float(np.abs(got - ref).max())
    print(f"{R.CASE_IDS[idx]} [{lo}, {hi}): max |err| = {err:.3e}, bound = {bnd:.3e}")
    assert err <= bnd
    if (H, W) == (Ho, Wo):
        assert np.array_equal(got, x), "identity must return the input's values"


def test_resize_nan_footprint():
    idx, (b, c, y, x0) = 4, (0, 1, 10, 20)
    B, C, H, W, Ho, Wo = R.CASES[idx]
    x, ref, bnd = _case(idx)
    x = x.copy()
    x[b, c, y, x0] = np.nan
    got = _run_resize(x, Ho, Wo).numpy()
    want = np.zeros((B, C, Ho, Wo), dtype=bool)
    want[b, c] = R.nan_footprint(H, W, Ho, Wo, y, x0)
    assert 0 < want.sum() < Ho * Wo
    assert np.array_equal(np.isnan(R.resize(x, Ho, Wo)), want)          # the reference itself spreads the NaN over that footprint
    assert np.array_equal(np.isnan(got), want)
    assert np.abs(got - ref)[~want].max() <= bnd


def test_resize_error_codes_and_the_8x_limit():
    from tpu_superresolution_amd._lib import lib
    x = torch.rand(1, 2, 16, 24, device="cuda")
    n = 2 * 8 * 12
    out = Guarded("f32", 1, n, n)
    assert _resize(None, out.ptr, 1, 2, 16, 24, 8, 12) == E_NULL
    assert _resize(x, None, 1, 2, 16, 24, 8, 12) == E_NULL
    for shape in ((0, 2, 16, 24, 8, 12), (1, 0, 16, 24, 8, 12), (1, 2, 0, 24, 8, 12), (1, 2, 16, -1, 8, 12), (1, 2, 16, 24, 0, 12),
                  (1, 2, 16, 24, 8, 0)):
        assert _resize(x, out.ptr, *shape) == E_SHAPE, shape
    assert _resize(x, out.ptr, 1, 2, 16, 24, 8, 12, 4) == E_SHAPE and b"quant_bits" in lib().srk_last_error()
    assert _resize(out.ptr, out.ptr, 1, 2, 8, 12, 8, 12) == E_SHAPE and b"overlap" in lib().srk_last_error()
    assert _resize(out.ptr - 4 * (2 * 16 * 24 - 1), out.ptr, 1, 2, 16, 24, 8, 12) == E_SHAPE          # windows sharing four bytes
    assert _resize(out.ptr + 4 * (n - 1), out.ptr, 1, 2, 16, 24, 8, 12) == E_SHAPE
    assert _resize(x, out.ptr, 1, 2, 16, 24, 8, 2) == E_UNSUPPORTED and b"8x" in lib().srk_last_error()          # 24 -> 2
    assert _resize(x, out.ptr, 1, 2, 16, 24, 1, 12) == E_UNSUPPORTED                                                # 16 -> 1
    torch.cuda.synchronize()
    out.assert_untouched("the output of a refused call")
    # exactly 8x is the widest footprint that is served
    xs = np.random.RandomState(9).rand(1, 1, 40, 136).astype(np.float32)
    got = _run_resize(xs, 5, 17).numpy()
    assert np.abs(got - R.resize(xs, 5, 17)).max() <= R.bound(40, 136, 5, 17, 1.0)


def test_resize_aa_python_entry():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd._lib import SrkUnsupported
    x, ref, bnd = _case(3)
    xd = torch.from_numpy(x).cuda()
    y = ops.resize_aa(xd, (6, 9))
    assert y.shape == (2, 3, 6, 9) and np.abs(y.cpu().numpy() - ref).max() <= bnd
    out = torch.empty_like(y)
    assert ops.resize_aa(xd, [6, 9], out=out) is out and torch.equal(out, y)
    for bad in (dict(size=(6,)), dict(size=(0, 9)), dict(size=(6, 9), quant_bits=4), dict(size=(6, 9), out=torch.empty(2, 3, 6, 8, device="cuda")),
                dict(size=(6, 9), out=out.double())):
        with pytest.raises(ValueError):
            ops.resize_aa(xd, **bad)
    with pytest.raises(ValueError):
        ops.resize_aa(xd[0], (6, 9))
    with pytest.raises(ValueError):
        ops.resize_aa(xd.half(), (6, 9))
    with pytest.raises(SrkUnsupported):
        ops.resize_aa(xd, (1, 9))
    lr, hr = ops.degrade_aa(xd, 4)
    assert hr.shape == (2, 3, 12, 16) and torch.equal(hr, xd[..., :12, :16]) and torch.equal(lr, ops.resize_aa(hr, (3, 4), 8))


@pytest.mark.parametrize("idx", R.QUANT_CASES, ids=[R.CASE_IDS[i] for i in R.QUANT_CASES])
def test_resize_quantised(idx):
    B, C, H, W, Ho, Wo = R.CASES[idx]
    x, ref, bnd = _case(idx)
    _check_quantised(_run_resize(x, Ho, Wo, 8).numpy(), ref, bnd, R.CASE_IDS[idx])


# ---- srk_crop_degrade_u8 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_case(s):
    """The pool of R.pool_images(s) on the device (packed by DeviceHRPool), its descriptors, and per sample: the window of ops.resize_aa
    on the converted, cropped whole image (quant_bits 0 and 8), the fp64 reference patch and its bound."""
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import DeviceHRPool
    imgs = R.pool_images(s)
    pool = DeviceHRPool(imgs, R.PATCH, s)
    pos = R.pool_positions(imgs, s)
    desc = torch.tensor([pool.meta[k][1] + (top, left) for k, top, left in pos], dtype=torch.int64).cuda()
    whole = {}
    for k, a in enumerate(imgs):
        H, W = a.shape[:2]
        reg = torch.from_numpy(R.to_unit3(a)[None, :, :H - H % s, :W - W % s].copy()).cuda()
        whole[k] = [ops.resize_aa(reg, (H // s, W // s), q) for q in (0, 8)]
    P = R.PATCH
    win = [torch.cat([whole[k][q][:, :, top // s:top // s + P, left // s:left // s + P] for k, top, left in pos]) for q in (0, 1)]
    ref = np.stack([R.patch(R.to_unit3(imgs[k]), top, left, P, s) for k, top, left in pos])
    bnd = np.array([R.bound(imgs[k].shape[0] // s * s, imgs[k].shape[1] // s * s, imgs[k].shape[0] // s, imgs[k].shape[1] // s, 1.0)
                    for k, _, _ in pos])
    return pool, pos, desc, win, ref, bnd


def _run_degrade(s, q):
    pool, pos, desc, _, _, _ = _pool_case(s)
    B, P = len(pos), R.PATCH
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 3 * P * P * s * s, B * 3 * P * P * s * s)
    assert _degrade(pool.pool, desc, lr.ptr, hr.ptr, B, P, s, q) == 0
    torch.cuda.synchronize()
    lr.assert_guards(f"crop_degrade /{s} lr_out")
    hr.assert_guards(f"crop_degrade /{s} hr_out")
    return lr.win.view(B, 3, P, P), hr.win.view(B, 3, P * s, P * s)


@pytest.mark.parametrize("s", R.SCALES)
def test_crop_degrade_direct(s):
    from tpu_superresolution_amd._lib import lib
    pool, pos, desc, win, ref, bnd = _pool_case(s)
    B, P = len(pos), R.PATCH
    lr, hr = _run_degrade(s, 0)
    # the HR patch: bit-identical to srk_paired_crop_u8 (its LR side reads the same image at (top / s, left / s), which is inside it)
    ld = desc.clone()
    ld[:, 4:] //= s
    lr2, hr2 = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
    assert lib().srk_paired_crop_u8(pool.pool.data_ptr(), ld.data_ptr(), desc.data_ptr(), lr2.data_ptr(), hr2.data_ptr(), B, P, s, _stream()) == 0
    assert torch.equal(hr, hr2)
    # the LR patch: bit-identical to the window of the whole-image resize, and within the bound of the reference
    assert torch.equal(lr, win[0])
    err = np.abs(lr.cpu().numpy() - ref).reshape(B, -1).max(axis=1)
    print(f"/{s}: max |err| / bound per sample = {np.round(err / bnd, 3).tolist()}")
    assert (err <= bnd).all()
    gray = [i for i, (k, _, _) in enumerate(pos) if k in (0, 2)]
    assert torch.equal(lr[gray, 0], lr[gray, 1]) and torch.equal(lr[gray, 0], lr[gray, 2])


@pytest.mark.parametrize("s", R.SCALES)
def test_crop_degrade_quantised(s):
    _, pos, _, win, ref, bnd = _pool_case(s)
    lr, _ = _run_degrade(s, 8)
    assert torch.equal(lr, win[1])
    _check_quantised(lr.cpu().numpy(), ref, bnd.reshape(-1, 1, 1, 1), f"crop_degrade /{s}")


def test_crop_degrade_error_codes():
    pool, pos, desc, _, _, _ = _pool_case(2)
    B, P = len(pos), R.PATCH
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 12 * P * P, B * 12 * P * P)
    for args in ((None, desc, lr.ptr, hr.ptr), (pool.pool, None, lr.ptr, hr.ptr), (pool.pool, desc, None, hr.ptr), (pool.pool, desc, lr.ptr, None)):
        assert _degrade(*args, B, P, 2) == E_NULL
    for b, p, s, q in ((0, P, 2, 0), (65536, P, 2, 0), (B, 0, 2, 0), (B, 4096, 2, 0), (B, P, 1, 0), (B, P, 5, 0), (B, P, 2, 4), (B, P, 2, 16)):
        assert _degrade(pool.pool, desc, lr.ptr, hr.ptr, b, p, s, q) == E_SHAPE, (b, p, s, q)
    torch.cuda.synchronize()
    lr.assert_untouched("lr_out of a refused call")
    hr.assert_untouched("hr_out of a refused call")


# ---- DeviceHRPool ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", ["none", "d4"])
def test_device_hr_pool_against_pair_pool_and_window_reference(augment):
    from tpu_superresolution_amd.augment import apply_op_host
    from tpu_superresolution_amd.sr_datasets import DeviceHRPool, DevicePairPool
    s, P = 2, R.PATCH
    imgs = R.pool_images(s)
    hr_pool = DeviceHRPool(imgs, P, s, augment=augment)
    pair_pool = DevicePairPool([(np.zeros((a.shape[0] // s, a.shape[1] // s), np.uint8), a) for a in imgs], P, s, augment=augment)
    sharded = DeviceHRPool(imgs, P, s, augment=augment, shard_bytes=11000)
    assert sharded.num_shards == 2 and [sharded.shard_of(i) for i in range(4)] == [0, 0, 1, 1]
    from tpu_superresolution_amd import ops
    for batch in ([0, 1, 1, 0, 0], [2, 3, 2]):
        random.seed(11)
        hd, codes = hr_pool.draw(batch)
        random.seed(11)
        lr, hr = hr_pool.sample(batch)
        state = random.getstate()
        random.seed(11)
        _, hr_pair = pair_pool.sample(batch)
        assert random.getstate() == state, "both pools must consume `random` alike"
        assert torch.equal(hr, hr_pair)
        assert augment == "none" or any(codes)
        for b, (d, code) in enumerate(zip(hd, codes)):
            a = imgs[batch[b]]
            H, W = a.shape[:2]
            reg = torch.from_numpy(R.to_unit3(a)[None, :, :H - H % s, :W - W % s].copy()).cuda()
            win = ops.resize_aa(reg, (H // s, W // s), 8)[0, :, d[4] // s:d[4] // s + P, d[5] // s:d[5] // s + P]
            assert torch.equal(lr[b], apply_op_host(win, code)), (batch, b, code)
        random.seed(11)
        lr2, hr2 = sharded.sample(batch)
        assert torch.equal(lr2, lr) and torch.equal(hr2, hr)
    with pytest.raises(ValueError, match="one shard"):
        sharded.sample([1, 2])


# ---- the command lines -------------------------------------------------------------------------------------------------------------------
def _make_hr_only_dataset(root, lr=72, scale=4):
    """The tree of test_gpu_dihedral._make_dataset without its LR directories."""
    import os

    from PIL import Image
    rng = np.random.RandomState(0)
    for split, n, size in (("train", 6, lr), ("valid", 2, lr), ("test", 2, 40)):
        hr_dir = os.path.join(root, "shuffled2D", f"shuffled2D_{split}_HR")
        os.makedirs(hr_dir)
        for i in range(n):
            Image.fromarray((rng.rand(size * scale, size * scale) * 255).astype(np.uint8), "L").save(os.path.join(hr_dir, f"{i:04d}.png"))


def test_scripts_train_and_evaluate_from_hr_only(tmp_path, capsys, monkeypatch):
    import re

    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    root = str(tmp_path / "data")
    _make_hr_only_dataset(root)
    monkeypatch.chdir(tmp_path)
    base = ["--data_root", root, "--scale", "X4", "--workers", "0", "--lr", "1e-4", "--gpu_data"]
    with pytest.raises(FileNotFoundError):          # the control: without the flag the LR set is still required
        F.main(base + ["--epochs", "1", "--batch_size", "2"])
    capsys.readouterr()
    F.main(base + ["--synth_lr", "--epochs", "1", "--batch_size", "2"])
    out = capsys.readouterr().out
    assert "[synth_lr] 6 HR images" in out and "[done] best_val_loss=" in out
    m = re.search(r"\[X4\] epoch 001/1 .*train L1=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB", out)
    assert m and all(np.isfinite(float(v)) for v in m.groups())
    for name in ("best_swinir_finetune_X4.pt", "bestpsnr_swinir_finetune_X4.pt"):
        args = torch.load(tmp_path / name, map_location="cpu", weights_only=False)["args"]
        assert args["synth_lr"] is True and "synth_lr_bits" not in args          # the default 8 leaves no trace
    res = evaluate.main(["--scale", "X4", "--data_root", root, "--ckpt", str(tmp_path / "bestpsnr_swinir_finetune_X4.pt"), "--batch_size", "1",
                         "--save_dir", str(tmp_path / "p"), "--save_n", "1", "--arch", "swinir", "--device", "cuda", "--synth_lr"])
    assert "[synth_lr]" in capsys.readouterr().out
    assert np.isfinite(res["psnr"]) and np.isfinite(res["ssim"]) and res["n"] == 2
