"""srk_jpeg_roundtrip_f32 (csrc/jpeg.hip) and what is built on it: ops.jpeg_roundtrip, sr_datasets.JpegSpec with DeviceHRPool(jpeg=) and
SynthLRBatches(jpeg=), and the --jpeg_quality command lines.  The reference is tests/jpeg_ref.py (pinned in tests/test_jpeg_ref.py).

Stage A compares the quantised coefficients (the coef_out port): a coefficient whose c / Q lies farther than 2 (8 + 8 + 4) u S / Q from
a half-integer is decided and must equal the reference; the others may differ by 1.  Stage B decodes THE DEVICE'S coefficients in the
reference: a pixel whose component values after the inverse DCT all lie farther than 2 (8 + 8 + 4) u S' from a half-integer is decided
and must have exactly the reference's level / 255.0f (the colour chains are restated bit for bit, so they add no bound); an undecided
pixel may differ by 1 level (gray) or 3 (colour: one level of Cb moves B by 1.772).  Blocks that keep only their DC term are restated
bit for bit in the reference (they decode to exactly x.5 whenever k Q = 4 mod 8) and count as decided.  tests/test_jpeg_ref.py caps the undecided shares
of these very inputs at 2 % and 1 %."""
import random

import numpy as np
import pytest
import torch

import jpeg_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL = -1, -2
CASES = list(R.cases())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _raw(x, out, q, B, C, H, W, sub, coef=None):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_jpeg_roundtrip_f32(_ptr(x), _ptr(out), _ptr(q), B, C, H, W, sub, _ptr(coef), _stream())


def _run(x, qs, sub, with_coef=True):
    """-> (out [B,C,H,W] on the device, coef int16 [B,C,Hm,Wm] | None), with the guards checked"""
    B, C, H, W = x.shape
    m = 16 if (sub and C == 3) else 8
    g = Guarded("f32", B * C * H, W, W)
    q = torch.tensor(qs, dtype=torch.int32).cuda()
    coef = torch.full((B, C, R.mcu_extent(H, m), R.mcu_extent(W, m)), R.SENTINEL, dtype=torch.int16).cuda() if with_coef else None
    assert _raw(x, g.ptr, q, B, C, H, W, sub, coef) == 0
    torch.cuda.synchronize()
    g.assert_guards(f"jpeg_roundtrip {tuple(x.shape)} sub={sub}")
    return g.win.view(B, C, H, W).clone(), coef


@pytest.mark.parametrize("C,H,W,sub", CASES)
def test_coefficients_then_pixels_against_the_reference(C, H, W, sub):
    xn = R.make_batch(C, H, W)
    x = torch.from_numpy(xn).cuda()
    out, coef = _run(x, R.QUALITIES, sub)
    out_n, coef_n = out.cpu().numpy(), coef.cpu().numpy()
    for b, q in enumerate(R.QUALITIES):
        if q == 0:          # passed through bit for bit, NaNs included; no coefficient written
            assert np.array_equal(out_n[b].view(np.uint32), xn[b].view(np.uint32)) and (coef_n[b] == R.SENTINEL).all()
            continue
        ref = R.roundtrip(xn[b], q, sub)
        assert (coef_n[b][~ref.coef_valid] == R.SENTINEL).all(), "coef_out was written outside its stated part"
        assert (coef_n[b][ref.coef_valid] != R.SENTINEL).all(), "a coefficient was not written"
        diff = np.abs(coef_n[b].astype(np.int64) - ref.coef)[ref.coef_valid]
        dec = ref.coef_decided[ref.coef_valid]
        print(f"b={b} q={q}: coefficients {dec.size}, undecided {(~dec).sum()}, of them different {(diff[~dec] != 0).sum()}")
        assert (diff[dec] == 0).all(), f"b={b} q={q}: {(diff[dec] != 0).sum()} decided coefficients differ (max {diff[dec].max()})"
        assert (diff <= 1).all()
        dec2 = R.roundtrip(xn[b], q, sub, coef=coef_n[b])
        assert np.isfinite(out_n[b]).all()
        mask = torch.from_numpy(np.broadcast_to(dec2.pix_decided, out_n[b].shape).copy())
        got, want = out[b].cpu(), torch.from_numpy(dec2.out)
        print(f"b={b} q={q}: pixels {dec2.pix_decided.size}, undecided {(~dec2.pix_decided).sum()}")
        assert torch.equal(got[mask], want[mask]), f"b={b} q={q}: {(got[mask] != want[mask]).sum()} decided pixel values differ"
        lev = np.abs(np.rint(out_n[b].astype(np.float64) * 255) - np.rint(dec2.out.astype(np.float64) * 255))
        assert lev.max() <= (1 if C == 1 else 3)


@pytest.mark.parametrize("C,sub", [(1, 0), (3, 0), (3, 1)])
def test_exact_identities(C, sub):
    H, W = 61, 45
    xn = R.make_batch(C, H, W, seed=1)
    x = torch.from_numpy(xn).cuda()
    out, coef = _run(x, R.QUALITIES, sub)
    again, coef2 = _run(x, R.QUALITIES, sub)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)) and torch.equal(coef, coef2)          # a second launch
    no_port, _ = _run(x, R.QUALITIES, sub, with_coef=False)
    assert torch.equal(out.view(torch.int32), no_port.view(torch.int32))          # the port does not change the pixels
    for b, q in enumerate(R.QUALITIES):          # sample b of the batch = the same image alone
        alone, c1 = _run(x[b:b + 1].contiguous(), [q], sub)
        assert torch.equal(alone[0].view(torch.int32), out[b].view(torch.int32)) and torch.equal(c1[0], coef[b])
    # any other bit pattern of the quality is clamped into 0..100
    odd, _ = _run(x, [-7, 101, 1 << 30, -(1 << 31), 100], sub, with_coef=False)
    want, _ = _run(x, [0, 100, 100, 0, 100], sub, with_coef=False)
    assert torch.equal(odd.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("sub", [0, 1])
def test_aligned_window_equals_the_window_of_the_whole_image(sub):
    big = torch.from_numpy(R.make_batch(3, 96, 128, seed=2)[[0, 3]]).cuda()
    whole, _ = _run(big, [35, 80], sub, with_coef=False)
    win, _ = _run(big[:, :, 16:80, 32:96].contiguous(), [35, 80], sub, with_coef=False)
    assert torch.equal(win.view(torch.int32), whole[:, :, 16:80, 32:96].contiguous().view(torch.int32))


def test_gray_in_three_channels_stays_gray_at_444():
    g = torch.from_numpy(R.make_batch(1, 40, 56, seed=3)[[0, 1, 2]]).cuda()
    out, _ = _run(g.repeat(1, 3, 1, 1).contiguous(), [20, 60, 95], 0, with_coef=False)
    assert torch.equal(out[:, 0], out[:, 1]) and torch.equal(out[:, 0], out[:, 2])
    gray, _ = _run(g, [20, 60, 95], 0, with_coef=False)
    assert torch.equal(out[:, :1], gray)          # Cb = Cr = 128 exactly: the Y plane alone decides


def test_ops_jpeg_roundtrip_equals_the_raw_entry_and_refuses():
    from tpu_superresolution_amd import ops
    xn = R.make_batch(3, 61, 45, seed=4)
    x = torch.from_numpy(xn).cuda()
    for sub in (0, 1):
        out, coef = _run(x, R.QUALITIES, sub)
        got, gcoef = ops.jpeg_roundtrip(x, list(R.QUALITIES), subsample=bool(sub), return_coef=True)
        assert torch.equal(got.view(torch.int32), out.view(torch.int32))
        assert torch.equal(gcoef, torch.where(coef == R.SENTINEL, torch.zeros_like(coef), coef))
        assert torch.equal(ops.jpeg_roundtrip(x, list(R.QUALITIES), subsample=bool(sub)).view(torch.int32), out.view(torch.int32))
    one, _ = _run(x, [40] * 5, 0, with_coef=False)
    assert torch.equal(ops.jpeg_roundtrip(x, 40).view(torch.int32), one.view(torch.int32))
    for bad in (dict(quality=101), dict(quality=-1), dict(quality=[50] * 4), dict(quality=[50, 50, 50, 50, 101]), dict(quality=50.5),
                dict(x=x[:, :2]), dict(x=x[0]), dict(x=x.double()), dict(x=x.cpu())):
        with pytest.raises(ValueError):
            ops.jpeg_roundtrip(**{"x": x, "quality": 50, **bad})


def test_refusals_of_the_raw_entry():
    x = torch.zeros(2, 3, 16, 16, device="cuda")
    g = Guarded("f32", 2 * 3 * 16, 16, 16)
    q = torch.tensor([50, 50], dtype=torch.int32).cuda()
    ok = dict(x=x, out=g.ptr, q=q, B=2, C=3, H=16, W=16, sub=0)
    for bad, code in ((dict(x=None), E_NULL), (dict(out=None), E_NULL), (dict(q=None), E_NULL), (dict(B=0), E_SHAPE), (dict(H=0), E_SHAPE),
                      (dict(W=-1), E_SHAPE), (dict(C=2), E_SHAPE), (dict(C=0), E_SHAPE), (dict(C=4), E_SHAPE), (dict(sub=2), E_SHAPE),
                      (dict(sub=-1), E_SHAPE), (dict(out=x), E_SHAPE), (dict(out=x.data_ptr() + 4 * 16 * 16), E_SHAPE),
                      (dict(B=1 << 20, H=1 << 30, W=1 << 30), E_SHAPE), (dict(B=1 << 30, C=1, H=17, W=33), E_SHAPE)):
        assert _raw(**{**ok, **bad}) == code, bad
    torch.cuda.synchronize()
    g.assert_untouched("the output of a refused call")
    assert _raw(**ok) == 0


@pytest.mark.parametrize("augment,blind", [("none", False), ("d4", True)])
def test_device_hr_pool_jpeg_is_ops_jpeg_roundtrip_of_the_plain_batch(augment, blind):
    import resize_ref as RS
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.augment import apply_op_host, inverse_op
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool, JpegSpec
    s, Pp, q = 2, RS.PATCH, 45
    imgs = RS.pool_images(s)
    kw = dict(augment=augment, degrade=DegradeSpec(seed=21) if blind else None, rank=2)
    plain = DeviceHRPool(imgs, Pp, s, **kw)
    coded = DeviceHRPool(imgs, Pp, s, jpeg=JpegSpec(quality=(q, q), p=1.0, subsample=True, seed=3), **kw)
    never = DeviceHRPool(imgs, Pp, s, jpeg=JpegSpec(quality=(q, q), p=0.0, seed=3), **kw)
    for batch in ([0, 1, 1, 0, 0], [2, 3, 2, 1]):
        random.seed(11)
        _, codes = plain.draw(batch)
        random.seed(11)
        lr0, hr0 = plain.sample(batch)
        state = random.getstate()
        random.seed(11)
        lr, hr = coded.sample(batch)
        assert random.getstate() == state, "the jpeg stage must not consume the global `random`"
        random.seed(11)
        lr_p0, hr_p0 = never.sample(batch)
        assert torch.equal(hr, hr0) and torch.equal(hr_p0, hr0) and torch.equal(lr_p0, lr0) and not torch.equal(lr, lr0)
        # coded BEFORE the D4 transform: the grid is anchored to the patch as cut, which is T^-1 of the plain pool's patch
        assert augment == "none" or any(codes)
        cut = torch.stack([apply_op_host(lr0[b], inverse_op(code)) for b, code in enumerate(codes)])
        want = ops.jpeg_roundtrip(cut, q, subsample=True)
        for b, code in enumerate(codes):
            assert torch.equal(lr[b], apply_op_host(want[b], code)), (batch, b, code)


def test_synth_lr_batches_jpeg():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import FixedDegrade, JpegSpec, SynthLRBatches
    g = torch.Generator().manual_seed(0)
    imgs = [torch.rand(2, 3, 21, 30, generator=g), torch.rand(2, 3, 21, 30, generator=g)]
    for degrade in (None, FixedDegrade((1.2, 0.6), (0.03, 0.0))):
        plain = list(SynthLRBatches(imgs, 2, 8, "cuda", degrade=degrade))
        coded = list(SynthLRBatches(imgs, 2, 8, "cuda", degrade=degrade, jpeg=JpegSpec(quality=(30, 50), subsample=True)))
        for (lr0, hr0), (lr, hr) in zip(plain, coded):
            assert torch.equal(hr, hr0) and torch.equal(lr, ops.jpeg_roundtrip(lr0, 40, subsample=True)) and not torch.equal(lr, lr0)
        again = list(SynthLRBatches(imgs, 2, 8, "cuda", degrade=degrade, jpeg=40, jpeg_subsample=True))
        assert all(torch.equal(a[0], b[0]) for a, b in zip(coded, again))


# ---- the command lines -------------------------------------------------------------------------------------------------------------------
def test_scripts_train_and_evaluate_with_jpeg(tmp_path, capsys, monkeypatch):
    import re

    from test_gpu_resize import _make_hr_only_dataset
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    root = str(tmp_path / "data")
    _make_hr_only_dataset(root)
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", root, "--scale", "X4", "--workers", "0", "--gpu_data", "--synth_lr", "--epochs", "1", "--batch_size", "2",
            "--degrade", "blind", "--jpeg_quality", "30", "90", "--jpeg_p", "0.8", "--jpeg_subsample", "420"])
    out = capsys.readouterr().out
    assert out.count("[degrade] jpeg:") == 1 and "validation: quality 60" in out and "[done] best_val_loss=" in out
    m = re.search(r"\[X4\] epoch 001/1 .*train L1=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB", out)
    assert m and all(np.isfinite(float(v)) for v in m.groups())
    args = torch.load(tmp_path / "bestpsnr_swinir_finetune_X4.pt", map_location="cpu", weights_only=False)["args"]
    assert args["jpeg_quality"] == [30, 90] and args["jpeg_p"] == 0.8 and args["jpeg_subsample"] == "420"
    ev = ["--scale", "X4", "--data_root", root, "--ckpt", str(tmp_path / "bestpsnr_swinir_finetune_X4.pt"), "--batch_size", "1", "--save_dir",
          str(tmp_path / "p"), "--save_n", "1", "--arch", "swinir", "--device", "cuda", "--synth_lr"]
    clean = evaluate.main(ev)
    res = evaluate.main(ev + ["--jpeg_quality", "40", "--jpeg_subsample", "420", "--tile", "24", "--tile_overlap", "8", "--self_ensemble"])
    assert "[degrade] jpeg: quality 40" in capsys.readouterr().out
    assert np.isfinite(res["psnr"]) and np.isfinite(res["ssim"]) and res["n"] == 2 and res["psnr"] != clean["psnr"]
