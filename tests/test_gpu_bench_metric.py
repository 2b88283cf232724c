"""srk_bench_planes_f32 / srk_bench_psnr (csrc/metrics.hip) and what is built on them -- ops.bench_planes / ops.bench_psnr,
metrics.bench_metrics, finetune_swinir.validate_bench -- against the fp64 restatement of tests/bench_metric_ref.py
within its derived bounds.  Outputs and workspace of the direct calls sit between the guard rows of tests/guarded.py."""
import functools
import math

import numpy as np
import pytest
import torch

import bench_metric_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

# B, C, H, W, border, mode: 1 x 2 crop (PSNR only, less than one wave) | 11 x 15 crop: one SSIM window row, odd W, batch offsets |
# odd border, misaligned vector head and tail, C = 1 | at least two partial blocks per image with a ragged last one | rows wider than a
# block's share: a block per row, 70 partials per image, more than the 64 lanes the finish step gives an image
CASES = [(1, 3, 9, 10, 4, "y"), (3, 3, 19, 23, 4, "y"), (3, 3, 19, 23, 4, "rgb"), (2, 1, 33, 37, 3, "y"), (2, 3, 70, 129, 0, "y"),
         (2, 3, 70, 129, 0, "rgb"), (2, 1, 70, 8201, 0, "y")]
IDS = ["-".join(str(v) for v in c) for c in CASES]
MODE_ID = {"y": 0, "rgb": 1}
E_SHAPE, E_NULL = -1, -2


def _L():
    from tpu_superresolution_amd import _lib
    return _lib.lib()


def _plane_shape(shape, border, mode):
    B, C, H, W = shape
    return B, (1 if mode == "y" else C), H - 2 * border, W - 2 * border


def _set_crop_prefix(img, border, values):
    """Writes values over the first elements of the cropped region of one image [C, H, W] (channel-major order)."""
    C, H, W = img.shape
    crop = img[:, border:H - border, border:W - border].copy()
    flat = crop.reshape(-1)
    n = min(values.size, flat.size)
    flat[:n] = values[:n]
    img[:, border:H - border, border:W - border] = flat.reshape(crop.shape)


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, border, mode):
    """Inputs (numpy fp32; target on the k / 255 grid, pred = target + noise with values outside [0, 1] and the 255 rounding ties
    in image 0) and their fp64 reference; computed once and shared: the tests copy before they change anything."""
    rng = np.random.RandomState(B * 1000 + H)
    t = (rng.randint(0, 256, size=(B, C, H, W)) / 255.0).astype(np.float32)
    p = (t + 0.04 * rng.standard_normal(t.shape)).astype(np.float32)
    _set_crop_prefix(p[0], border, R.tie_inputs()[0])
    return p, t, R.bench_ref(p, t, border, mode)


def _direct(p, t, border, mode, planes=True, psnr_sum=None, nan_ok=False):
    """One srk_bench_planes_f32 + srk_bench_psnr on guarded buffers -> (pp, pt [B, Cm, Hc, Wc] or None, sqsum [B], psnr [B]) on the CPU."""
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd._lib import check
    B, C, H, W = p.shape
    _, Cm, Hc, Wc = _plane_shape(p.shape, border, mode)
    L = _L()
    nws = int(L.srk_bench_workspace(B, Cm, Hc, Wc)) // 4
    assert nws >= B and nws % B == 0
    ws = Guarded("f32", 1, nws, nws)
    gpp, gpt = Guarded("f32", B * Cm * Hc, Wc, Wc), Guarded("f32", B * Cm * Hc, Wc, Wc)
    gsq, gps = Guarded("f32", 1, B, B), Guarded("f32", 1, B, B)
    check(L.srk_bench_planes_f32(ops._p(p), ops._p(t), gpp.ptr if planes else None, gpt.ptr if planes else None, ws.ptr, B, C, H, W,
                                 border, MODE_ID[mode], ops._stream()))
    check(L.srk_bench_psnr(ws.ptr, B, Cm, Hc, Wc, gsq.ptr, gps.ptr, ops._p(psnr_sum), ops._stream()))
    torch.cuda.synchronize()
    for g, what in ((ws, "workspace"), (gsq, "sqsum"), (gps, "psnr")):
        g.assert_guards(what)
    for g, what in ((gpp, "planes of pred"), (gpt, "planes of target")):
        if planes:
            g.assert_guards(what)
        else:
            g.assert_untouched(what)
    assert nan_ok or not bool(torch.isnan(ws.data()).any()), "a workspace entry was not written"
    shape = (B, Cm, Hc, Wc)
    return (gpp.data().view(shape) if planes else None, gpt.data().view(shape) if planes else None, gsq.data().view(B), gps.data().view(B))


def _f64(x):
    return x.numpy().astype(np.float64)


# ---- values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,border,mode", CASES, ids=IDS)
def test_planes_sums_psnr_and_ssim_against_the_restatement(B, C, H, W, border, mode):
    from tpu_superresolution_amd import ops
    p, t, ref = _case(B, C, H, W, border, mode)
    pp, pt, sq, ps = _direct(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda(), border, mode)
    count = ref["pp"][0].size
    for got, want, x in ((pp, ref["pp"], p), (pt, ref["pt"], t)):
        err = np.abs(_f64(got) - want)
        print(f"plane max err {err.max():.3e} (bound {R.plane_bound(mode, C):.3e})")
        assert np.all(err <= R.plane_bound(mode, C))
        if mode == "rgb" or C == 1:
            q = (torch.from_numpy(x).clamp(0, 1) * 255).round()[:, :, border:H - border, border:W - border]
            assert torch.equal(got, q)
    sq_err, sq_bound = np.abs(_f64(sq) - ref["sqsum"]), R.sqsum_bound(ref["sqsum"], count, mode, C)
    ps_err, ps_bound = np.abs(_f64(ps) - ref["psnr"]), R.psnr_bound(ref["sqsum"], count, mode, C)
    print(f"sqsum err {sq_err} (bound {sq_bound}); psnr err {ps_err} (bound {ps_bound})")
    assert np.all(sq_err <= sq_bound) and np.all(ps_err <= ps_bound)
    if ref["ssim"] is not None:
        ss = ops.ssim(pp.cuda(), pt.cuda(), 255.0)[0].cpu()
        ss_err = np.abs(_f64(ss) - ref["ssim"])
        print(f"ssim err {ss_err} (bound {R.SSIM_BOUND})")
        assert np.all(ss_err <= R.SSIM_BOUND)
    else:
        assert min(H, W) - 2 * border < 11


def test_rounding_ties_go_to_the_even_level():
    x, k = R.tie_inputs()
    assert x.size == 255
    img = torch.from_numpy(x).view(1, 1, 15, 17).cuda()
    pp, pt, sq, ps = _direct(img, img.clone(), 0, "rgb")
    even = torch.from_numpy(np.where(k % 2 == 0, k, k + 1).astype(np.float32)).view(1, 1, 15, 17)
    assert torch.equal(pp, even) and torch.equal(pt, even) and float(sq) == 0.0 and math.isinf(float(ps)) and float(ps) > 0


@pytest.mark.parametrize("B,C,H,W,border,mode", [c[:5] + ("rgb",) for c in CASES if c[5] == "y" or c[1] == 1], ids=lambda v: str(v))
def test_exact_integer_sums(B, C, H, W, border, mode):
    """pred = target + d / 255 on the grid with integer |d| <= 3: every partial sum is an integer below 2^24 in any order, so the sum
    of squares is exact: one dropped, doubled or misplaced element shows."""
    rng = np.random.RandomState(7)
    k = rng.randint(3, 253, size=(B, C, H, W))
    d = rng.randint(-3, 4, size=k.shape)
    t, p = (k / 255.0).astype(np.float32), ((k + d) / 255.0).astype(np.float32)
    dc = d[:, :, border:H - border, border:W - border]
    want = (dc.astype(np.int64) ** 2).reshape(B, -1).sum(1)
    assert want.max() < 2 ** 24
    pp, pt, sq, ps = _direct(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda(), border, mode)
    assert torch.equal(pp - pt, torch.from_numpy(dc.astype(np.float32)))
    assert torch.equal(sq, torch.from_numpy(want.astype(np.float32))), (sq, want)
    count = C * (H - 2 * border) * (W - 2 * border)
    assert np.all(np.abs(_f64(ps) - R.psnr_from_sqsum(want.astype(np.float64), count)) <= R.psnr_bound(want.astype(np.float64), count, mode, C))


def test_identical_images_give_inf_and_psnr_sum_accumulates():
    p, t, ref = _case(*CASES[1])
    dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    _, _, sq, ps = _direct(dp, dp.clone(), 4, "y")
    assert torch.equal(sq, torch.zeros(3)) and bool(torch.isposinf(ps).all())
    acc = torch.zeros(1, dtype=torch.float32, device="cuda")
    ps1 = _direct(dp, dt, 4, "y", psnr_sum=acc)[3]
    first = float(acc)
    ps2 = _direct(dt * 0.5, dp, 4, "y", psnr_sum=acc)[3]
    want = np.float32(0)
    for batch in (ps1, ps2):                                   # each call adds the sum of its images, formed in image order
        s = np.float32(0)
        for v in batch.numpy():
            s = np.float32(s + v)
        want = np.float32(want + s)
        if batch is ps1:
            assert first == float(want)
    assert float(acc) == float(want) and math.isfinite(float(want)) and not torch.equal(ps1, ps2)


# ---- crop, NaN, null outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,border,mode", [c for c in CASES if c[4] > 0], ids=[i for c, i in zip(CASES, IDS) if c[4] > 0])
def test_the_cropped_frame_is_never_read_and_a_nan_inside_reaches_its_image_only(B, C, H, W, border, mode):
    p, t, _ = _case(B, C, H, W, border, mode)
    clean = _direct(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda(), border, mode)
    framed = []
    for a in (p, t):
        f = np.full_like(a, np.nan)
        f[:, :, border:H - border, border:W - border] = a[:, :, border:H - border, border:W - border]
        framed.append(torch.from_numpy(f).cuda())
    got = _direct(framed[0], framed[1], border, mode)
    for g, c in zip(got, clean):
        assert bool(torch.isfinite(g).all()) and torch.equal(g, c)
    if B < 2:
        return
    framed[0][1, C - 1, H - border - 1, W - border - 1] = float("nan")          # the last element inside the crop of image 1
    pp, pt, sq, ps = _direct(framed[0], framed[1], border, mode, nan_ok=True)
    bad = torch.isnan(ps)
    assert bad.tolist() == [b == 1 for b in range(B)] and torch.isnan(sq).tolist() == bad.tolist()
    assert torch.equal(ps[~bad], clean[3][~bad]) and torch.equal(pt, clean[1]) and int(torch.isnan(pp).sum()) == 1


@pytest.mark.parametrize("B,C,H,W,border,mode", [CASES[3], CASES[4]], ids=[IDS[3], IDS[4]])
def test_null_plane_pointers_write_no_planes_and_leave_the_psnr_as_it_is(B, C, H, W, border, mode):
    p, t, _ = _case(B, C, H, W, border, mode)
    dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    with_planes, without = _direct(dp, dt, border, mode), _direct(dp, dt, border, mode, planes=False)
    assert without[0] is None and torch.equal(with_planes[2], without[2]) and torch.equal(with_planes[3], without[3])


def test_the_large_case_spans_several_blocks_with_a_ragged_last_one():
    L = _L()
    for Cm in (1, 3):
        blocks = lambda rows: int(L.srk_bench_workspace(2, 1, rows, 129)) // (4 * 2)          # noqa: E731
        rows_per_block = max(r for r in range(1, 3 * 70 + 1) if blocks(r) == 1)
        n = int(L.srk_bench_workspace(2, Cm, 70, 129)) // (4 * 2)
        assert n >= 2 and n == -(-Cm * 70 // rows_per_block) and (Cm * 70) % rows_per_block != 0
    assert int(L.srk_bench_workspace(2, 1, 70, 8201)) // (4 * 2) == 70          # the wide case: a block per row


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_points():
    L = _L()
    a, b, o1, o2, w = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000          # dummies: every call is refused before any launch
    ok = dict(B=2, C=3, H=19, W=23, border=4, mode=0)

    def planes(pred=a, target=b, pp=o1, pt=o2, ws=w, **kw):
        v = {**ok, **kw}
        return L.srk_bench_planes_f32(pred, target, pp, pt, ws, v["B"], v["C"], v["H"], v["W"], v["border"], v["mode"], None)

    assert planes(pred=None) == E_NULL and planes(target=None) == E_NULL and planes(ws=None) == E_NULL
    assert b"bench_planes" in L.srk_last_error()
    assert planes(B=1025) == E_SHAPE and planes(B=0) == E_SHAPE
    assert planes(C=2) == E_SHAPE and planes(C=4) == E_SHAPE and planes(C=0, mode=1) == E_SHAPE and planes(mode=2) == E_SHAPE
    assert planes(border=-1) == E_SHAPE
    assert planes(border=10) == E_SHAPE and planes(H=8) == E_SHAPE            # 2 border >= H
    assert planes(border=12, H=40) == E_SHAPE and planes(W=8) == E_SHAPE      # 2 border >= W
    assert planes(pp=a) == E_SHAPE and planes(pt=b + 4) == E_SHAPE            # planes overlapping an input
    assert L.srk_bench_psnr(None, 2, 1, 11, 15, o1, o2, None, None) == E_NULL
    assert L.srk_bench_psnr(w, 2, 1, 11, 15, None, None, None, None) == E_NULL
    assert L.srk_bench_psnr(w, 1025, 1, 11, 15, o1, o2, None, None) == E_SHAPE and L.srk_bench_psnr(w, 2, 1, 0, 15, o1, o2, None, None) == E_SHAPE
    assert L.srk_bench_workspace(1025, 1, 11, 15) == 0 and L.srk_bench_workspace(2, 0, 11, 15) == 0 and L.srk_bench_workspace(2, 1, 11, -1) == 0
    assert L.srk_bench_workspace(2, 1, 11, 15) == 4 * 2


def test_python_wrappers_raise_before_any_launch(monkeypatch):
    from tpu_superresolution_amd import metrics, ops
    x = torch.rand(2, 3, 19, 23, device="cuda")

    def no_launch(*a, **k):
        raise AssertionError("the C entry point was reached")

    L = _L()
    for name in ("srk_bench_planes_f32", "srk_bench_psnr", "srk_ssim"):
        monkeypatch.setattr(L, name, no_launch)
    for bad in ((x, x, 10), (x, x, -1), (x, x, 4, "ycbcr"), (x, x, 2.0), (x[:, :2], x[:, :2], 4, "y"), (x, x[:, :, 1:], 4), (x, x.double(), 4),
                (torch.rand(1025, 1, 3, 3, device="cuda"),) * 2 + (0,), (x[0], x[0], 4)):
        with pytest.raises(ValueError):
            ops.bench_planes(*bad)
    ws = torch.zeros(2, 1, device="cuda")
    for bad in ((ws, (2, 1, 0, 15)), (ws, (1025, 1, 11, 15)), (ws, (2, 1, 70, 129)), (ws.double(), (2, 1, 11, 15)),
                (ws, (2, 1, 11, 15), torch.zeros(2, device="cuda"))):
        with pytest.raises(ValueError):
            ops.bench_psnr(*bad)
    with pytest.raises(ValueError, match="9 x 13"):
        metrics.bench_metrics(x, x, 5, "y")


# ---- the public function and the validation loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,border,mode", CASES, ids=IDS)
def test_bench_metrics_on_the_device_against_its_cpu_form(B, C, H, W, border, mode):
    from tpu_superresolution_amd import metrics
    p, t, ref = _case(B, C, H, W, border, mode)
    with_ssim = ref["ssim"] is not None
    tp, tt = torch.from_numpy(p), torch.from_numpy(t)
    cpu_ps, cpu_ss = metrics.bench_metrics(tp, tt, border, mode, with_ssim=with_ssim)
    ps, ss = metrics.bench_metrics(tp.cuda(), tt.cuda(), border, mode, with_ssim=with_ssim)
    assert ps.is_cuda and ps.dtype == torch.float32 and ps.shape == (B,)
    bound = R.psnr_bound(ref["sqsum"], ref["pp"][0].size, mode, C)
    assert np.all(np.abs(_f64(ps.cpu()) - ref["psnr"]) <= bound)
    assert np.all(np.abs(_f64(ps.cpu()) - _f64(cpu_ps)) <= 2 * bound)          # each within the bound of the exact value
    if with_ssim:
        assert ss.is_cuda and ss.shape == (B,) and np.all(np.abs(_f64(ss.cpu()) - _f64(cpu_ss)) <= 2 * R.SSIM_BOUND)
    else:
        assert ss is None and cpu_ss is None


class _Nearest(torch.nn.Module):
    """An exact stand-in model: s x nearest upsample."""

    def __init__(self, s):
        super().__init__()
        self.s = s

    def forward(self, x):
        return x.repeat_interleave(self.s, dim=2).repeat_interleave(self.s, dim=3)


def test_validate_accumulates_the_per_image_mean_on_the_device():
    from tpu_superresolution_amd import finetune_swinir as F
    from tpu_superresolution_amd import metrics
    g = torch.Generator().manual_seed(3)
    model = _Nearest(2)
    loader = []
    for b, noise in ((2, 0.05), (1, 0.1)):                      # a short, noisier second batch
        lr = torch.rand(b, 3, 12, 14, generator=g)
        loader.append((lr, (model(lr) + noise * torch.randn(b, 3, 24, 28, generator=g)).clamp(0, 1)))
    plain = F.validate(model, loader, "cuda")
    assert len(plain) == 3 and F.validate_bench(model, loader, "cuda", None, 0)[:2] == plain[:2]
    assert len(F.validate_bench(model, loader, "cuda", None, 0)) == 3
    for mode in ("y", "rgb"):
        per = [metrics.bench_metrics(model(lr.cuda()), hr.cuda(), 2, mode) for lr, hr in loader]
        want_p = float(torch.cat([v[0] for v in per]).double().mean())
        want_s = float(torch.cat([v[1] for v in per]).double().mean())
        out = F.validate_bench(model, loader, "cuda", mode, 2)
        assert len(out) == 5 and out[:2] == plain[:2]
        assert out[2] == pytest.approx(want_p, rel=1e-6) and out[3] == pytest.approx(want_s, rel=1e-6)
        over_batches = (float(per[0][0].mean()) + float(per[1][0].mean())) / 2
        assert abs(over_batches - want_p) > 1e-4 * abs(want_p)
    with_ssim = F.validate_bench(model, loader, "cuda", "y", 2, with_ssim=True)
    assert len(with_ssim) == 6 and with_ssim[:2] == plain[:2] and with_ssim[2] == F.validate(model, loader, "cuda", with_ssim=True)[2]
    with pytest.raises(ValueError, match="11 x 11"):
        F.validate_bench(model, loader, "cuda", "y", 7)


def test_finetune_script_reports_and_saves_the_scores(tmp_path, capsys, monkeypatch):
    """finetune_swinir.main --val_bench_metric y with --val_tile: the epoch line and both checkpoints gain the two figures."""
    import os
    import re

    from PIL import Image

    from tpu_superresolution_amd import finetune_swinir as F
    rng = np.random.RandomState(0)
    for split, n in (("train", 4), ("valid", 3)):
        hr_dir = tmp_path / "shuffled2D" / f"shuffled2D_{split}_HR"
        lr_dir = tmp_path / "shuffled2D" / f"shuffled2D_{split}_LR_default_X4"
        os.makedirs(hr_dir), os.makedirs(lr_dir)
        for i in range(n):
            hr = (rng.rand(288, 288) * 255).astype(np.uint8)
            Image.fromarray(hr, "L").save(str(hr_dir / f"{i:04d}.png"))
            Image.fromarray(hr, "L").resize((72, 72), Image.BICUBIC).save(str(lr_dir / f"{i:04d}x4.png"))
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--lr", "1e-4",
            "--val_bench_metric", "y", "--val_tile", "48", "--val_tile_overlap", "8"])
    text = capsys.readouterr().out
    m = re.search(r"PSNR=(-?[\d.]+)dB, bench PSNR-Y=(-?[\d.]+)dB SSIM-Y=(-?[\d.]+) \(8-bit, border 4\) \(", text)
    assert m, text
    for name in ("best_swinir_finetune_X4.pt", "bestpsnr_swinir_finetune_X4.pt"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=False)
        assert f"{ck['val_bench_psnr']:.2f}" == m.group(2) and f"{ck['val_bench_ssim']:.4f}" == m.group(3)
        assert math.isfinite(ck["val_bench_psnr"]) and -1.0 <= ck["val_bench_ssim"] <= 1.0
        assert ck["args"]["val_bench_metric"] == "y" and "val_crop_border" not in ck["args"]
        # grey images replicated to RGB: the luma spans 219 of 255 levels, which alone is worth 1.32 dB over the script's own PSNR
        assert ck["val_bench_psnr"] > ck.get("val_psnr", ck.get("best_val_psnr")) + 1.0
