"""srk_psnrb and srk_msssim (csrc/fullref.hip) through the C ABI against the fp64 restatement of tests/fullref_ref.py, then metrics.psnrb /
metrics.ms_ssim and the score command line end to end.  Inputs and outputs of the direct calls sit between the NaN guard rows of
tests/guarded.py: a read outside an input reaches the output as a NaN, a write outside an output changes a guard row.

MS-SSIM, measured on an MI355X over every case below: the worst |device - restatement| of a level mean is 0.395 of its 2e-5 bound (161 x 161,
the one map position of the coarsest level), of the combined score 0.064 of the propagated bound (printed by the tests)."""
import functools
import math

import numpy as np
import pytest
import torch
from PIL import Image

import fullref_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MEAN_BOUND = 2e-5          # the bound tests/test_gpu_metrics.py holds the same map arithmetic to


def _L():
    from tpu_superresolution_amd import _lib
    return _lib.lib()


def _stream():
    from tpu_superresolution_amd import ops
    return ops._stream()


def _check(rc):
    from tpu_superresolution_amd._lib import check
    check(rc)


def _guarded_in(a):
    """An input in a guarded buffer: NaN rows before and after it."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    a2 = a.reshape(-1, a.shape[-1])
    return Guarded("f32", a2.shape[0], a2.shape[1], a2.shape[1], fill=torch.from_numpy(a2))


# ---- PSNR-B ----------------------------------------------------------------------------------------------------------------------------
PB_SHAPES = [(16, 16), (20, 27), (24, 40), (65, 33)]          # both 1 (mod 8) axes; 65 rows split into runs of 32, 32 and 1
PB_BATCH = [(1, 1), (1, 3), (3, 1), (3, 3)]                   # B, Cm
PB_KINDS = ["int15", "u8", "luma"]


@functools.lru_cache(maxsize=None)
def _pb_input(H, W, B, Cm, kind):
    rng = np.random.RandomState(H * 131 + W * 7 + B * 3 + Cm + len(kind))
    if kind == "int15":                                          # every sum stays below 2^24: exact in fp32 in any order
        p, t = rng.randint(0, 16, (B, Cm, H, W)), rng.randint(0, 16, (B, Cm, H, W))
    elif kind == "u8":
        t = rng.randint(0, 256, (B, Cm, H, W))
        p = np.clip(t + np.round(9.0 * rng.standard_normal(t.shape)), 0, 255)
    else:                                                        # non-integer values on the luma scale
        t = 16.0 + 219.0 * rng.rand(B, Cm, H, W)
        p = np.clip(t + 5.0 * rng.standard_normal(t.shape), 16.0, 235.0)
    return np.asarray(p, np.float32), np.asarray(t, np.float32)


@functools.lru_cache(maxsize=None)
def _pb_ref(H, W, B, Cm, kind):
    p, t = _pb_input(H, W, B, Cm, kind)
    sums = np.array([[R.psnrb_sums(p[b, c], t[b, c]) for c in range(Cm)] for b in range(B)])
    eb, es = R.psnrb_bound(p, t)
    return sums, R.psnrb(p, t), eb, es


def _run_psnrb(p, t, want_sums=True, want_score=True):
    B, Cm, H, W = p.shape
    gp, gt = _guarded_in(p), _guarded_in(t)
    nws = _L().srk_psnrb_workspace(B, Cm, H, W) // 4
    ws, sums, out = Guarded("f32", 1, nws, nws), Guarded("f32", B * Cm, 5, 5), Guarded("f32", 1, B, B)
    _check(_L().srk_psnrb(gp.ptr, gt.ptr, ws.ptr, B, Cm, H, W, sums.ptr if want_sums else None, out.ptr if want_score else None, _stream()))
    torch.cuda.synchronize()
    for g, what in ((ws, "workspace"), (sums, "sums"), (out, "psnrb")):
        g.assert_guards(what)
    gp.assert_untouched("planes_pred")
    gt.assert_untouched("planes_target")
    if not want_sums:
        sums.assert_untouched("sums")
    if not want_score:
        out.assert_untouched("psnrb")
    return sums.data().view(B, Cm, 5).double().numpy(), out.data().view(B).double().numpy()


@pytest.mark.parametrize("B,Cm", PB_BATCH, ids=[f"B{b}C{c}" for b, c in PB_BATCH])
@pytest.mark.parametrize("H,W", PB_SHAPES, ids=[f"{h}x{w}" for h, w in PB_SHAPES])
@pytest.mark.parametrize("kind", PB_KINDS)
def test_psnrb_sums_and_score_match_the_restatement(kind, H, W, B, Cm):
    p, t = _pb_input(H, W, B, Cm, kind)
    want_sums, want, eb, es = _pb_ref(H, W, B, Cm, kind)
    sums, got = _run_psnrb(p, t)
    if kind == "int15":
        assert np.array_equal(sums, want_sums)                   # torch.equal with the restatement: integers below 2^24
    else:
        err = np.abs(sums - want_sums)
        assert (err <= eb).all(), (float((err / np.maximum(eb, 1e-30)).max()), "of the 2 n u S bound")
    assert np.isfinite(got).all() and (np.abs(got - want) <= es).all(), (got, want, es)
    again_sums, again = _run_psnrb(p, t)
    assert np.array_equal(again_sums, sums) and np.array_equal(again, got)      # a fixed order: equal bits


def test_psnrb_either_output_may_be_absent():
    p, t = _pb_input(24, 40, 3, 3, "u8")
    sums, got = _run_psnrb(p, t)
    s2, _ = _run_psnrb(p, t, want_score=False)
    _, g2 = _run_psnrb(p, t, want_sums=False)
    assert np.array_equal(s2, sums) and np.array_equal(g2, got)


def test_psnrb_special_values():
    """D_b < D_n gives bef exactly 0 (equal planes then give +inf, which any bef > 0 would make finite); equal planes whose neighbours all
    differ alike (D_b = D_n) give +inf; equal blocky planes stay finite; a NaN inside either plane reaches the result."""
    rng = np.random.RandomState(4)
    H, W = 40, 33
    p = rng.randint(0, 256, (2, 1, H, W)).astype(np.float32)
    for x in range(7, W - 1, 8):
        p[..., x + 1] = p[..., x]                                # no step at any boundary: D_b = 0 < D_n
    for y in range(7, H - 1, 8):
        p[..., y + 1, :] = p[..., y, :]
    s = R.psnrb_sums(p[0, 0], p[0, 0])
    assert s[1] == 0 and s[3] == 0 and s[2] > 0 and s[4] > 0
    sums, got = _run_psnrb(p, p.copy())
    assert np.isposinf(got).all() and (sums[..., 0] == 0).all() and (sums[..., 1] == 0).all() and (sums[..., 2] > 0).all()
    yy, xx = np.meshgrid(np.arange(H), np.arange(W - 1), indexing="ij")      # 40 x 32: at 1 (mod 8) the published counts alone make D_b > D_n
    ramp = np.broadcast_to((20.0 + xx + yy).astype(np.float32), (1, 3, H, W - 1)).copy()
    assert np.isposinf(R.psnrb(ramp, ramp)).all() and np.isposinf(_run_psnrb(ramp, ramp.copy())[1]).all()
    blocks = (100.0 + 6.0 * ((yy // 8 + xx // 8) % 2)).astype(np.float32)[None, None]
    _, fin = _run_psnrb(blocks, blocks.copy())
    assert np.isfinite(fin).all() and abs(fin[0] - R.psnrb(blocks, blocks)[0]) < 1e-4
    for who in (0, 1):
        a, b = p.copy(), p.copy()
        (a if who == 0 else b)[1, 0, 17, 9] = np.nan
        _, got = _run_psnrb(a, b)
        assert np.isposinf(got[0]) and np.isnan(got[1]), (who, got)


# ---- MS-SSIM ---------------------------------------------------------------------------------------------------------------------------
# H, W, C, levels: the smallest legal shape, odd at every level | mixed parity | even then odd | one level on the bare window | three levels
MS_CASES = [(161, 161, 1, 5), (161, 161, 3, 5), (176, 163, 1, 5), (176, 163, 3, 5), (162, 200, 1, 5), (162, 200, 3, 5), (11, 11, 3, 1), (41, 44, 3, 3)]
MS_B = 2
SIGMAS = (4, 12, 30)


@functools.lru_cache(maxsize=None)
def _ms_input(H, W, C, levels):
    x = np.stack([np.stack([R.pink_image(H * 7 + W + 10 * b + c, H, W) for c in range(C)]) for b in range(MS_B)])
    y = np.stack([np.stack([R.noised(x[b, c], SIGMAS[(b * C + c + H) % 3], b + c) for c in range(C)]) for b in range(MS_B)])
    return x, y


@functools.lru_cache(maxsize=None)
def _ms_ref(H, W, C, levels):
    x, y = _ms_input(H, W, C, levels)
    means = np.zeros((levels, MS_B, C, 2))
    pyr = [[None] * (MS_B * C) for _ in range(levels - 1)]
    for b in range(MS_B):
        for c in range(C):
            m, p = R.msssim_levels(x[b, c], y[b, c], levels)
            means[:, b, c] = m
            for s in range(levels - 1):
                pyr[s][b * C + c] = p[s]
    return means, pyr


def _ms_score_and_bound(means, weights):
    """means [levels, 2] of one channel (the restatement's) -> (score, the MEAN_BOUND of every level propagated through the power product:
    ms * sum_s w_s * MEAN_BOUND / v_s)."""
    L = len(means)
    v = [means[s][1] if s < L - 1 else means[s][0] for s in range(L)]
    ms = R.msssim_from_means(means, weights)
    return ms, ms * sum(weights[s] * MEAN_BOUND / v[s] for s in range(L))


def _run_msssim(x, y, levels):
    B, C, H, W = x.shape
    gx, gy = _guarded_in(x), _guarded_in(y)
    nws = _L().srk_msssim_workspace(B, C, H, W, levels) // 4
    rows = -(-nws // 64)
    ws = Guarded("f32", rows, 64, 64, fill=torch.full((rows, 64), -7.0))
    means = Guarded("f32", levels * B * C, 2, 2)
    _check(_L().srk_msssim(gx.ptr, gy.ptr, ws.ptr, B, C, H, W, levels, 255.0, means.ptr, _stream()))
    torch.cuda.synchronize()
    ws.assert_guards("workspace")
    means.assert_guards("means")
    gx.assert_untouched("x")
    gy.assert_untouched("y")
    flat = ws.data().reshape(-1)
    assert bool((flat[nws:] == -7.0).all()), "floats behind the stated workspace size were written"
    return means.data().view(levels, B, C, 2), flat[:nws].clone()


@pytest.mark.parametrize("H,W,C,levels", MS_CASES, ids=[f"{h}x{w}-C{c}-L{l}" for h, w, c, l in MS_CASES])
def test_msssim_pyramid_means_and_score_match_the_restatement(H, W, C, levels):
    x, y = _ms_input(H, W, C, levels)
    want, pyr = _ms_ref(H, W, C, levels)
    assert want.min() >= 0.4, "a condition on the inputs: no level mean near the clamp at 0"
    means, ws = _run_msssim(x, y, levels)
    # the pooled pyramids: integer planes stay exactly representable through four poolings, so this is bit equality
    off, planes = 0, MS_B * C
    for s in range(levels - 1):
        Hs, Ws = pyr[s][0][0].shape
        for k in (0, 1):                                         # the x planes, then the y planes
            got = ws[off:off + planes * Hs * Ws].view(planes, Hs, Ws)
            ref = torch.from_numpy(np.stack([pyr[s][q][k] for q in range(planes)]))
            assert torch.equal(got.double(), ref), (s, "xy"[k])
            off += planes * Hs * Ws
    err = np.abs(means.double().numpy() - want)
    worst = float(err.max()) / MEAN_BOUND
    weights = R.WEIGHTS[:levels] if levels == 5 else tuple(1.0 / levels for _ in range(levels))
    worst_ms = 0.0
    for b in range(MS_B):
        for c in range(C):
            ms, bound = _ms_score_and_bound(want[:, b, c], weights)
            got = R.msssim_from_means(means[:, b, c].double().numpy(), weights)
            worst_ms = max(worst_ms, abs(got - ms) / bound)
    print(f"[msssim {H}x{W} C{C} L{levels}] worst level-mean error / 2e-5 = {worst:.3f}; worst score error / propagated bound = {worst_ms:.3f}")
    assert worst <= 1.0, err.max()
    assert worst_ms <= 1.0
    means2, ws2 = _run_msssim(x, y, levels)
    assert torch.equal(means2, means) and torch.equal(ws2, ws)      # two runs give equal bits


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _images(B, C, H, W, sigma, seed):
    x = np.stack([np.stack([R.pink_image(seed + 10 * b + c, H, W) for c in range(C)]) for b in range(B)])
    y = np.stack([np.stack([R.noised(x[b, c], sigma, b + c) for c in range(C)]) for b in range(B)])
    return torch.from_numpy(x / 255.0).float(), torch.from_numpy(y / 255.0).float()


def _db_bound(n):
    """PSNR: an fp32 sum of n non-negative terms is within 2 n u of the exact one, relatively; 10 log10 turns that into decibels."""
    return 10.0 / math.log(10.0) * 2.0 * n * U + 1e-5


def _psnrb_bound(sr, gt, border, mode):
    """PSNR-B: fullref_ref.psnrb_bound on the planes of the CPU form (their bits are the device's)."""
    from tpu_superresolution_amd import metrics as M
    pp, pt = M.bench_planes_pair(sr, gt, border, mode)
    return R.psnrb_bound(pp.numpy(), pt.numpy())[1]


@pytest.mark.parametrize("mode,C,border", [("y", 3, 2), ("rgb", 3, 0), ("y", 1, 3)])
def test_metrics_psnrb_on_the_device_equals_the_cpu_form(mode, C, border):
    from tpu_superresolution_amd import metrics as M
    gt, sr = _images(3, C, 43, 57, 10, 3)
    want = M.psnrb(sr, gt, border, mode)
    got = M.psnrb(sr.cuda(), gt.cuda(), border, mode)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (3,)
    assert ((got.cpu() - want).abs().double().numpy() <= _psnrb_bound(sr, gt, border, mode) + 1e-5).all()      # 1e-5: want is rounded to fp32
    with pytest.raises(ValueError, match="at least 16 x 16"):
        M.psnrb(sr.cuda(), gt.cuda(), 14, mode)


@pytest.mark.parametrize("C,H,W", [(1, 161, 161), (3, 170, 165)])
def test_metrics_ms_ssim_on_the_device_equals_the_cpu_form(C, H, W, monkeypatch):
    from tpu_superresolution_amd import metrics as M
    gt, sr = _images(2, C, H, W, 12, 5)
    X, Y = (sr * 255).round(), (gt * 255).round()
    want = M.ms_ssim(X.double(), Y.double(), size_average=False)
    bound = max(_ms_score_and_bound(R.msssim_levels(X[b, c].numpy(), Y[b, c].numpy())[0], R.WEIGHTS)[1] for b in range(2) for c in range(C))
    got = M.ms_ssim(X.cuda(), Y.cuda(), size_average=False)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (2,)
    assert float((got.cpu().double() - want).abs().max()) <= bound
    assert abs(float(M.ms_ssim(X.cuda(), Y.cuda())) - float(want.mean())) <= bound
    w3 = (0.2, 0.3, 0.5)
    got3 = M.ms_ssim(X.cuda()[:, :, :60, :50].contiguous(), Y.cuda()[:, :, :60, :50].contiguous(), size_average=False, weights=w3)
    assert float((got3.cpu().double() - M.ms_ssim(X.double()[:, :, :60, :50], Y.double()[:, :, :60, :50], size_average=False, weights=w3)).abs().max()) <= 1e-4
    assert float(M.ms_ssim(X.cuda(), X.cuda())) == pytest.approx(1.0, abs=1e-5)
    taken = []                                                   # no gradient on the device path: an X that requires grad goes to the torch form
    monkeypatch.setattr(M, "ms_ssim_torch", lambda X, Y, **kw: taken.append(kw) or X.sum())
    assert M.ms_ssim(X.cuda().requires_grad_(True), Y.cuda()).requires_grad and len(taken) == 1
    M.ms_ssim(X.cuda(), Y.cuda(), win_size=7)                    # and so does another window
    assert len(taken) == 2 and taken[1]["win_size"] == 7
    monkeypatch.undo()
    with pytest.raises(ValueError, match="smaller side above 160"):
        M.ms_ssim(X.cuda()[:, :, :160].contiguous(), Y.cuda()[:, :, :160].contiguous())


def test_jpeg_blocks_lower_psnrb_below_psnr_and_a_blur_does_not():
    from tpu_superresolution_amd import metrics as M
    from tpu_superresolution_amd import ops
    yy, xx = np.meshgrid(np.arange(96), np.arange(128), indexing="ij")
    # whether an unblocked image has D_b <= D_n is a matter of where its gradients fall on the grid: these periods leave the blur D_b < D_n
    img = 0.5 + 0.25 * np.sin(xx / 19.0) * np.cos(yy / 9.0) + 0.15 * np.sin((xx + 2 * yy) / 31.0)
    x = torch.from_numpy(img).float()[None, None].cuda()
    jpg = ops.jpeg_roundtrip(x, 10)
    psnr = M.bench_metrics(jpg, x, 0, "y", with_ssim=False)[0]
    pb = M.psnrb(jpg, x, 0, "y")
    assert float(pb) < float(psnr) - 0.1, (float(pb), float(psnr))
    blur = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x.cpu(), (2, 2, 2, 2), mode="replicate"), 5, stride=1)
    pp, pt = M.bench_planes_pair(blur, x.cpu(), 0, "y")
    blur = blur.cuda()
    assert R.psnrb_parts(R.psnrb_sums(pp[0, 0].numpy(), pt[0, 0].numpy()), 96, 128)[1] == 0.0, "a condition on the input: D_b <= D_n"
    assert float(M.psnrb(blur, x, 0, "y")) == float(M.bench_metrics(blur, x, 0, "y", with_ssim=False)[0])
    assert float(M.psnrb(x, jpg, 0, "y")) > float(pb) + 0.1      # the blocking effect is the restored image's, not the target's


def test_score_command_line_on_the_device_equals_the_cpu_run(tmp_path):
    from tpu_superresolution_amd import score as S
    gt, sr = tmp_path / "gt", tmp_path / "sr"
    gt.mkdir()
    sr.mkdir()
    for k, (n, H, W) in enumerate([("a", 170, 165), ("b", 170, 165), ("c", 64, 72), ("d", 64, 72)]):
        a = np.stack([R.pink_image(40 + 3 * k + j, H, W) for j in range(3)], axis=-1)
        Image.fromarray(a.astype(np.uint8), mode="RGB").save(gt / f"{n}.png")
        Image.fromarray(R.noised(a, 6 + 5 * k, k).astype(np.uint8), mode="RGB").save(sr / f"{n}_sr.png")
    argv = ["--sr", str(sr), "--gt", str(gt), "--batch_size", "2", "--crop_border", "2", "--metrics", "psnr", "ssim", "psnrb", "ms_ssim"]
    lines = []
    dev = S.main(argv + ["--device", "cuda"], log=lines.append)
    cpu = S.main(argv + ["--device", "cpu"], log=lambda s: None)
    assert lines[0] == "[device] cuda" and dev["n"] == 4 and list(dev["scores"]) == list(cpu["scores"])
    def both(n):
        return [torch.from_numpy(np.array(Image.open(q))).permute(2, 0, 1)[None].float() / 255.0 for q in (sr / f"{n}_sr.png", gt / f"{n}.png")]

    tol = {"psnr": _db_bound(166 * 161), "psnrb": max(float(_psnrb_bound(*both(n), 2, "y")[0]) for n in "abcd") + 1e-5, "ssim": MEAN_BOUND,
           "ms_ssim": 1e-4}
    for n, s in dev["scores"].items():
        for m, v in s.items():
            w = cpu["scores"][n][m]
            assert (v is None) == (w is None) and (v is None or abs(v - w) <= tol[m]), (n, m, v, w)
    assert dev["scores"]["c_sr.png"]["ms_ssim"] is None and dev["scores"]["a_sr.png"]["ms_ssim"] is not None
    assert any(ln.startswith("[score] c_sr.png") and ln.endswith("ms_ssim=-") for ln in lines)
    for m in tol:
        assert abs(dev["mean"][m] - cpu["mean"][m]) <= tol[m]
