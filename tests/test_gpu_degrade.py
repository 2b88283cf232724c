"""srk_crop_degrade_blind_u8 / srk_degrade_blind_f32 (csrc/degrade.hip) and what is built on them: ops.degrade_blind,
sr_datasets.DeviceHRPool(degrade=DegradeSpec), SynthLRBatches(degrade=...) and the --degrade blind command lines.  The reference is
tests/degrade_ref.py (fp64 numpy, pinned in tests/test_degrade_ref.py).

Tolerances (derived, not tuned).  Noise off: degrade_ref.bound = 2 (Ky + Kx + 4) u Ly Lx max|x| on the COMPOSED tables (the rule of
tests/test_gpu_resize.py).  Noise on: that plus C_NOISE u (r + |z|) std per element, r = sqrt(-2 ln u1): the error of the device's
logf / sqrtf / cospif chain scaled by the noise amplitude.  No HIP document with ulp bounds of these functions ships with the toolchain,
so C_NOISE = 4 x the largest |z_dev - z| / (u (r + |z|)) measured by test_device_normal below (recorded in degrade_ref.py and DESIGN
7k).  The noisy cases keep sigma_n > 0, which bounds how far the filter's own error moves the amplitude: |d std / d v| <= gain / (2
sigma_n) <= 1 / 6.  Everything that can be exact is compared with torch.equal: sigma (0, 0) without noise against srk_crop_degrade_u8,
the HR patch against srk_paired_crop_u8, a patch against the window of the whole-image form, a second launch with the same ids."""
import functools
import random

import numpy as np
import pytest
import torch

import degrade_ref as D
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL = -1, -2
P = D.PATCH
CASES = [(s, k) for s in D.SCALES for k in range(len(D.SOURCES))]
CASE_IDS = [f"x{s}-{D.SOURCES[k]}" for s, k in CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _blind(pool, desc, lr, hr, B, patch, s, q=0):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_crop_degrade_blind_u8(_ptr(pool), _ptr(desc), _ptr(lr), _ptr(hr), B, patch, s, q, _stream())


def _whole(x, out, par, B, C, H, W, s, q=0):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_degrade_blind_f32(_ptr(x), _ptr(out), _ptr(par), B, C, H, W, s, q, _stream())


@functools.lru_cache(maxsize=None)
def _pool_case(s, k):
    """The one-image pool of case (s, k) on the device and its samples."""
    from tpu_superresolution_amd.sr_datasets import DeviceHRPool
    pool = DeviceHRPool([D.case_image(s, k)], P, s)
    return pool, D.case_samples(s, k)


def _desc(s, k, noisy, ids=None):
    pool, samples = _pool_case(s, k)
    rows = [list(pool.meta[0][1]) + [top, left] + D.pack(sigma, noise if noisy else (0.0, 0.0), nid if ids is None else ids[b], gray)
            for b, (top, left, sigma, noise, nid, gray) in enumerate(samples)]
    return torch.tensor(rows, dtype=torch.int64).cuda()


def _run(s, k, noisy, q, ids=None):
    pool, samples = _pool_case(s, k)
    B = len(samples)
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 3 * P * P * s * s, B * 3 * P * P * s * s)
    assert _blind(pool.pool, _desc(s, k, noisy, ids), lr.ptr, hr.ptr, B, P, s, q) == 0
    torch.cuda.synchronize()
    lr.assert_guards(f"crop_degrade_blind x{s} {D.SOURCES[k]} lr_out")
    hr.assert_guards(f"crop_degrade_blind x{s} {D.SOURCES[k]} hr_out")
    return lr.win.view(B, 3, P, P).clone(), hr.win.view(B, 3, P * s, P * s).clone()


def _run_whole(s, k, noisy, q):
    """srk_degrade_blind_f32 on five copies of the converted region of case (s, k), copy b with the parameters of sample b."""
    _, samples = _pool_case(s, k)
    a = D.case_image(s, k)
    H, W = a.shape[0] // s * s, a.shape[1] // s * s
    B = len(samples)
    x = torch.from_numpy(D.to_unit3(a)[None, :, :H, :W].copy()).cuda().repeat(B, 1, 1, 1).contiguous()
    par = torch.tensor([D.pack(sigma, noise if noisy else (0.0, 0.0), nid, gray) for _, _, sigma, noise, nid, gray in samples],
                       dtype=torch.int64).cuda()
    n = B * 3 * (H // s) * (W // s)
    out = Guarded("f32", 1, n, n)
    assert _whole(x, out.ptr, par, B, 3, H, W, s, q) == 0
    torch.cuda.synchronize()
    out.assert_guards(f"degrade_blind x{s} {D.SOURCES[k]}")
    return out.win.view(B, 3, H // s, W // s).clone()


def _windows(whole, s, k):
    _, samples = _pool_case(s, k)
    return torch.stack([whole[b, :, top // s:top // s + P, left // s:left // s + P] for b, (top, left, *_) in enumerate(samples)])


def _check_quantised(got, ref, bnd, what):
    """Every value is k / 255.0f exactly; k is the reference's level, except where 255 x the reference's unquantised value lies within
    255 x bound of a half-integer, where either neighbouring level passes -- for at most 1 % of a sample."""
    got = np.asarray(got, dtype=np.float32)
    lv = np.rint(got.astype(np.float64) * 255.0)
    assert np.array_equal(got, (lv.astype(np.float32) / np.float32(255)).astype(np.float32)), f"{what}: values that are not k / 255.0f"
    level = D.quant8(ref)[1]
    near = D.near_half(ref, bnd)
    share = near.reshape(len(near), -1).mean(axis=1)
    print(f"{what}: {int((lv != level).sum())} levels differ from the reference, near a half-integer per sample: {np.round(100 * share, 3).tolist()} %")
    assert share.max() <= 0.01, what
    wrong = (lv != level) & ~(near & (np.abs(lv - level) <= 1))
    assert not wrong.any(), f"{what}: {int(wrong.sum())} levels differ from the reference away from a half-integer"


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def test_device_normal():
    """The device's z alone: a zero image, sigma_n = 1, gain = 0, no blur, no rounding -> out = 0 + sqrtf(1) z = z.  Prints the largest
    |z_dev - z| / (u (r + |z|)), the figure C_NOISE is 4 x of, and asserts C_NOISE on these 3 x 2 x 96 x 160 draws."""
    B, C, H, W, s = 2, 3, 192, 320, 2
    x = torch.zeros(B, C, H, W, device="cuda")
    ids = [D.NOISE_ID0, 3]
    par = torch.tensor([D.pack((0.0, 0.0), (1.0, 0.0), nid, False) for nid in ids], dtype=torch.int64).cuda()
    n = B * C * (H // s) * (W // s)
    out = Guarded("f32", 1, n, n)
    assert _whole(x, out.ptr, par, B, C, H, W, s, 0) == 0
    torch.cuda.synchronize()
    out.assert_guards("degrade_blind on zeros")
    got = out.win.view(B, C, H // s, W // s).cpu().numpy().astype(np.float64)
    zr = [D.normal_field(C, 0, 0, H // s, W // s, nid, False) for nid in ids]
    z, r = np.stack([a for a, _ in zr]), np.stack([b for _, b in zr])
    ratio = np.abs(got - z) / (D.U * (r + np.abs(z)))
    print(f"device z against the fp64 reference over {z.size} draws: max |dz| / (u (r + |z|)) = {ratio.max():.3f}; C_NOISE = {D.C_NOISE}; "
          f"mean = {got.mean():.3e}, var = {got.var():.5f}")
    assert ratio.max() <= D.C_NOISE
    assert abs(got.mean()) <= 5.0 / np.sqrt(z.size) and abs(got.var() - 1.0) <= 5.0 * np.sqrt(2.0 / z.size)


# ---- direct calls ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,k", CASES, ids=CASE_IDS)
def test_blind_clean_unquantised(s, k):
    from tpu_superresolution_amd._lib import lib
    pool, samples = _pool_case(s, k)
    B = len(samples)
    ref, bnd = D.case_reference(s, k, False)
    lr, hr = _run(s, k, False, 0)
    err = np.abs(lr.cpu().numpy() - ref)
    print(f"x{s} {D.SOURCES[k]}: max |err| / bound per sample = {np.round((err / bnd).reshape(B, -1).max(axis=1), 3).tolist()} "
          f"(sigmas {[smp[2] for smp in samples]}, bounds {[float(f'{b.max():.2e}') for b in bnd]})")
    assert (err <= bnd).all()
    # the HR patch: bit-identical to srk_paired_crop_u8, whatever the blur
    hd = _desc(s, k, False)[:, :6].contiguous()
    ld = hd.clone()
    ld[:, 4:] //= s
    lr2, hr2 = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
    assert lib().srk_paired_crop_u8(pool.pool.data_ptr(), ld.data_ptr(), hd.data_ptr(), lr2.data_ptr(), hr2.data_ptr(), B, P, s, _stream()) == 0
    assert torch.equal(hr, hr2)
    # sigma (0, 0) without noise: the bits of srk_crop_degrade_u8, at both roundings
    plain = [b for b, smp in enumerate(samples) if smp[2] == (0.0, 0.0)]
    assert len(plain) == 1
    lrq, _ = _run(s, k, False, 8)
    for q, mine in ((0, lr), (8, lrq)):
        lr3, hr3 = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
        assert lib().srk_crop_degrade_u8(pool.pool.data_ptr(), hd.data_ptr(), lr3.data_ptr(), hr3.data_ptr(), B, P, s, q, _stream()) == 0
        assert torch.equal(mine[plain], lr3[plain]) and torch.equal(hr, hr3)
        blurred = [b for b in range(B) if b not in plain]
        assert not torch.equal(mine[blurred], lr3[blurred])
    if D.SOURCES[k] != "rgb8":
        assert torch.equal(lr[:, 0], lr[:, 1]) and torch.equal(lr[:, 0], lr[:, 2])
    # the whole-image form: every patch is its window, bit for bit
    assert torch.equal(lr, _windows(_run_whole(s, k, False, 0), s, k))
    _check_quantised(lrq.cpu().numpy(), ref, bnd, f"x{s} {D.SOURCES[k]} clean")


@pytest.mark.parametrize("s,k", CASES, ids=CASE_IDS)
def test_blind_noisy(s, k):
    _, samples = _pool_case(s, k)
    B = len(samples)
    ref, bnd = D.case_reference(s, k, True)
    clean, _ = D.case_reference(s, k, False)
    lr, hr = _run(s, k, True, 0)
    got = lr.cpu().numpy()
    err = np.abs(got - ref)
    print(f"x{s} {D.SOURCES[k]} noisy: max |err| / bound per sample = {np.round((err / bnd).reshape(B, -1).max(axis=1), 3).tolist()}, "
          f"noise std per sample = {np.round((got - clean).reshape(B, -1).std(axis=1), 4).tolist()}")
    assert (err <= bnd).all()
    assert ((got - clean).reshape(B, -1).std(axis=1) > 0.005).all()
    # the same ids: the same bits on a second launch; the HR patch is untouched by the noise
    lr2, hr2 = _run(s, k, True, 0)
    assert torch.equal(lr, lr2) and torch.equal(hr, hr2) and torch.equal(hr, _run(s, k, False, 0)[1])
    # other ids: other noise, in every sample
    lr3, _ = _run(s, k, True, 0, ids=[smp[4] + 1 for smp in samples])
    assert all((lr3[b] != lr[b]).float().mean() > 0.99 for b in range(B))
    # gray flag (or a gray source): three equal channels; colour noise: three distinct draws
    noise = lr - torch.from_numpy(np.array(clean)).float().cuda()
    for b, smp in enumerate(samples):
        if smp[5]:
            assert torch.equal(lr[b, 0], lr[b, 1]) and torch.equal(lr[b, 0], lr[b, 2]) or D.SOURCES[k] == "rgb8"
            if D.SOURCES[k] == "rgb8":          # one z for the three channels: the reference above holds it to the bound; here only the sign
                assert ((noise[b, 0] * noise[b, 1] > 0).float().mean() > 0.99) and not torch.equal(lr[b, 0], lr[b, 1])
        else:
            assert D.SOURCES[k] == "rgb8"
            cc = np.corrcoef(noise[b].reshape(3, -1).cpu().numpy())
            assert np.abs(cc[np.triu_indices(3, 1)]).max() < 0.1
    # patch == window of the whole-image form, with the rounding
    lrq, _ = _run(s, k, True, 8)
    assert torch.equal(lr, _windows(_run_whole(s, k, True, 0), s, k))
    assert torch.equal(lrq, _windows(_run_whole(s, k, True, 8), s, k))
    _check_quantised(lrq.cpu().numpy(), ref, bnd, f"x{s} {D.SOURCES[k]} noisy")


def test_planted_nan_comes_out_on_the_composed_footprint():
    s, sigma = 3, (0.3, 2.5)
    B, C, H, W = 1, 2, 60, 249
    x = np.random.RandomState(4).rand(B, C, H, W).astype(np.float32)
    ref = D.filtered(x[0], s, *sigma)
    x[0, 1, 31, 100] = np.nan
    par = torch.tensor([D.pack(sigma, (0.0, 0.0), 0, False)], dtype=torch.int64).cuda()
    n = C * (H // s) * (W // s)
    out = Guarded("f32", 1, n, n)
    assert _whole(torch.from_numpy(x).cuda(), out.ptr, par, B, C, H, W, s, 0) == 0
    torch.cuda.synchronize()
    out.assert_guards("degrade_blind with a NaN")
    got = out.win.view(C, H // s, W // s).cpu().numpy()
    want = np.zeros(got.shape, dtype=bool)
    want[1] = D.nan_footprint(H, W, s, sigma, 31, 100)
    plain = np.zeros_like(want)
    plain[1] = D.nan_footprint(H, W, s, (0.0, 0.0), 31, 100)
    assert 0 < plain.sum() < want.sum() < want[1].size
    assert np.array_equal(np.isnan(D.filtered(x[0], s, *sigma)), want)
    assert np.array_equal(np.isnan(got), want)
    assert np.abs(got - ref)[~want].max() <= D.bound(H, W, s, sigma, 1.0)


def test_garbage_parameter_rows_stay_inside():
    """Any bit pattern in slots 6..9: R is clamped to 0..8, the amplitudes to [0, 16] (NaN -> 0); the output stays finite and inside."""
    s, k = 4, 1
    pool, samples = _pool_case(s, k)
    bad = [float("nan"), -1.0, 1e30, float("inf"), -float("inf")]
    rows = []
    for b, (top, left, *_) in enumerate(samples):
        v = bad[b]
        w = bad[(b + 2) % 5]
        rows.append(list(pool.meta[0][1]) + [top, left, D.signed64(D.bits(v) | D.bits(w) << 32), D.signed64(D.bits(w) | D.bits(v) << 32),
                                             -1 - b, -1])
    B = len(rows)
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 3 * P * P * s * s, B * 3 * P * P * s * s)
    assert _blind(pool.pool, torch.tensor(rows, dtype=torch.int64).cuda(), lr.ptr, hr.ptr, B, P, s, 0) == 0
    torch.cuda.synchronize()
    lr.assert_guards("garbage parameters, lr_out")
    hr.assert_guards("garbage parameters, hr_out")
    assert bool(torch.isfinite(lr.win).all()) and bool(torch.isfinite(hr.win).all())
    lrq = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P)
    assert _blind(pool.pool, torch.tensor(rows, dtype=torch.int64).cuda(), lrq.ptr, hr.ptr, B, P, s, 8) == 0
    torch.cuda.synchronize()
    lrq.assert_guards("garbage parameters, quantised lr_out")
    assert bool(((lrq.win >= 0) & (lrq.win <= 1)).all())


def test_error_codes():
    from tpu_superresolution_amd._lib import lib
    s, k = 2, 0
    pool, samples = _pool_case(s, k)
    desc = _desc(s, k, True)
    B = len(samples)
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 12 * P * P, B * 12 * P * P)
    for args in ((None, desc, lr.ptr, hr.ptr), (pool.pool, None, lr.ptr, hr.ptr), (pool.pool, desc, None, hr.ptr), (pool.pool, desc, lr.ptr, None)):
        assert _blind(*args, B, P, 2) == E_NULL
    for b, p, sc, q in ((0, P, 2, 0), (65536, P, 2, 0), (B, 0, 2, 0), (B, 4096, 2, 0), (B, P, 1, 0), (B, P, 5, 0), (B, P, 2, 4), (B, P, 2, 16)):
        assert _blind(pool.pool, desc, lr.ptr, hr.ptr, b, p, sc, q) == E_SHAPE, (b, p, sc, q)
    x = torch.rand(1, 2, 16, 24, device="cuda")
    par = torch.tensor([D.pack((1.0, 1.0), (0.1, 0.0), 1, False)], dtype=torch.int64).cuda()
    n = 2 * 8 * 12
    out = Guarded("f32", 1, n, n)
    for args in ((None, out.ptr, par), (x, None, par), (x, out.ptr, None)):
        assert _whole(*args, 1, 2, 16, 24, 2) == E_NULL
    for shape in ((0, 2, 16, 24, 2), (1, 0, 16, 24, 2), (1, 2, 0, 24, 2), (1, 2, 16, -1, 2), (1, 2, 16, 24, 1), (1, 2, 16, 24, 5),
                  (1, 2, 15, 24, 2), (1, 2, 16, 23, 2), (1, 2, 16, 24, 3)):
        assert _whole(x, out.ptr, par, *shape) == E_SHAPE, shape
    assert _whole(x, out.ptr, par, 1, 2, 16, 24, 2, 4) == E_SHAPE and b"quant_bits" in lib().srk_last_error()
    assert _whole(out.ptr, out.ptr, par, 1, 2, 8, 12, 2) == E_SHAPE and b"overlap" in lib().srk_last_error()
    assert _whole(out.ptr - 4 * (2 * 16 * 24 - 1), out.ptr, par, 1, 2, 16, 24, 2) == E_SHAPE          # windows sharing four bytes
    assert _whole(out.ptr + 4 * (n - 1), out.ptr, par, 1, 2, 16, 24, 2) == E_SHAPE
    torch.cuda.synchronize()
    for g, what in ((lr, "lr_out"), (hr, "hr_out"), (out, "out")):
        g.assert_untouched(f"{what} of a refused call")


def test_degrade_blind_python_entry():
    from tpu_superresolution_amd import ops
    x = torch.rand(2, 3, 25, 34, device="cuda")
    lr, hr = ops.degrade_blind(x, 4, (1.0, 2.0), (0.02, 0.01), [5, 6], gray_noise=[True, False])
    assert hr.shape == (2, 3, 24, 32) and torch.equal(hr, x[..., :24, :32]) and lr.shape == (2, 3, 6, 8)
    ref = np.stack([D.degrade(x[b, :, :24, :32].cpu().numpy(), 4, (1.0, 2.0), (0.02, 0.01), 5 + b, b == 0)[0] for b in range(2)])
    lv = np.rint(lr.cpu().numpy().astype(np.float64) * 255)
    assert np.abs(lv - D.quant8(ref)[1]).max() <= 1 and (lv == D.quant8(ref)[1]).mean() > 0.95
    lr0, _ = ops.degrade_blind(x, 4, (1.0, 2.0), (0.02, 0.01), [5, 6], gray_noise=[True, False], quant_bits=0)
    nb = np.stack([D.degrade(x[b, :, :24, :32].cpu().numpy(), 4, (1.0, 2.0), (0.02, 0.01), 5 + b, b == 0)[1] for b in range(2)])
    assert (np.abs(lr0.cpu().numpy() - ref) <= D.bound(24, 32, 4, (1.0, 2.0), 1.0) + nb).all()
    # per-sample rows, and no blur + no noise = degrade_aa
    lr1, _ = ops.degrade_blind(x, 4, [(1.0, 2.0), (0.0, 0.0)], [(0.02, 0.01), (0.0, 0.0)], [5, 6], gray_noise=[True, False])
    assert torch.equal(lr1[0], lr[0]) and torch.equal(lr1[1], ops.degrade_aa(x, 4)[0][1])
    for bad in (dict(blur=(2.6, 1.0)), dict(blur=(1.0,)), dict(noise=(-0.1, 0.0)), dict(noise=(0.1, 1.5)), dict(noise_ids=[5]), dict(scale=5),
                dict(quant_bits=4), dict(gray_noise=[True]), dict(blur=[(1.0, 1.0)] * 3)):
        with pytest.raises(ValueError):
            ops.degrade_blind(**{"hr": x, "scale": 4, "blur": (1.0, 2.0), "noise": (0.02, 0.01), "noise_ids": [5, 6], **bad})
    with pytest.raises(ValueError):
        ops.degrade_blind(x.cpu(), 4, (1.0, 2.0), (0.0, 0.0), [5, 6])


# ---- DeviceHRPool / SynthLRBatches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", ["none", "d4"])
def test_device_hr_pool_blind_patch_is_the_window_of_degrade_blind(augment):
    import resize_ref as R
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.augment import apply_op_host
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool
    s, Pp = 2, R.PATCH
    imgs = R.pool_images(s)
    spec = DegradeSpec(blur_sigma=(0.2, 2.5), noise_sigma=(0.0, 0.04), noise_gain=(0.0, 0.01), gray_noise_p=0.5, seed=21)
    plain = DeviceHRPool(imgs, Pp, s, augment=augment)
    blind = DeviceHRPool(imgs, Pp, s, augment=augment, degrade=spec, rank=2)
    replay = spec.rng(2)
    for batch in ([0, 1, 1, 0, 0], [2, 3, 2, 1]):
        random.seed(11)
        hd, codes = blind.draw(batch)
        random.seed(11)
        lr0, hr0 = plain.sample(batch)
        state = random.getstate()
        random.seed(11)
        lr, hr = blind.sample(batch)
        assert random.getstate() == state, "the blind pool must consume the global `random` like the plain pool"
        assert torch.equal(hr, hr0) and not torch.equal(lr, lr0)
        assert augment == "none" or any(codes)
        for b, (d, code) in enumerate(zip(hd, codes)):
            a = imgs[batch[b]]
            H, W = a.shape[:2]
            blur, noise, nid, gray = spec.draw(replay, colour=a.ndim == 3)
            reg = torch.from_numpy(R.to_unit3(a)[None, :, :H - H % s, :W - W % s].copy()).cuda()
            whole, _ = ops.degrade_blind(reg, s, blur, noise, [nid], gray, 8)
            win = whole[0, :, d[4] // s:d[4] // s + Pp, d[5] // s:d[5] // s + Pp]
            assert torch.equal(lr[b], apply_op_host(win, code)), (batch, b, code)


def test_synth_lr_batches_fixed_parameters_and_image_index_ids():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.sr_datasets import FixedDegrade, SynthLRBatches
    g = torch.Generator().manual_seed(0)
    gray = torch.rand(2, 1, 21, 30, generator=g).repeat(1, 3, 1, 1)
    colour = torch.rand(2, 3, 21, 30, generator=g)
    fixed = FixedDegrade((1.2, 0.6), (0.03, 0.0))
    batches = list(SynthLRBatches([gray, colour], 2, 8, "cuda", degrade=fixed))
    again = list(SynthLRBatches([gray, colour], 2, 8, "cuda", degrade=fixed))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(batches, again))
    (lr_g, hr_g), (lr_c, hr_c) = batches
    assert torch.equal(hr_g, gray[..., :20, :].cuda()) and lr_g.shape == (2, 3, 10, 15)
    assert torch.equal(lr_g[:, 0], lr_g[:, 1]) and torch.equal(lr_g[:, 0], lr_g[:, 2])          # equal channels in, gray noise, equal channels out
    assert torch.equal(lr_g, ops.degrade_blind(gray.cuda(), 2, fixed.blur, fixed.noise, [0, 1], True)[0])
    assert torch.equal(lr_c, ops.degrade_blind(colour.cuda(), 2, fixed.blur, fixed.noise, [2, 3], False)[0])
    plain = list(SynthLRBatches([gray, colour], 2, 8, "cuda"))
    assert torch.equal(plain[0][0], ops.degrade_aa(gray.cuda(), 2)[0]) and not torch.equal(plain[1][0], lr_c)


# ---- the command lines -------------------------------------------------------------------------------------------------------------------
def test_scripts_train_and_evaluate_blind(tmp_path, capsys, monkeypatch):
    import re

    from test_gpu_resize import _make_hr_only_dataset
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    root = str(tmp_path / "data")
    _make_hr_only_dataset(root)
    monkeypatch.chdir(tmp_path)
    # --lr 0: the weight-gradient kernels accumulate with atomics, so two trainings differ in their last bits; with the weights held,
    # validation depends on the seeded initialisation and on the LR images alone, and must repeat exactly
    base = ["--data_root", root, "--scale", "X4", "--workers", "0", "--lr", "0", "--gpu_data", "--synth_lr", "--epochs", "1", "--batch_size", "2"]
    val = []
    for run in range(2):
        F.main(base + ["--degrade", "blind", "--noise_gain", "0", "0.01"])
        out = capsys.readouterr().out
        assert "[degrade] blind" in out and "[done] best_val_loss=" in out
        m = re.search(r"\[X4\] epoch 001/1 .*train L1=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB", out)
        assert m and all(np.isfinite(float(v)) for v in m.groups())
        val.append(m.groups()[1:])
    assert val[0] == val[1], "validation scores the same LR images in every run"
    args = torch.load(tmp_path / "bestpsnr_swinir_finetune_X4.pt", map_location="cpu", weights_only=False)["args"]
    assert args["degrade"] == "blind" and args["noise_gain"] == [0.0, 0.01]
    assert not {"blur_sigma", "blur_aniso_p", "noise_sigma", "gray_noise_p", "degrade_seed"} & set(args)          # defaults leave no trace
    ev = ["--scale", "X4", "--data_root", root, "--ckpt", str(tmp_path / "bestpsnr_swinir_finetune_X4.pt"), "--batch_size", "1", "--save_dir",
          str(tmp_path / "p"), "--save_n", "1", "--arch", "swinir", "--device", "cuda", "--synth_lr", "--degrade", "blind"]
    res = evaluate.main(ev + ["--blur_sigma", "1.5", "0.5", "--noise_sigma", "8", "--noise_gain", "0.01"])
    assert "[degrade] blind" in capsys.readouterr().out
    assert np.isfinite(res["psnr"]) and np.isfinite(res["ssim"]) and res["n"] == 2
    tiled = evaluate.main(ev + ["--tile", "24", "--tile_overlap", "8", "--self_ensemble"])
    assert np.isfinite(tiled["psnr"]) and tiled["n"] == 2 and tiled["psnr"] != res["psnr"]
