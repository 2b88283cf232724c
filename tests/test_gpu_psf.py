"""srk_blur2d_f32 / srk_crop_degrade_psf_u8 (csrc/blur2d.hip) and what is built on them: ops.blur2d, ops.degrade_psf,
sr_datasets.DeviceHRPool(psf=PsfSpec) and the --blur_kernel / --blur_psf / --blur_theta command lines.  The reference is tests/psf_ref.py
(fp64 numpy, pinned in tests/test_psf_ref.py).

Tolerances (derived in psf_ref's docstring, not tuned): blur 2 (2 n + 2) u S / m per pixel; through the resize Ly Lx max(blur bound) +
2 (Ky + Kx + 4) u Ly Lx max|blurred|; with noise degrade_ref's C_NOISE term on top (sigma_n > 0 in every noisy case).  Quantised outputs
are the reference's level exactly except within the bound of a half-integer, for at most 1 % of a sample -- a condition on the inputs
that tests/test_psf_ref.py asserts from the reference alone.  Everything that can be exact is compared with torch.equal: a patch against
the window of ops.degrade_psf (srk_blur2d_f32, then srk_degrade_blind_f32 at sigma 0) on the whole converted region, the HR patch against
srk_paired_crop_u8, a second launch, a table against its zero-padded form, a delta table (k = 1: psf_ref's bit rule) against a plain copy
and against srk_crop_degrade_u8."""
import functools
import random

import numpy as np
import pytest
import torch

import degrade_ref as D
import psf_ref as Pr
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL = -1, -2
P = Pr.PATCH
CASES = [(s, k) for s in Pr.SCALES for k in range(len(Pr.SOURCES))]
CASE_IDS = [f"x{s}-{Pr.SOURCES[k]}" for s, k in CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _blur(x, psf, out, B, C, H, W, ks):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_blur2d_f32(_ptr(x), _ptr(psf), _ptr(out), B, C, H, W, ks, _stream())


def _psf(pool, desc, psf, ks, lr, hr, B, patch, s, q=0):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_crop_degrade_psf_u8(_ptr(pool), _ptr(desc), _ptr(psf), ks, _ptr(lr), _ptr(hr), B, patch, s, q, _stream())


def _framed(a):
    """The fp32 array `a` on the device inside a frame of NaNs: an operand that a kernel must not read past."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * 4096,), float("nan"), dtype=torch.float32, device="cuda")
    buf[4096:4096 + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return buf, buf[4096:4096 + a.size].view(*a.shape)


# ---- srk_blur2d_f32 ----------------------------------------------------------------------------------------------------------------------
BLUR_SHAPES = [(2, 3, 45, 61), (1, 1, 5, 7), (1, 1, 1, 1), (1, 2, 33, 130)]          # the last one crosses a tile edge in x and in y


def _rand_table(rng, ks):
    t = rng.rand(ks, ks) + 0.02
    return (t / t.sum()).astype(np.float32)


def _run_blur(x, tabs):
    B, C, H, W = x.shape
    ks = tabs.shape[-1]
    _, xd = _framed(x)
    _, kd = _framed(tabs)
    out = Guarded("f32", 1, x.size, x.size)
    assert _blur(xd, kd, out.ptr, B, C, H, W, ks) == 0
    torch.cuda.synchronize()
    out.assert_guards(f"blur2d {x.shape} ks {ks}")
    return out.win.view(B, C, H, W).clone()


@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=["x".join(map(str, s)) for s in BLUR_SHAPES])
@pytest.mark.parametrize("ks", [3, 7, 21])
def test_blur2d_against_the_reference(shape, ks):
    B, C, H, W = shape
    rng = np.random.RandomState(17 * ks + H)
    x = (rng.rand(B, C, H, W) * 2.0 - 0.5).astype(np.float32)
    tabs = np.stack([_rand_table(rng, ks) for _ in range(B)])
    got = _run_blur(x, tabs)
    assert not bool(torch.isnan(got).any()), "the NaN frame around x or psf was read"
    worst = 0.0
    for b in range(B):
        ref, bnd = Pr.blur2d(x[b], tabs[b]), Pr.blur_bound(x[b], tabs[b])
        err = np.abs(got[b].cpu().numpy() - ref)
        worst = max(worst, float((err / bnd).max()))
        assert (err <= bnd).all(), (b, float((err / bnd).max()))
    print(f"blur2d {shape} ks {ks}: max |err| / bound = {worst:.3f}")
    # a second launch, and the table zero-padded to 21: the same bits
    assert torch.equal(got, _run_blur(x, tabs))
    if ks < 21:
        assert torch.equal(got, _run_blur(x, np.stack([Pr.pad_to(t, 21) for t in tabs])))


@pytest.mark.parametrize("shape", BLUR_SHAPES[:3], ids=["x".join(map(str, s)) for s in BLUR_SHAPES[:3]])
def test_blur2d_delta_tables_copy_bit_for_bit(shape):
    """psf_ref's bit rule: K = delta with k = 1 gives fl(fl(1 x) / 1) = x at any ks; k = 0.5 is exact too (a power of two), k = 0.3 is
    x up to the two roundings of x * k / k."""
    B, C, H, W = shape
    x = (np.random.RandomState(5).rand(B, C, H, W) * 4.0 - 2.0).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    for ks in (1, 3, 21):
        assert torch.equal(_run_blur(x, np.stack([Pr.delta(ks)] * B)), xt)
    assert torch.equal(_run_blur(x, np.stack([Pr.pad_to(Pr.delta(3), 21)] * B)), xt)
    assert torch.equal(_run_blur(x, np.stack([Pr.delta(7, 0.5)] * B)), xt)
    k = np.float32(0.3)
    want = ((x * k).astype(np.float32) / k).astype(np.float32)
    assert torch.equal(_run_blur(x, np.stack([Pr.delta(7, k)] * B)), torch.from_numpy(want).cuda())


def test_blur2d_garbage_tables_stay_inside():
    """Any table bits: the kernel checks nothing of them and still writes its window alone (the values are unspecified)."""
    x = np.random.RandomState(6).rand(2, 1, 37, 70).astype(np.float32)
    tabs = np.stack([_rand_table(np.random.RandomState(7), 7)] * 2)
    tabs[0, 2, 3], tabs[0, 3, 3], tabs[1, 0, 0], tabs[1, 6, 6] = np.nan, -np.inf, 1e38, -1.0
    _run_blur(x, tabs)


# ---- srk_crop_degrade_psf_u8 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_case(s, k):
    from tpu_superresolution_amd.sr_datasets import DeviceHRPool
    pool = DeviceHRPool([Pr.case_image(s, k)], P, s)
    return pool, Pr.case_samples(s, k)


def _desc(s, k, noisy, only=None):
    pool, samples = _pool_case(s, k)
    rows = [list(pool.meta[0][1]) + [top, left] + Pr.pack(noise if noisy else (0.0, 0.0), nid, gray)
            for b, (top, left, _, noise, nid, gray) in enumerate(samples) if only is None or b in only]
    return torch.tensor(rows, dtype=torch.int64).cuda()


def _tables(s, k, ks, only=None):
    _, samples = _pool_case(s, k)
    return np.stack([Pr.pad_to(smp[2], ks) for b, smp in enumerate(samples) if only is None or b in only])


def _run(s, k, noisy, q, ks=21, only=None, tabs=None):
    pool, _ = _pool_case(s, k)
    tabs = _tables(s, k, ks, only) if tabs is None else tabs
    B = len(tabs)
    _, kd = _framed(tabs)
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 3 * P * P * s * s, B * 3 * P * P * s * s)
    assert _psf(pool.pool, _desc(s, k, noisy, only), kd, tabs.shape[-1], lr.ptr, hr.ptr, B, P, s, q) == 0
    torch.cuda.synchronize()
    lr.assert_guards(f"crop_degrade_psf x{s} {Pr.SOURCES[k]} lr_out")
    hr.assert_guards(f"crop_degrade_psf x{s} {Pr.SOURCES[k]} hr_out")
    return lr.win.view(B, 3, P, P).clone(), hr.win.view(B, 3, P * s, P * s).clone()


def _windows_of_whole(s, k, noisy, q, tabs=None):
    """ops.degrade_psf on five copies of the converted region, copy b with the table and the parameters of sample b -> the patches' windows."""
    from tpu_superresolution_amd import ops
    _, samples = _pool_case(s, k)
    a = Pr.case_image(s, k)
    H, W = a.shape[0] // s * s, a.shape[1] // s * s
    x = torch.from_numpy(Pr.to_unit3(a)[None, :, :H, :W].copy()).cuda().repeat(len(samples), 1, 1, 1).contiguous()
    whole, _ = ops.degrade_psf(x, s, [smp[2] for smp in samples] if tabs is None else tabs,
                               [smp[3] if noisy else (0.0, 0.0) for smp in samples], [smp[4] for smp in samples], [smp[5] for smp in samples], q)
    return torch.stack([whole[b, :, top // s:top // s + P, left // s:left // s + P] for b, (top, left, *_) in enumerate(samples)])


def _check_quantised(got, ref, bnd, what):
    got = np.asarray(got, dtype=np.float32)
    lv = np.rint(got.astype(np.float64) * 255.0)
    assert np.array_equal(got, (lv.astype(np.float32) / np.float32(255)).astype(np.float32)), f"{what}: values that are not k / 255.0f"
    level = Pr.quant8(ref)[1]
    near = Pr.near_half(ref, bnd)
    share = near.reshape(len(near), -1).mean(axis=1)
    print(f"{what}: {int((lv != level).sum())} levels differ from the reference, undecided per sample: {np.round(100 * share, 3).tolist()} %")
    assert share.max() <= 0.01, what
    wrong = (lv != level) & ~(near & (np.abs(lv - level) <= 1))
    assert not wrong.any(), f"{what}: {int(wrong.sum())} levels differ from the reference away from a half-integer"


@pytest.mark.parametrize("s,k", CASES, ids=CASE_IDS)
def test_psf_clean(s, k):
    from tpu_superresolution_amd._lib import lib
    pool, samples = _pool_case(s, k)
    B = len(samples)
    ref, bnd = Pr.case_reference(s, k, False)
    lr, hr = _run(s, k, False, 0)
    err = np.abs(lr.cpu().numpy() - ref)
    print(f"x{s} {Pr.SOURCES[k]}: max |err| / bound per sample = {np.round((err / bnd).reshape(B, -1).max(axis=1), 3).tolist()} "
          f"(ks {[smp[2].shape[0] for smp in samples]}, bounds {[float(f'{b.max():.2e}') for b in bnd]})")
    assert (err <= bnd).all()
    # the HR patch: bit-identical to srk_paired_crop_u8, whatever the blur
    hd = _desc(s, k, False)[:, :6].contiguous()
    ld = hd.clone()
    ld[:, 4:] //= s
    lr2, hr2 = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
    assert lib().srk_paired_crop_u8(pool.pool.data_ptr(), ld.data_ptr(), hd.data_ptr(), lr2.data_ptr(), hr2.data_ptr(), B, P, s, _stream()) == 0
    assert torch.equal(hr, hr2)
    if Pr.SOURCES[k] != "rgb8":
        assert torch.equal(lr[:, 0], lr[:, 1]) and torch.equal(lr[:, 0], lr[:, 2])
    # a second launch; the whole-image composition: every patch is its window, bit for bit, at both roundings
    lrq, hrq = _run(s, k, False, 8)
    assert torch.equal(lr, _run(s, k, False, 0)[0]) and torch.equal(hr, hrq)
    assert torch.equal(lr, _windows_of_whole(s, k, False, 0))
    assert torch.equal(lrq, _windows_of_whole(s, k, False, 8))
    # a table against its padded form: the samples whose tables are at most 7 x 7, launched at ks 7, against the ks 21 launch
    small = [b for b, smp in enumerate(samples) if smp[2].shape[0] <= 7]
    assert 0 < len(small) < B
    assert torch.equal(_run(s, k, False, 0, ks=7, only=small)[0], lr[small])
    _check_quantised(lrq.cpu().numpy(), ref, bnd, f"x{s} {Pr.SOURCES[k]} clean")


@pytest.mark.parametrize("s,k", CASES, ids=CASE_IDS)
def test_psf_noisy(s, k):
    _, samples = _pool_case(s, k)
    B = len(samples)
    ref, bnd = Pr.case_reference(s, k, True)
    clean, _ = Pr.case_reference(s, k, False)
    lr, hr = _run(s, k, True, 0)
    got = lr.cpu().numpy()
    err = np.abs(got - ref)
    print(f"x{s} {Pr.SOURCES[k]} noisy: max |err| / bound per sample = {np.round((err / bnd).reshape(B, -1).max(axis=1), 3).tolist()}, "
          f"noise std per sample = {np.round((got - clean).reshape(B, -1).std(axis=1), 4).tolist()}")
    assert (err <= bnd).all()
    assert ((got - clean).reshape(B, -1).std(axis=1) > 0.005).all()
    lr2, hr2 = _run(s, k, True, 0)
    assert torch.equal(lr, lr2) and torch.equal(hr, hr2) and torch.equal(hr, _run(s, k, False, 0)[1])
    for b, smp in enumerate(samples):
        if smp[5] and Pr.SOURCES[k] != "rgb8":
            assert torch.equal(lr[b, 0], lr[b, 1]) and torch.equal(lr[b, 0], lr[b, 2])
        elif not smp[5]:
            cc = np.corrcoef((got - clean)[b].reshape(3, -1))
            assert np.abs(cc[np.triu_indices(3, 1)]).max() < 0.1
    lrq, _ = _run(s, k, True, 8)
    assert torch.equal(lr, _windows_of_whole(s, k, True, 0))
    assert torch.equal(lrq, _windows_of_whole(s, k, True, 8))
    _check_quantised(lrq.cpu().numpy(), ref, bnd, f"x{s} {Pr.SOURCES[k]} noisy")


@pytest.mark.parametrize("s", Pr.SCALES)
def test_psf_delta_table_has_the_bits_of_crop_degrade_u8(s):
    """psf_ref's bit rule gives it: with K = delta (k = 1) the blur is a copy, so without noise the entry is srk_crop_degrade_u8."""
    from tpu_superresolution_amd._lib import lib
    k = 1
    pool, samples = _pool_case(s, k)
    B = len(samples)
    hd = _desc(s, k, False)[:, :6].contiguous()
    for q in (0, 8):
        lr3, hr3 = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
        assert lib().srk_crop_degrade_u8(pool.pool.data_ptr(), hd.data_ptr(), lr3.data_ptr(), hr3.data_ptr(), B, P, s, q, _stream()) == 0
        for ks in (1, 21):
            lr, hr = _run(s, k, False, q, tabs=np.stack([Pr.delta(ks)] * B))
            assert torch.equal(lr, lr3) and torch.equal(hr, hr3), (q, ks)


def test_planted_nan_comes_out_on_the_dilated_footprint():
    from tpu_superresolution_amd import ops
    s, ks = 3, 7
    B, C, H, W = 1, 2, 60, 249
    x = np.random.RandomState(4).rand(B, C, H, W).astype(np.float32)
    K = Pr.kernel("gaussian", ks, 1.5, 0.8, 0.7)
    K[0, :] = 0.0                                # zero taps still carry a NaN: the footprint is the whole ks x ks window
    K = (K / K.sum()).astype(np.float32)
    ref, bnd = Pr.filtered(x[0], s, K)
    x[0, 1, 31, 100] = np.nan
    lr, _ = ops.degrade_psf(torch.from_numpy(x).cuda(), s, K, quant_bits=0)
    got = lr[0].cpu().numpy()
    want = np.zeros(got.shape, dtype=bool)
    want[1] = Pr.nan_footprint(H, W, s, ks, 31, 100)
    plain = np.zeros_like(want)
    plain[1] = Pr.nan_footprint(H, W, s, 1, 31, 100)
    assert 0 < plain.sum() < want.sum() < want[1].size
    assert np.array_equal(np.isnan(Pr.filtered(x[0], s, K)[0]), want)
    assert np.array_equal(np.isnan(got), want)
    assert np.abs(got - ref)[~want].max() <= bnd


def test_garbage_tables_and_parameters_stay_inside():
    s, k = 4, 1
    pool, samples = _pool_case(s, k)
    B = len(samples)
    tabs = _tables(s, k, 21).copy()
    tabs[0, 10, 10], tabs[1, 0, 0], tabs[2, 20, 20], tabs[3, 5, 5], tabs[4] = np.nan, np.inf, -1e38, -1.0, 0.0
    bad = [float("nan"), -1.0, 1e30, float("inf"), -float("inf")]
    rows = [list(pool.meta[0][1]) + [top, left, D.signed64(D.bits(bad[b]) | D.bits(bad[(b + 2) % 5]) << 32),
                                     D.signed64(D.bits(bad[(b + 2) % 5]) | D.bits(bad[b]) << 32), -1 - b, -1]
            for b, (top, left, *_) in enumerate(samples)]
    _, kd = _framed(tabs)
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 3 * P * P * s * s, B * 3 * P * P * s * s)
    assert _psf(pool.pool, torch.tensor(rows, dtype=torch.int64).cuda(), kd, 21, lr.ptr, hr.ptr, B, P, s, 8) == 0
    torch.cuda.synchronize()
    lr.assert_guards("garbage tables, lr_out")
    hr.assert_guards("garbage tables, hr_out")
    assert bool(torch.isfinite(hr.win).all())


def test_error_codes():
    from tpu_superresolution_amd._lib import lib
    s, k = 2, 0
    pool, samples = _pool_case(s, k)
    desc = _desc(s, k, True)
    B = len(samples)
    tabs = torch.from_numpy(_tables(s, k, 21)).cuda()
    lr, hr = Guarded("f32", 1, B * 3 * P * P, B * 3 * P * P), Guarded("f32", 1, B * 12 * P * P, B * 12 * P * P)
    for args in ((None, desc, tabs, 21, lr.ptr, hr.ptr), (pool.pool, None, tabs, 21, lr.ptr, hr.ptr), (pool.pool, desc, None, 21, lr.ptr, hr.ptr),
                 (pool.pool, desc, tabs, 21, None, hr.ptr), (pool.pool, desc, tabs, 21, lr.ptr, None)):
        assert _psf(*args, B, P, 2) == E_NULL
    for b, p, sc, q in ((0, P, 2, 0), (65536, P, 2, 0), (B, 0, 2, 0), (B, 4096, 2, 0), (B, P, 1, 0), (B, P, 5, 0), (B, P, 2, 4), (B, P, 2, 16)):
        assert _psf(pool.pool, desc, tabs, 21, lr.ptr, hr.ptr, b, p, sc, q) == E_SHAPE, (b, p, sc, q)
    for ks in (0, -1, 2, 20, 22, 23, 1 << 30):
        assert _psf(pool.pool, desc, tabs, ks, lr.ptr, hr.ptr, B, P, 2, 0) == E_SHAPE and b"ks" in lib().srk_last_error(), ks
    x = torch.rand(1, 2, 16, 24, device="cuda")
    n = 2 * 16 * 24
    out = Guarded("f32", 1, n, n)
    for args in ((None, tabs, out.ptr), (x, None, out.ptr), (x, tabs, None)):
        assert _blur(*args, 1, 2, 16, 24, 21) == E_NULL
    for shape in ((0, 2, 16, 24, 21), (1, 0, 16, 24, 21), (1, 2, 0, 24, 21), (1, 2, 16, -1, 21), (1, 2, 16, 24, 0), (1, 2, 16, 24, 4),
                  (1, 2, 16, 24, 23), (1, 2, 16, 24, -3)):
        assert _blur(x, tabs, out.ptr, *shape) == E_SHAPE, shape
    assert _blur(out.ptr, tabs, out.ptr, 1, 2, 16, 24, 21) == E_SHAPE and b"overlap" in lib().srk_last_error()
    assert _blur(out.ptr - 4 * (n - 1), tabs, out.ptr, 1, 2, 16, 24, 21) == E_SHAPE          # windows sharing four bytes
    assert _blur(x, out.ptr + 4 * (n - 1), out.ptr, 1, 2, 16, 24, 21) == E_SHAPE             # psf inside out
    torch.cuda.synchronize()
    for g, what in ((lr, "lr_out"), (hr, "hr_out"), (out, "out")):
        g.assert_untouched(f"{what} of a refused call")


def test_python_entries():
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd import ops
    x = torch.rand(2, 3, 25, 34, device="cuda")
    tabs = [bk.gaussian(5, 1.0, 2.0, 0.4), bk.plateau(9, 2.0, 1.0, -0.3, 1.5)]
    y = ops.blur2d(x, tabs)
    for b in range(2):
        ref, bnd = Pr.blur2d(x[b].cpu().numpy(), tabs[b]), Pr.blur_bound(x[b].cpu().numpy(), tabs[b])
        assert (np.abs(y[b].cpu().numpy() - ref) <= bnd).all()
    assert torch.equal(ops.blur2d(x, tabs[0])[0], y[0]) and torch.equal(ops.blur2d(x, np.stack([bk.pad_to(t, 9) for t in tabs])), y)
    lr, hr = ops.degrade_psf(x, 4, tabs, (0.02, 0.01), [5, 6], gray_noise=[True, False])
    assert hr.shape == (2, 3, 24, 32) and torch.equal(hr, x[..., :24, :32]) and lr.shape == (2, 3, 6, 8)
    lr0, _ = ops.degrade_psf(x, 4, tabs, (0.02, 0.01), [5, 6], gray_noise=[True, False], quant_bits=0)
    for b in range(2):
        ref, bnd = Pr.degrade(x[b, :, :24, :32].cpu().numpy(), 4, tabs[b], (0.02, 0.01), 5 + b, b == 0)
        assert (np.abs(lr0[b].cpu().numpy() - ref) <= bnd).all()
    # a delta table and no noise = degrade_aa
    assert torch.equal(ops.degrade_psf(x, 4, Pr.delta(3))[0], ops.degrade_aa(x, 4)[0])
    neg = tabs[0].copy()
    neg[0, 0] = -1e-6
    zero_centre = tabs[0].copy()
    zero_centre[2, 2] = 0.0
    for bad in (neg, zero_centre, tabs[0] * 2.0, np.full((4, 4), 1 / 16, np.float32), np.full((23, 23), 1 / 529, np.float32),
                np.full((3, 3), np.nan, np.float32), [tabs[0]] * 3):
        with pytest.raises(ValueError):
            ops.blur2d(x, bad)
    with pytest.raises(ValueError):
        ops.blur2d(x.cpu(), tabs[0])
    with pytest.raises(ValueError):
        ops.degrade_psf(x, 5, tabs[0])


# ---- DeviceHRPool(psf=) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["rotated", "mixed"])
def test_device_hr_pool_psf_patch_is_the_window_of_degrade_psf(mode):
    import resize_ref as R
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.augment import apply_op_host
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool, PsfSpec
    s, Pp = 2, R.PATCH
    imgs = R.pool_images(s)
    spec = DegradeSpec(blur_sigma=(0.2, 2.5), noise_sigma=(0.0, 0.04), noise_gain=(0.0, 0.01), gray_noise_p=0.5, seed=21)
    psf = PsfSpec(mode=mode, seed=21)
    plain = DeviceHRPool(imgs, Pp, s, augment="d4")
    blind = DeviceHRPool(imgs, Pp, s, augment="d4", degrade=spec, rank=2)
    pool = DeviceHRPool(imgs, Pp, s, augment="d4", degrade=spec, rank=2, psf=psf)
    replay, replay_psf = spec.rng(2), psf.rng(2)
    for batch in ([0, 1, 1, 0, 0], [2, 3, 2, 1]):
        random.seed(11)
        hd, codes = pool.draw(batch)
        random.seed(11)
        lr0, hr0 = plain.sample(batch)
        state = random.getstate()
        random.seed(11)
        lrb, _ = blind.sample(batch)
        random.seed(11)
        lr, hr = pool.sample(batch)
        assert random.getstate() == state, "the PSF pool must consume the global `random` like the plain pool"
        assert torch.equal(hr, hr0) and not torch.equal(lr, lr0) and not torch.equal(lr, lrb)
        for b, (d, code) in enumerate(zip(hd, codes)):
            a = imgs[batch[b]]
            H, W = a.shape[:2]
            blur, noise, nid, gray = spec.draw(replay, colour=a.ndim == 3)
            K = psf.draw(replay_psf, blur)
            reg = torch.from_numpy(R.to_unit3(a)[None, :, :H - H % s, :W - W % s].copy()).cuda()
            whole, _ = ops.degrade_psf(reg, s, K, noise, [nid], gray, 8)
            win = whole[0, :, d[4] // s:d[4] // s + Pp, d[5] // s:d[5] // s + Pp]
            assert torch.equal(lr[b], apply_op_host(win, code)), (batch, b, code)
    assert blind._degrade_rng.getstate() == pool._degrade_rng.getstate(), "a PsfSpec must not move the DegradeSpec's generator"


# ---- the command lines -------------------------------------------------------------------------------------------------------------------
def test_scripts_train_and_evaluate_with_2d_kernels(tmp_path, capsys, monkeypatch):
    import re

    from test_gpu_resize import _make_hr_only_dataset
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    root = str(tmp_path / "data")
    _make_hr_only_dataset(root)
    monkeypatch.chdir(tmp_path)
    psf_file = str(tmp_path / "psf.npy")
    np.save(psf_file, np.stack([bk.plateau(9, 2.0, 1.0, 0.4, 1.3), bk.gaussian(9, 1.0, 1.0)]))
    base = ["--data_root", root, "--scale", "X4", "--workers", "0", "--lr", "0", "--gpu_data", "--synth_lr", "--epochs", "1", "--batch_size", "2",
            "--degrade", "blind"]
    val = {}
    for name, extra in (("axis", []), ("mixed", ["--blur_kernel", "mixed"]), ("file", ["--blur_psf", psf_file])):
        F.main(base + extra)
        out = capsys.readouterr().out
        assert ("[degrade] blur kernel" in out) == bool(extra) and "[done] best_val_loss=" in out
        m = re.search(r"\[X4\] epoch 001/1 .*train L1=([0-9.]+) .*val L1=([0-9.]+), PSNR=([0-9.]+)dB", out)
        assert m and all(np.isfinite(float(v)) for v in m.groups())
        val[name] = m.groups()[1:]
    # --lr 0: the weights are the seeded initialisation, so validation depends on the LR images alone.  Generated kernels keep the isotropic
    # midpoints of today's validation; a PSF file scores table 0
    assert val["mixed"] == val["axis"] and val["file"] != val["axis"]
    args = torch.load(tmp_path / "bestpsnr_swinir_finetune_X4.pt", map_location="cpu", weights_only=False)["args"]
    assert args["blur_psf"] == psf_file and not {"blur_kernel", "blur_ksize", "blur_beta_g", "blur_beta_p", "blur_kernel_prob"} & set(args)
    ev = ["--scale", "X4", "--data_root", root, "--ckpt", str(tmp_path / "bestpsnr_swinir_finetune_X4.pt"), "--batch_size", "1", "--save_dir",
          str(tmp_path / "p"), "--save_n", "1", "--arch", "swinir", "--device", "cuda", "--synth_lr", "--degrade", "blind", "--blur_sigma", "2.0", "0.5"]
    plain = evaluate.main(ev)
    capsys.readouterr()
    res = {th: evaluate.main(ev + ["--blur_theta", th]) for th in ("0", "45")}
    assert "[degrade] blur kernel" in capsys.readouterr().out
    assert all(np.isfinite(r["psnr"]) and r["n"] == 2 for r in res.values())
    # theta 0 is the same Gaussian on the 2-D path: another border rule, nearly the same score; 45 degrees is another blur
    assert abs(res["0"]["psnr"] - plain["psnr"]) < 0.5 and res["45"]["psnr"] != res["0"]["psnr"]
    file = evaluate.main(ev + ["--blur_psf", psf_file, "--tile", "24", "--tile_overlap", "8", "--self_ensemble", "--jpeg_quality", "70",
                               "--bench_metric", "y"])
    assert np.isfinite(file["psnr"]) and file["n"] == 2
