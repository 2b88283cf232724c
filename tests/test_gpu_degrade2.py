"""The second-order degradation on the device: srk_filter2d_f32 (csrc/filter2d.hip), srk_resize_aa_ragged_f32 and
srk_jpeg_roundtrip_ragged_f32 (csrc/ragged.hip), srk_crop_u8, and what is built on them: ops.filter2d / resize_aa_ragged /
jpeg_roundtrip_ragged / degrade_second_order and sr_datasets.DeviceHR2Pool.

Ragged is dense: the in-extent output of every sample of a ragged launch is torch.equal to the existing dense entry on that sample
alone; input padding is NaN (a read of it would show), output padding carries a NaN pattern that must keep its bits.
Filter: exact (torch.equal) on integer data, 2 n u S otherwise (tests/filter2d_ref.py derives it; nothing here is tuned), quantised
levels equal to the reference's except within that bound of a half-integer, for at most 1 % of a sample.
Chain: torch.equal to the per-sample composition of the dense ops."""
import random

import numpy as np
import pytest
import torch

import filter2d_ref as Fr
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3
PAT = 0x7FC0BEEF


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _lib():
    from tpu_superresolution_amd._lib import lib
    return lib()


def _filter(x, tab, out, ext, B, C, Hp, Wp, ks, q=0):
    return _lib().srk_filter2d_f32(_ptr(x), _ptr(tab), _ptr(out), _ptr(ext), B, C, Hp, Wp, ks, q, _stream())


def _resize(x, ei, out, eo, B, C, Hp, Wp, Hop, Wop, q=0):
    return _lib().srk_resize_aa_ragged_f32(_ptr(x), _ptr(ei), _ptr(out), _ptr(eo), B, C, Hp, Wp, Hop, Wop, q, _stream())


def _jpeg(x, out, qual, ext, B, C, Hp, Wp, sub=0):
    return _lib().srk_jpeg_roundtrip_ragged_f32(_ptr(x), _ptr(out), _ptr(qual), _ptr(ext), B, C, Hp, Wp, sub, _stream())


def _ext(ext):
    return None if ext is None else torch.tensor(ext, dtype=torch.int32).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """A guarded padded output [B][C][Hp][Wp] prefilled with a NaN pattern."""

    def __init__(self, B, C, Hp, Wp):
        self.g = Guarded("f32", 1, B * C * Hp * Wp, B * C * Hp * Wp)
        self.t = self.g.win.view(B, C, Hp, Wp)
        self.ptr = self.g.ptr

    def check(self, ext, what):
        """Guards intact, padding bit-unchanged; -> the list of in-extent samples."""
        torch.cuda.synchronize()
        self.g.assert_guards(what)
        B, _, Hp, Wp = self.t.shape
        outs = []
        for b in range(B):
            h, w = (Hp, Wp) if ext is None else ext[b]
            pad = torch.ones(Hp, Wp, dtype=torch.bool, device="cuda")
            pad[:h, :w] = False
            assert bool((_bits(self.t[b])[:, pad] == PAT).all()), f"{what}: the output padding of sample {b} was written"
            outs.append(self.t[b, :, :h, :w].clone())
        return outs


EXT = Fr.RAGGED_EXT
HP, WP = Fr.RAGGED_PAD
RESIZE_TARGETS = {
    "up": [(60, 108), (50, 75), (24, 22), (23, 96)],
    "down": [(20, 36), (11, 17), (4, 5), (12, 8)],
    "identity": list(EXT),
    "noninteger": [(29, 47), (40, 41), (7, 13), (31, 50)],
}


# ---- ragged == dense --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("case", list(RESIZE_TARGETS))
def test_resize_ragged_is_dense(case, C):
    from tpu_superresolution_amd import ops
    buf, samples = Fr.ragged_batch(11 + C, C)
    x = torch.from_numpy(buf).cuda()
    eo = RESIZE_TARGETS[case]
    Hop, Wop = max(h for h, _ in eo), max(w for _, w in eo)
    for q in (0, 8):
        out = Out(len(EXT), C, Hop, Wop)
        assert _resize(x, _ext(EXT), out.ptr, _ext(eo), len(EXT), C, HP, WP, Hop, Wop, q) == 0
        got = out.check(eo, f"resize_aa_ragged {case}")
        for b, s in enumerate(samples):
            want = ops.resize_aa(torch.from_numpy(s[None]).cuda(), eo[b], q)[0]
            assert bool(torch.isfinite(got[b]).all()), f"sample {b}: the NaN padding of the input was read"
            assert torch.equal(got[b], want), f"{case} C={C} q={q}: sample {b} differs from srk_resize_aa_f32 on it alone"
        again = Out(len(EXT), C, Hop, Wop)
        assert _resize(x, _ext(EXT), again.ptr, _ext(eo), len(EXT), C, HP, WP, Hop, Wop, q) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.t), _bits(again.t))
    # through ops (q = 8, as the last run above), at the default padding and into a larger padded buffer
    for pad in (None, (Hop + 5, Wop + 9)):
        via = ops.resize_aa_ragged(x, EXT, eo, pad, 8)
        for b, (ho, wo) in enumerate(eo):
            assert torch.equal(via[b, :, :ho, :wo], got[b])


def test_resize_ragged_null_extents_are_the_dense_entry():
    from tpu_superresolution_amd import ops
    x = torch.from_numpy(np.random.RandomState(3).rand(2, 3, 37, 70).astype(np.float32)).cuda()
    for size in ((19, 35), (50, 101), (37, 70)):
        out = Out(2, 3, *size)
        assert _resize(x, None, out.ptr, None, 2, 3, 37, 70, size[0], size[1], 0) == 0
        got = out.check(None, "resize_aa_ragged dense")
        assert torch.equal(torch.stack(got), ops.resize_aa(x, size))
    # one table only: a ragged input into a dense output
    buf, samples = Fr.ragged_batch(5, 1)
    got = ops.resize_aa_ragged(torch.from_numpy(buf).cuda(), EXT, None, (20, 30))
    for b, s in enumerate(samples):
        assert torch.equal(got[b], ops.resize_aa(torch.from_numpy(s[None]).cuda(), (20, 30))[0])


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("sub", [0, 1])
def test_jpeg_ragged_is_dense(sub, C):
    from tpu_superresolution_amd import ops
    buf, samples = Fr.ragged_batch(21 + C, C)
    x = torch.from_numpy(buf).cuda()
    B = len(EXT)
    quals = [0, 5, 75, 100]
    for rot in range(4):
        qs = quals[rot:] + quals[:rot]
        out = Out(B, C, HP, WP)
        assert _jpeg(x, out.ptr, torch.tensor(qs, dtype=torch.int32).cuda(), _ext(EXT), B, C, HP, WP, sub) == 0
        got = out.check(EXT, f"jpeg_roundtrip_ragged sub={sub}")
        for b, s in enumerate(samples):
            want = ops.jpeg_roundtrip(torch.from_numpy(s[None]).cuda(), qs[b], bool(sub))[0]
            assert bool(torch.isfinite(got[b]).all())
            assert torch.equal(got[b], want), f"sub={sub} C={C}: sample {b} at quality {qs[b]} differs from srk_jpeg_roundtrip_f32 on it alone"
        again = ops.jpeg_roundtrip_ragged(x, qs, EXT, bool(sub))
        for b, (h, w) in enumerate(EXT):
            assert torch.equal(again[b, :, :h, :w], got[b])
    # ext == NULL: the dense entry
    d = torch.from_numpy(np.random.RandomState(4).rand(2, C, 37, 70).astype(np.float32)).cuda()
    out = Out(2, C, 37, 70)
    assert _jpeg(d, out.ptr, torch.tensor([60, 0], dtype=torch.int32).cuda(), None, 2, C, 37, 70, sub) == 0
    assert torch.equal(torch.stack(out.check(None, "jpeg dense")), ops.jpeg_roundtrip(d, [60, 0], bool(sub)))


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("ks", [7, 21])
def test_filter_ragged_is_dense(ks, C):
    """(12, 11) under ks 21 is the extent of R + 1."""
    from tpu_superresolution_amd import blur_kernels as bk, ops
    buf, samples = Fr.ragged_batch(31 + C, C)
    x = torch.from_numpy(buf).cuda()
    B = len(EXT)
    tabs = np.stack([bk.sinc(np.pi / 2, ks), Fr.pad_to(bk.gaussian(5, 1.0, 0.6, 0.3), ks), bk.sinc(np.pi / 4, ks), Fr.delta(ks)])
    for q in (0, 8):
        out = Out(B, C, HP, WP)
        assert _filter(x, torch.from_numpy(tabs).cuda(), out.ptr, _ext(EXT), B, C, HP, WP, ks, q) == 0
        got = out.check(EXT, f"filter2d ragged ks {ks}")
        for b, s in enumerate(samples):
            want = Out(1, C, *EXT[b])
            assert _filter(torch.from_numpy(s[None]).cuda(), torch.from_numpy(tabs[b:b + 1]).cuda(), want.ptr, None, 1, C, EXT[b][0], EXT[b][1], ks, q) == 0
            assert bool(torch.isfinite(got[b]).all()), f"sample {b}: the NaN padding of the input was read"
            assert torch.equal(got[b], want.check(None, "filter2d dense")[0]), f"ks {ks} C={C} q={q}: sample {b} differs from the dense launch on it alone"
            if q == 0:
                ref, bnd = Fr.filter2d(s, tabs[b]), Fr.bound(s, tabs[b])
                assert (np.abs(got[b].cpu().numpy() - ref) <= bnd).all()
        again = ops.filter2d(x, list(tabs), EXT, q)
        for b, (h, w) in enumerate(EXT):
            assert torch.equal(again[b, :, :h, :w], got[b])


def test_filter_sample_smaller_than_the_padded_radius():
    """A batch of mixed table sizes is padded to the largest; a sample no larger than THAT radius (but larger than its own table's) still
    gets the bits of its own table on it alone: the added taps are zeros on in-extent pixels."""
    from tpu_superresolution_amd import blur_kernels as bk, ops
    ext = [(40, 72), (9, 9), (4, 10), (10, 5)]
    buf, samples = Fr.ragged_batch(77, 3, ext=ext)
    tabs = [bk.sinc(1.2, 21), bk.sinc(2.0, 7), bk.sinc(2.5, 7), bk.gaussian(9, 1.5, 0.7, 0.2)]
    got = ops.filter2d(torch.from_numpy(buf).cuda(), tabs, ext)
    for b, (s, (h, w)) in enumerate(zip(samples, ext)):
        assert torch.equal(got[b, :, :h, :w], ops.filter2d(torch.from_numpy(s[None]).cuda(), tabs[b])[0]), b


def test_garbage_extents_stay_inside():
    """Any bit pattern in ext: the kernels clamp it into the padded buffer (the values are then unspecified)."""
    x = torch.from_numpy(np.random.RandomState(8).rand(4, 3, HP, WP).astype(np.float32)).cuda()
    bad = _ext([(0, -5), (10 ** 9, 3), (-2 ** 31, 2 ** 31 - 1), (HP + 1, WP + 1)])
    tab = torch.from_numpy(np.stack([Fr.int_table(np.random.RandomState(1), 5)] * 4)).cuda()
    for run in (lambda o: _filter(x, tab, o, bad, 4, 3, HP, WP, 5), lambda o: _resize(x, bad, o, bad, 4, 3, HP, WP, HP, WP),
                lambda o: _jpeg(x, o, torch.tensor([50, 0, 90, 10], dtype=torch.int32).cuda(), bad, 4, 3, HP, WP, 1)):
        out = Out(4, 3, HP, WP)
        assert run(out.ptr) == 0
        torch.cuda.synchronize()
        out.g.assert_guards("garbage extents")


# ---- the filter against the reference ---------------------------------------------------------------------------------------------------
FILTER_SHAPES = [(2, 3, 45, 61), (1, 2, 33, 130), (1, 1, 11, 11)]          # the second crosses a tile edge in x and in y; the third is R + 1 at ks 21


def _run_filter(x, tabs, q=0):
    B, C, H, W = x.shape
    out = Out(B, C, H, W)
    assert _filter(torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(tabs)).cuda(), out.ptr, None, B, C, H, W, tabs.shape[-1], q) == 0
    return torch.stack(out.check(None, f"filter2d {x.shape} ks {tabs.shape[-1]}"))


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=["x".join(map(str, s)) for s in FILTER_SHAPES])
@pytest.mark.parametrize("ks", [1, 3, 7, 21])
def test_filter_integer_data_is_exact(shape, ks):
    """Taps in -3..3 (asymmetric) on levels 0..31: every partial sum is an integer below 2^24, so fp32 is exact in any order."""
    B, C, H, W = shape
    rng = np.random.RandomState(100 + ks + H)
    x = rng.randint(0, 32, size=shape).astype(np.float32)
    tabs = np.stack([Fr.int_table(rng, ks) for _ in range(B)])
    assert ks == 1 or not np.array_equal(tabs[0], tabs[0].T) and not np.array_equal(tabs[0], tabs[0][::-1, ::-1])
    got = _run_filter(x, tabs)
    want = np.stack([Fr.filter2d(x[b], tabs[b]) for b in range(B)])
    assert torch.equal(got, torch.from_numpy(want.astype(np.float32)).cuda())


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=["x".join(map(str, s)) for s in FILTER_SHAPES])
@pytest.mark.parametrize("ks", [7, 13, 21])
def test_filter_sinc_and_gaussian_tables(shape, ks):
    from tpu_superresolution_amd import blur_kernels as bk
    B, C, H, W = shape
    rng = np.random.RandomState(7 * ks + W)
    x = (rng.rand(*shape) * 1.5 - 0.25).astype(np.float32)
    tabs = np.stack([bk.sinc(np.pi / 3 + 0.4 * b, ks) if b % 2 == 0 else bk.gaussian(ks, 1.7, 0.8, 0.5) for b in range(B)])
    got = _run_filter(x, tabs)
    worst = 0.0
    for b in range(B):
        err, bnd = np.abs(got[b].cpu().numpy() - Fr.filter2d(x[b], tabs[b])), Fr.bound(x[b], tabs[b])
        worst = max(worst, float((err / bnd).max()))
        assert (err <= bnd).all(), (b, float((err / bnd).max()))
    print(f"filter2d {shape} ks {ks}: max |err| / bound = {worst:.3f}")
    assert torch.equal(got, _run_filter(x, tabs))
    if ks < 21:
        assert torch.equal(got, _run_filter(x, np.stack([Fr.pad_to(t, 21) for t in tabs])))


def test_filter_delta_copies_bits():
    x = (np.random.RandomState(5).rand(2, 3, 37, 70) * 4.0 - 2.0).astype(np.float32)
    xi = x.view(np.int32)
    xi[0, 0, 0, :6] = [0x7FC0BEEF, 0x7F800001, -0x80000000, 0x7F800000, -0x00800000, 0x00000001]          # NaNs with payloads, -0, inf, -inf, a denormal
    xi[1, 2, 36, 69] = 0x7FA12345
    xt = torch.from_numpy(x).cuda()
    for ks in (1, 3, 21):
        assert torch.equal(_bits(_run_filter(x, np.stack([Fr.delta(ks)] * 2))), _bits(xt)), ks
    # one delta sample beside a filtered one: the pass-through is per sample
    from tpu_superresolution_amd import blur_kernels as bk
    x[0, 0, 0, :6] = 0.5
    x[1, 2, 36, 69] = 0.25
    got = _run_filter(x, np.stack([Fr.delta(7), bk.sinc(2.0, 7)]))
    assert torch.equal(_bits(got[0]), _bits(torch.from_numpy(x[0]).cuda()))
    assert (np.abs(got[1].cpu().numpy() - Fr.filter2d(x[1], bk.sinc(2.0, 7))) <= Fr.bound(x[1], bk.sinc(2.0, 7))).all()


@pytest.mark.parametrize("ks", [7, 13, 21])
def test_filter_quantised_levels(ks):
    from tpu_superresolution_amd import blur_kernels as bk
    x = np.stack([Fr.dim_image(40 + b, channels=3) for b in range(2)])
    tabs = np.stack([bk.sinc(np.pi / 3, ks), bk.sinc(2.5, ks)])
    got = _run_filter(x, tabs, 8).cpu().numpy()
    lv = np.rint(got.astype(np.float64) * 255.0)
    assert np.array_equal(got, (lv.astype(np.float32) / np.float32(255)).astype(np.float32)), "values that are not k / 255.0f"
    for b in range(2):
        ref, bnd = Fr.filter2d(x[b], tabs[b]), Fr.bound(x[b], tabs[b])
        level, near = Fr.quant8(ref)[1], Fr.near_half(ref, bnd)
        print(f"ks {ks} sample {b}: {int((lv[b] != level).sum())} levels differ, {100 * near.mean():.3f} % undecided")
        assert near.mean() <= 0.01
        wrong = (lv[b] != level) & ~(near & (np.abs(lv[b] - level) <= 1))
        assert not wrong.any(), f"{int(wrong.sum())} levels differ from the reference away from a half-integer"


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
S, P, M = 2, 16, 4
E = S * (P + 2 * M)


def _chain_params():
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd.ops import SecondOrder
    g = bk.gaussian(9, 1.4, 0.7, 0.4)
    return [
        SecondOrder(g, 1.3, (0.02, 0.0), False, 60, bk.sinc(1.8, 7), 0.9, (0.03, 0.01), True, 45, False, bk.sinc(2.2, 13), 11),          # up, order A
        SecondOrder(bk.sinc(1.5, 11), 0.4, (0.01, 0.02), True, 90, bk.delta(), 1.2, (0.05, 0.0), False, 30, True, bk.delta(), 12),          # down, order B
        SecondOrder(bk.plateau(7, 1.0, 2.0, 1.0, 1.5), 1.0, (0.0, 0.0), False, 35, g, 1.0, (0.02, 0.0), False, 95, True, bk.sinc(3.0, 21), 13),          # keep
        SecondOrder(g, 0.7, (0.04, 0.0), False, 75, bk.gaussian(5, 0.8, 0.8), 0.55, (0.0, 0.0), True, 50, False, bk.sinc(1.0, 7), 2 ** 63 + 5),
    ]


def _compose(x1, s, p, sub=False):
    """The chain of ONE sample from the dense ops alone."""
    from tpu_superresolution_amd import ops
    H, W = x1.shape[-2:]
    z1, z2, zo = ops.second_order_sizes(H, W, s, p)
    i1, i2 = ops.second_order_noise_ids(p)
    a = ops.filter2d(x1, p.k1)
    a = ops.resize_aa(a, z1)
    a = ops.noise(a, p.noise1, [i1], p.gray1)
    a = ops.jpeg_roundtrip(a, p.q1, sub)
    a = ops.filter2d(a, p.k2)
    a = ops.resize_aa(a, z2)
    a = ops.noise(a, p.noise2, [i2], p.gray2)
    if not p.jpeg_last:
        a = ops.jpeg_roundtrip(a, p.q2, sub)
    a = ops.resize_aa(a, zo)
    a = ops.filter2d(a, p.k3, quant_bits=8)
    return ops.jpeg_roundtrip(a, p.q2, sub) if p.jpeg_last else a


@pytest.mark.parametrize("C", [3, 1])
def test_chain_is_the_composition_of_the_dense_ops(C):
    from tpu_superresolution_amd import ops
    ps = _chain_params()
    x = torch.from_numpy(np.random.RandomState(60 + C).rand(4, C, E, E).astype(np.float32)).cuda()
    for sub in (False, True):
        got = ops.degrade_second_order(x, S, ps, sub)
        assert got.shape == (4, C, E // S, E // S)
        for b, p in enumerate(ps):
            assert torch.equal(got[b:b + 1], _compose(x[b:b + 1], S, p, sub)), f"C={C} sub={sub}: sample {b} differs from the dense composition"
            # the sample alone, and inside larger padded buffers kept between calls
            assert torch.equal(got[b:b + 1], ops.degrade_second_order(x[b:b + 1], S, [p], sub))
        bufs = {}
        big = ops.degrade_second_order(x, S, ps, sub, pads=((80, 90), (40, 33)), bufs=bufs)
        assert torch.equal(big, got) and torch.equal(ops.degrade_second_order(x, S, ps, sub, pads=((80, 90), (40, 33)), bufs=bufs), got)
    g = got.cpu().numpy()
    assert np.array_equal(g, (np.rint(g.astype(np.float64) * 255.0).astype(np.float32) / np.float32(255)).astype(np.float32)), "values that are not k / 255.0f"


def test_chain_identity_is_the_quantised_resize():
    from tpu_superresolution_amd import blur_kernels as bk, ops
    d = bk.delta()
    ident = ops.SecondOrder(d, 1.0, (0.0, 0.0), False, 0, d, 1.0, (0.0, 0.0), False, 0, False, d, 0)
    x = torch.from_numpy(np.random.RandomState(9).rand(2, 3, E, E).astype(np.float32)).cuda()
    for last in (False, True):
        got = ops.degrade_second_order(x, S, [ident._replace(jpeg_last=last)] * 2)
        assert torch.equal(got, ops.resize_aa(x, (E // S, E // S), 8))


# ---- the pool ---------------------------------------------------------------------------------------------------------------------------
def _pool(images, seed=3, **kw):
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHR2Pool, SecondOrderSpec
    return DeviceHR2Pool(images, P, S, SecondOrderSpec(seed=seed), DegradeSpec(seed=seed), margin=M, **kw)


def test_pool_patches_are_windows_of_the_window_chain():
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd.augment import dihedral
    rng = np.random.RandomState(70)
    images = [rng.randint(0, 256, size=(E + 7, E + 20, 3), dtype=np.uint8), rng.randint(0, 256, size=(E + 1, E, 1), dtype=np.uint8),
              rng.randint(0, 65536, size=(2 * E, E + 33, 3)).astype(np.uint16)]
    idx = [0, 1, 2, 0, 2, 1]
    a, b = _pool(images, augment="d4"), _pool(images, augment="d4")
    clamped = 0
    for step in range(3):
        random.seed(100 + step)
        lr, hr = a.sample(idx)
        random.seed(100 + step)
        hd, codes = b.draw(idx)
        wd, offs, params = b.draw_second_order(hd)
        clamped += sum(o != (M, M) for o in offs)
        # the HR patch: srk_paired_crop_u8's
        B = len(idx)
        hdt = torch.tensor(hd, dtype=torch.int64).cuda()
        ldt = hdt.clone()
        ldt[:, 4:] //= S
        lr2, hr2 = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * S, P * S, device="cuda")
        assert _lib().srk_paired_crop_u8(b.pool.data_ptr(), ldt.data_ptr(), hdt.data_ptr(), lr2.data_ptr(), hr2.data_ptr(), B, P, S, _stream()) == 0
        whole = ops.degrade_second_order(b._crop(b.pool, wd, E), S, params)
        want = torch.stack([whole[k, :, oy:oy + P, ox:ox + P] for k, (oy, ox) in enumerate(offs)])
        ops_t = torch.tensor(codes, dtype=torch.int32).cuda()
        assert torch.equal(hr, dihedral(hr2, ops_t) if any(codes) else hr2)
        assert torch.equal(lr, dihedral(want, ops_t) if any(codes) else want)
        for k, ((ho, hh, hw, hc, top, left), (_, _, _, _, wt, wl), (oy, ox)) in enumerate(zip(hd, wd, offs)):
            assert 0 <= wt <= hh - hh % S - E and 0 <= wl <= hw - hw % S - E and wt + oy * S == top and wl + ox * S == left
    assert clamped > 0, "no patch of this test clamped its window: the corner case is not covered"
    # the same random state cuts the same HR patches as DeviceHRPool
    from tpu_superresolution_amd.sr_datasets import DeviceHRPool
    random.seed(5)
    want = DeviceHRPool(images, P, S).draw(idx)
    random.seed(5)
    assert _pool(images).draw(idx) == want


def test_pool_refuses_an_image_smaller_than_the_window():
    img = np.zeros((E - 1, E + 10, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="tiny.png"):
        _pool([np.zeros((E, E, 3), dtype=np.uint8), img], names=["ok.png", "tiny.png"])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from tpu_superresolution_amd import blur_kernels as bk, ops
    from tpu_superresolution_amd._lib import SrkUnsupported
    x = torch.zeros(2, 3, 24, 40, device="cuda")
    o = torch.zeros(2, 3, 24, 40, device="cuda")
    tab = torch.zeros(2, 7, 7, device="cuda")
    e = _ext([(24, 40), (10, 9)])
    q = torch.tensor([50, 0], dtype=torch.int32).cuda()
    # srk_filter2d_f32
    assert _filter(None, tab, o, e, 2, 3, 24, 40, 7) == E_NULL and _filter(x, None, o, e, 2, 3, 24, 40, 7) == E_NULL
    assert _filter(x, tab, None, e, 2, 3, 24, 40, 7) == E_NULL
    for ks in (0, 2, 8, 23, -7):
        assert _filter(x, tab, o, e, 2, 3, 24, 40, ks) == E_SHAPE
    assert _filter(x, tab, o, e, 0, 3, 24, 40, 7) == E_SHAPE and _filter(x, tab, o, e, 2, 0, 24, 40, 7) == E_SHAPE
    assert _filter(x, tab, o, e, 2, 3, 3, 40, 7) == E_SHAPE and _filter(x, tab, o, e, 2, 3, 24, 3, 7) == E_SHAPE          # an extent <= R
    assert _filter(x, tab, o, e, 2, 3, 24, 40, 7, 3) == E_SHAPE
    assert _filter(x, tab, x, e, 2, 3, 24, 40, 7) == E_SHAPE and _filter(x, o, o, e, 1, 1, 24, 40, 7) == E_SHAPE          # overlaps
    # srk_resize_aa_ragged_f32
    assert _resize(None, e, o, e, 2, 3, 24, 40, 24, 40) == E_NULL and _resize(x, e, None, e, 2, 3, 24, 40, 24, 40) == E_NULL
    assert _resize(x, e, o, e, 2, 3, 24, 40, 0, 40) == E_SHAPE and _resize(x, e, o, e, 2, 3, 24, 0, 24, 40) == E_SHAPE
    assert _resize(x, e, o, e, 2, 3, 24, 40, 24, 40, 4) == E_SHAPE and _resize(x, e, x, e, 2, 3, 24, 40, 24, 40) == E_SHAPE
    assert _resize(x, None, o, None, 2, 3, 24, 40, 2, 40) == E_UNSUPPORTED and _resize(x, None, o, None, 2, 3, 24, 40, 3, 4) == E_UNSUPPORTED
    assert _resize(x, None, o, None, 2, 3, 24, 40, 3, 5) == 0
    with pytest.raises(SrkUnsupported):
        ops.resize_aa_ragged(x, [(24, 40), (10, 9)], [(24, 40), (1, 9)])
    # srk_jpeg_roundtrip_ragged_f32
    assert _jpeg(None, o, q, e, 2, 3, 24, 40) == E_NULL and _jpeg(x, None, q, e, 2, 3, 24, 40) == E_NULL and _jpeg(x, o, None, e, 2, 3, 24, 40) == E_NULL
    assert _jpeg(x, o, q, e, 2, 2, 24, 40) == E_SHAPE and _jpeg(x, o, q, e, 2, 3, 24, 40, 2) == E_SHAPE and _jpeg(x, o, q, e, 2, 3, 0, 40) == E_SHAPE
    assert _jpeg(x, x, q, e, 2, 3, 24, 40) == E_SHAPE
    # srk_crop_u8
    pool, d = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda")
    crop = lambda *a: _lib().srk_crop_u8(*[_ptr(v) for v in a], _stream())          # noqa: E731
    assert crop(None, d, o, 1, 2) == E_NULL and crop(pool, None, o, 1, 2) == E_NULL and crop(pool, d, None, 1, 2) == E_NULL
    assert crop(pool, d, o, 0, 2) == E_SHAPE and crop(pool, d, o, 1, 0) == E_SHAPE and crop(pool, d, o, 1, 8193) == E_SHAPE
    torch.cuda.synchronize()
    # the host rules of ops
    with pytest.raises(ValueError):
        ops.filter2d(x, np.full((3, 3), 0.5, dtype=np.float32))          # sums to 4.5
    with pytest.raises(ValueError):
        ops.filter2d(x, bk.sinc(1.0, 21), [(24, 40), (10, 9)])          # an extent <= R
    ops.filter2d(x, [bk.sinc(1.0, 21), bk.sinc(1.0, 7)], [(24, 40), (10, 9)])          # R of the sample's own table counts, not of the padded one
    with pytest.raises(ValueError):
        ops.filter2d(x, Fr.delta(3), [(25, 40), (10, 9)])          # an extent outside the padded buffer
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip_ragged(x, [50, 101], [(24, 40), (10, 9)])
