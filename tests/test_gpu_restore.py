"""The scale-1 restoration pairs on the device (csrc/restore.hip: srk_noise_f32, srk_crop_restore_u8) against tests/restore_ref.py.

Exact (torch.equal): the clean target against the host conversion and ops.to_gray; the degraded patch against the WINDOW of
ops.restore_degrade (srk_noise_f32, then srk_jpeg_roundtrip_f32) on the whole converted image, at every offset, phase, quality and
subsampling -- the entries share their device routines; quality 0 with sigma 0 against the clean target; a second launch; a sample
alone; ops.noise with zero amplitudes against a copy; a gray source in three channels against its one-channel output repeated.
Bounded: srk_noise_f32 against the fp64 reference within restore_ref.noised's bound -- the 7k noise term (degrade_ref.C_NOISE, not
re-tuned) plus the roundings of the sum and of the amplitude; quantised, decided pixels equal the reference's level and undecided ones
may take either neighbour (tests/test_restore_ref.py caps their share from the reference alone).
JPEG itself has no further parity here: it is pinned by the window identity plus tests/test_gpu_jpeg.py.
Outputs go through guarded buffers; the pool's images are surrounded by NaN bytes."""
import numpy as np
import pytest
import torch

import degrade_ref as D
import restore_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL = -1, -2
PAD = 4096          # bytes of 0xFF (fp32 / fp16 NaN patterns, u8 255) before, between and after the images of a pool


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if isinstance(t, int) or t is None else t.data_ptr()


def _pool():
    """-> (device uint8 pool, [(byte offset, H, W, C | wide << 8)] per image of restore_ref.SOURCES)"""
    chunks, meta, off = [np.full(PAD, 0xFF, np.uint8)], [], PAD
    for k in range(len(R.SOURCES)):
        a = R.case_image(k)
        wide = int(a.dtype == np.uint16)
        meta.append((off, a.shape[0], a.shape[1], (1 if a.ndim == 2 else 3) | (wide << 8)))
        flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        pad = PAD + (-(off + flat.size)) % 2
        chunks += [flat, np.full(pad, 0xFF, np.uint8)]
        off += flat.size + pad
    return torch.from_numpy(np.concatenate(chunks)).cuda(), meta


@pytest.fixture(scope="module")
def pool():
    return _pool()


def _desc(meta, k, offs, qualities, sigma, ids, grays):
    from tpu_superresolution_amd.ops import pack_restore_params
    return [tuple(meta[k]) + tuple(o) + tuple(pack_restore_params(q, (sigma, 0.0), i, g)) for o, q, i, g in zip(offs, qualities, ids, grays)]


def _raw(pool_t, desc, clean, degraded, B, P, oc, sub, qb):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_crop_restore_u8(_ptr(pool_t), _ptr(desc), _ptr(clean), _ptr(degraded), B, P, oc, sub, qb, _stream())


def _run(pool_t, rows, P, oc, sub, qb):
    """-> (clean, degraded) [B,oc,P,P] on the device, with the guards of both outputs checked"""
    B = len(rows)
    desc = torch.tensor(rows, dtype=torch.int64).cuda()
    gc, gd = Guarded("f32", B * oc * P, P, P), Guarded("f32", B * oc * P, P, P)
    assert _raw(pool_t, desc, gc.ptr, gd.ptr, B, P, oc, sub, qb) == 0
    torch.cuda.synchronize()
    gc.assert_guards(f"crop_restore clean P={P} oc={oc}")
    gd.assert_guards(f"crop_restore degraded P={P} oc={oc}")
    return gc.win.view(B, oc, P, P).clone(), gd.win.view(B, oc, P, P).clone()


def _expand(t, oc):
    return t if t.shape[1] == oc else t.repeat(1, oc, 1, 1)


@pytest.mark.parametrize("P", [20, 32])
@pytest.mark.parametrize("oc", [1, 3])
@pytest.mark.parametrize("k", range(len(R.SOURCES)))
def test_clean_and_the_window_identity(pool, k, oc, P):
    from tpu_superresolution_amd import ops
    pool_t, meta = pool
    a = R.case_image(k)
    offs = R.offsets(k, P)
    x = torch.from_numpy(R.convert(a, oc)).cuda()          # the coded planes [Cc,H,W] of the whole converted image
    want_clean = torch.stack([_expand(x[None], oc)[0][:, t:t + P, l:l + P] for t, l in offs])
    if a.ndim == 3 and oc == 1:          # the same through the public CPU luma
        g = ops.to_gray(a).astype(np.float32) / np.float32(65535.0 if a.dtype == np.uint16 else 255.0)
        assert torch.equal(x[0].cpu(), torch.from_numpy(g))
    ids = [R.NOISE_ID0 + 7 * b + k for b in range(5)]
    for sub in (0, 1):
        for sigma, gray in ((0.0, False), (R.SIGMA, False), (R.SIGMA, True)):
            for qb in (0, 8):
                qs = list(R.QUALITIES[sub:]) + list(R.QUALITIES[:sub])          # the pass-through moves to another offset with sub
                grays = [gray] * 5
                what = f"image {k} oc {oc} P {P} sub {sub} sigma {sigma:.3f} gray {gray} bits {qb}"
                clean, degr = _run(pool_t, _desc(meta, k, offs, qs, sigma, ids, grays), P, oc, sub, qb)
                assert torch.equal(clean, want_clean), what
                whole = _expand(ops.restore_degrade(x[None].repeat(5, 1, 1, 1), (sigma, 0.0), ids, grays, qs, bool(sub), qb), oc)
                for b, (t, l) in enumerate(offs):
                    assert torch.equal(degr[b], whole[b, :, t:t + P, l:l + P]), f"{what}: sample {b} at {(t, l)} quality {qs[b]}"
                if sigma == 0.0 and qb == 0:
                    assert torch.equal(degr[qs.index(0)], clean[qs.index(0)]), what
    # a second launch, and a sample alone
    rows = _desc(meta, k, offs, R.QUALITIES, R.SIGMA, ids, [False] * 5)
    c1, d1 = _run(pool_t, rows, P, oc, 1, 0)
    c2, d2 = _run(pool_t, rows, P, oc, 1, 0)
    assert torch.equal(c1, c2) and torch.equal(d1, d2)
    c3, d3 = _run(pool_t, rows[2:3], P, oc, 1, 0)
    assert torch.equal(c3[0], c1[2]) and torch.equal(d3[0], d1[2])


def test_a_gray_source_in_three_channels_is_its_one_channel_output_repeated(pool):
    pool_t, meta = pool
    P, offs, ids = 32, R.offsets(1, 32), list(range(5))
    for sub in (0, 1):
        rows = _desc(meta, 1, offs, R.QUALITIES, R.SIGMA, ids, [False, True, False, True, False])
        c1, d1 = _run(pool_t, rows, P, 1, sub, 0)
        c3, d3 = _run(pool_t, rows, P, 3, sub, 0)
        assert torch.equal(c3, c1.repeat(1, 3, 1, 1)) and torch.equal(d3, d1.repeat(1, 3, 1, 1))


def test_quality_words_outside_0_100_are_clamped(pool):
    """The host refuses them (ops.pack_restore_params); the kernel reads the low word of slot 6 as an int32 and clamps it."""
    from tpu_superresolution_amd import ops
    pool_t, meta = pool
    for bad in (101, -1, 2.5, True):
        with pytest.raises(ValueError):
            ops.pack_restore_params(bad, (0.0, 0.0), 0, False)
    base = _desc(meta, 0, [(3, 5)] * 4, [100, 100, 0, 0], 0.0, [1] * 4, [False] * 4)
    words = [250, 0x7FFFFFFF, 0xFFFFFFFB, (7 << 32) | 0x80000000]          # > 100 -> 100; negative int32 low words -> 0 (the high word is not read)
    rows = [r[:6] + (D.signed64(w),) + r[7:] for r, w in zip(base, words)]
    _, want = _run(pool_t, base, 20, 3, 0, 0)
    _, got = _run(pool_t, rows, 20, 3, 0, 0)
    assert torch.equal(got, want)


def test_noise_with_zero_amplitudes_is_a_copy():
    from tpu_superresolution_amd import ops
    x = torch.randn(2, 3, 33, 50, device="cuda")
    xi = x.view(torch.int32)
    xi[0, 0, 0, :4] = torch.tensor([0x7FC0BEEF, -1, 0x7F800001, -(1 << 31)], dtype=torch.int32, device="cuda")          # NaN payloads, -0.0
    y = ops.noise(x, (0.0, 0.0), [3, 4], [False, True], 0)
    assert y.data_ptr() != x.data_ptr() and torch.equal(y.view(torch.int32), xi)


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("oc", [1, 3])
@pytest.mark.parametrize("k", range(len(R.SOURCES)))
def test_noise_against_the_reference(k, oc, gray):
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd._lib import lib
    ref, bnd = R.noise_reference(k, oc, gray)
    B, C, H, W = ref.shape
    x = torch.from_numpy(R.convert(R.case_image(k), oc)).cuda()[None].repeat(B, 1, 1, 1).contiguous()
    ids = [R.NOISE_ID0 + 7 * b + k for b in range(B)]
    par = torch.tensor([ops.pack_restore_params(0, (R.SIGMA, 0.0), i, gray) for i in ids], dtype=torch.int64).cuda()
    outs = {}
    for qb in (0, 8):
        g = Guarded("f32", B * C * H, W, W)
        assert lib().srk_noise_f32(x.data_ptr(), g.ptr, par.data_ptr(), B, C, H, W, qb, _stream()) == 0
        torch.cuda.synchronize()
        g.assert_guards(f"noise image {k} bits {qb}")
        outs[qb] = g.win.view(B, C, H, W).cpu().numpy()
        assert torch.equal(ops.noise(x, (R.SIGMA, 0.0), ids, gray, qb).cpu(), torch.from_numpy(outs[qb]))
    err = np.abs(outs[0].astype(np.float64) - ref)
    print(f"noise image {k} oc {oc} gray {gray}: max |err| / bound = {(err / bnd).max():.3f}, max |err| = {err.max():.3e}")
    assert (err <= bnd).all()
    got = outs[8]
    lv = np.rint(got.astype(np.float64) * 255.0)
    assert np.array_equal(got, (lv.astype(np.float32) / np.float32(255)).astype(np.float32)), "values that are not k / 255.0f"
    level, near = D.quant8(ref)[1], D.near_half(ref, bnd)
    print(f"  quantised: {int((lv != level).sum())} levels differ from the reference, {int(near.sum())} pixels undecided")
    wrong = (lv != level) & ~(near & (np.abs(lv - level) <= 1))
    assert not wrong.any(), f"{int(wrong.sum())} decided levels differ from the reference"


def test_refusals(pool):
    from tpu_superresolution_amd._lib import lib
    pool_t, meta = pool
    P, B = 20, 2
    desc = torch.tensor(_desc(meta, 0, [(0, 0), (3, 5)], [50, 0], 0.0, [0, 1], [False, False]), dtype=torch.int64).cuda()
    gc, gd = Guarded("f32", B * 3 * P, P, P), Guarded("f32", B * 3 * P, P, P)
    ok = dict(pool_t=pool_t, desc=desc, clean=gc.ptr, degraded=gd.ptr, B=B, P=P, oc=3, sub=0, qb=0)
    for bad, code in ((dict(pool_t=None), E_NULL), (dict(desc=None), E_NULL), (dict(clean=None), E_NULL), (dict(degraded=None), E_NULL),
                      (dict(B=0), E_SHAPE), (dict(B=65536), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(P=0), E_SHAPE), (dict(P=2049), E_SHAPE),
                      (dict(oc=2), E_SHAPE), (dict(oc=0), E_SHAPE), (dict(oc=4), E_SHAPE), (dict(sub=2), E_SHAPE), (dict(sub=-1), E_SHAPE),
                      (dict(qb=4), E_SHAPE), (dict(qb=16), E_SHAPE), (dict(degraded=gc.ptr), E_SHAPE), (dict(degraded=gc.ptr + 4), E_SHAPE)):
        assert _raw(**{**ok, **bad}) == code, bad
    x = torch.zeros(2, 3, 16, 16, device="cuda")
    gn = Guarded("f32", 2 * 3 * 16, 16, 16)
    par = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    nok = dict(x=x, out=gn.ptr, par=par, B=2, C=3, H=16, W=16, qb=0)

    def noise_raw(x, out, par, B, C, H, W, qb):
        return lib().srk_noise_f32(_ptr(x), _ptr(out), _ptr(par), B, C, H, W, qb, _stream())

    for bad, code in ((dict(x=None), E_NULL), (dict(out=None), E_NULL), (dict(par=None), E_NULL), (dict(B=0), E_SHAPE), (dict(H=0), E_SHAPE),
                      (dict(W=-1), E_SHAPE), (dict(C=2), E_SHAPE), (dict(C=0), E_SHAPE), (dict(C=4), E_SHAPE), (dict(qb=1), E_SHAPE),
                      (dict(out=x), E_SHAPE), (dict(out=x.data_ptr() + 4 * 16 * 16), E_SHAPE),
                      (dict(B=1 << 20, H=1 << 30, W=1 << 30), E_SHAPE), (dict(B=1 << 30, C=3, H=17, W=33), E_SHAPE),
                      (dict(B=1 << 20, C=1, H=1 << 15, W=1 << 15), E_SHAPE)):
        assert noise_raw(**{**nok, **bad}) == code, bad
    torch.cuda.synchronize()
    for g in (gc, gd, gn):
        g.assert_untouched("the output of a refused call")
    assert _raw(**ok) == 0 and noise_raw(**nok) == 0
    torch.cuda.synchronize()
