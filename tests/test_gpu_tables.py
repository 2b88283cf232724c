"""Blur and sinc tables built on the device: srk_kernel_tables_f32 (csrc/tables.hip) called directly, and what is built on
it -- ops.kernel_tables / DeviceTables in ops.filter2d, ops.blur2d, ops.degrade_second_order, and the tables="device" pools.

Parity is against the HOST tables (blur_kernels), per tap |dev - host| <= spacing32(host) + [sinc] 2^-36 max|host| -- tests/tables_ref.py
derives it; nothing here is tuned.  The number of taps that differ in any bit is printed, not asserted.  The output sits between
guard rows of a NaN pattern, desc and bank between NaN rows: a read outside them would show as a NaN table, a write as a changed guard."""
import math
import random

import numpy as np
import pytest
import torch

import tables_ref as TR
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL = -1, -2
PI = math.pi


def _bk():
    from tpu_superresolution_amd import blur_kernels as bk
    return bk


def _lib():
    from tpu_superresolution_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _between_nans(arr, dtype):
    """arr [n][m] on the device with 64 rows of NaN before and after it -> (the whole tensor, the view of the data)."""
    a = np.asarray(arr)
    n, m = a.shape
    whole = torch.full(((n + 128) * m,), float("nan"), dtype=dtype, device="cuda")
    view = whole[64 * m:(64 + n) * m].view(n, m)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))
    return whole, view


def _launch(rows, ks, bank=None, bank_args=None):
    """srk_kernel_tables_f32 on raw descriptor rows (fp64 [n][8], any bits) -> fp32 numpy [n][ks][ks]; guards checked."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    n = rows.shape[0]
    keep_d, desc = _between_nans(rows, torch.float64)
    desc.view(torch.int64).copy_(torch.from_numpy(rows.view(np.int64)).cuda())          # the bits, NaN payloads included
    bptr, n_bank, kb, keep_b = None, 0, 0, None
    if bank is not None:
        b = np.asarray(bank, dtype=np.float32)
        n_bank, kb = b.shape[0], b.shape[1]
        keep_b, bv = _between_nans(b.reshape(n_bank, kb * kb), torch.float32)
        bv.view(torch.int32).copy_(torch.from_numpy(b.reshape(n_bank, kb * kb).view(np.int32)).cuda())
        bptr = bv.data_ptr()
    if bank_args is not None:
        bptr, n_bank, kb = bank_args
    out = Guarded("f32", n, ks * ks, ks * ks)
    rc = _lib().srk_kernel_tables_f32(desc.data_ptr(), bptr, n_bank, kb, out.ptr, n, ks, _stream())
    assert rc == 0, (rc, _lib().srk_last_error())
    torch.cuda.synchronize()
    out.assert_guards(f"kernel_tables n={n} ks={ks}")
    return out.data().numpy().reshape(n, ks, ks)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _bank(kb):
    bk = _bk()
    b = np.stack([bk.gaussian(kb, 0.9, 1.7, 0.4), bk.plateau(kb, 1.1, 0.6, -0.8, 1.5), bk.delta(kb)])
    b[2, 0, 0], b[2, -1, -1] = -0.0, 1e-40          # a -0 and a denormal: a copy keeps the words
    return b


def _descs(own):
    """Every kind at one own size: sigmas 0.2 (denormal taps) and 3, beta 0.5 and 4, cutoff pi / 5 and exactly pi.  An isotropic
    sigma of 0.2 leaves only the four taps at x^2 + y^2 = 8 in the fp32 denormal range (the next ring underflows to 0); sigma 0.9 puts
    the whole ring 142 <= x^2 + y^2 <= 167 of a 21 x 21 table there, so two tables at 0.9 carry the bulk of the denormals."""
    TD = _bk().TableDesc
    ds = [TD.delta(own), TD.gaussian(own, 0.2, 0.2), TD.gaussian(own, 3.0, 3.0), TD.gaussian(own, 3.0, 0.2, 0.6), TD.gaussian(own, 0.2, 3.0, -1.2),
          TD.generalized(own, 3.0, 0.2, 0.3, 0.5), TD.generalized(own, 0.2, 3.0, -0.7, 4.0), TD.generalized(own, 3.0, 3.0, 0.0, 4.0),
          TD.plateau(own, 0.2, 0.2, 0.0, 0.5), TD.plateau(own, 3.0, 0.2, 1.1, 4.0), TD.plateau(own, 3.0, 3.0, -0.4, 0.5),
          TD.sinc(PI / 5, own), TD.sinc(PI, own), TD.sinc(1.9, own), TD.bank(0, own), TD.bank(2, own),
          TD.gaussian(own, 0.9, 0.9), TD.gaussian(own, 0.9, 0.2, 0.6)]
    return ds


def _check_parity(dev, descs, ks, bank, what):
    """-> (taps that differ in any bit, taps)"""
    bk = _bk()
    differ = taps = 0
    for i, d in enumerate(descs):
        host = bk.pad_to(d.table(bank), ks)
        ok, n = TR.within(dev[i], host, d.kind)
        err = np.abs(dev[i].astype(np.float64) - host.astype(np.float64))
        assert ok, f"{what}: table {i} {d} leaves the bound: max |dev - host| = {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}, " \
                   f"bound there {TR.bound(host, d.kind).flat[err.argmax()]:.3e}"
        differ, taps = differ + n, taps + host.size
    return differ, taps


@pytest.mark.parametrize("own", [1, 3, 7, 13, 21])
def test_parity_with_the_host_tables_every_kind(own):
    descs, bank = _descs(own), _bank(own)
    rows = [d.row() for d in descs]
    for ks in sorted({own, 21}):
        dev = _launch(rows, ks, bank)
        differ, taps = _check_parity(dev, descs, ks, bank, f"own={own} ks={ks}")
        print(f"own={own} ks={ks}: {differ} of {taps} taps differ from the host tables in any bit")
        r = (ks - own) // 2
        frame = np.ones((ks, ks), dtype=bool)
        frame[r:r + own, r:r + own] = False
        assert not dev.view(np.uint32)[:, frame].any(), "the padding is not all +0 words"
    if own == 21:
        hosts = [d.table(bank) for d in descs if d.kind in (1, 2, 3)]
        assert sum(int(((h != 0) & (np.abs(h) < 2.0 ** -126)).sum()) for h in hosts) >= 56, "the denormal cases hold too few denormals"


def _mixed(n, seed):
    TD, rng = _bk().TableDesc, random.Random(seed)
    out = []
    for i in range(n):
        own = rng.choice([1, 3, 5, 7, 9, 13, 17, 21])
        s1, s2, th, beta = rng.uniform(0.2, 3.0), rng.uniform(0.2, 3.0), rng.uniform(-PI / 2, PI / 2), rng.uniform(0.5, 4.0)
        out.append([TD.delta(own), TD.gaussian(own, s1, s2, th), TD.generalized(own, s1, s2, th, beta), TD.plateau(own, s1, s2, th, beta),
                    TD.sinc(rng.uniform(PI / 5, PI), own), TD.bank(rng.randrange(3), 5)][i % 6])
    return out


@pytest.mark.parametrize("n", [1, 37])
def test_parity_mixed_kinds_and_sizes(n):
    descs, bank = _mixed(n, 40 + n), _bank(5)
    if n == 1:
        descs = [_bk().TableDesc.sinc(2.4, 13)]
    ks = max(21 if n > 1 else 0, max(d.ks for d in descs))
    dev = _launch([d.row() for d in descs], ks, bank)
    differ, taps = _check_parity(dev, descs, ks, bank, f"n={n}")
    print(f"n={n} ks={ks}: {differ} of {taps} taps differ from the host tables in any bit")


def test_exact_statements():
    bk = _bk()
    TD = bk.TableDesc
    bank = _bank(7)
    # delta: bitwise blur_kernels.delta, padded; bank: the words, -0 and the denormal included
    dev = _launch([TD.delta(1).row(), TD.delta(9).row(), TD.bank(2, 7).row(), TD.bank(1, 7).row()], 13, bank)
    assert _same(dev[0], bk.pad_to(bk.delta(1), 13)) and _same(dev[1], bk.pad_to(bk.delta(9), 13))
    assert _same(dev[2], np.pad(bank[2], 3)) and _same(dev[3], np.pad(bank[1], 3))
    assert np.signbit(dev[2][3, 3]) and dev[2][3, 3] == 0 and dev[2][9, 9] == np.float32(1e-40) != 0
    # symmetry: a quadratic form is even, K[a][b] == K[ks-1-a][ks-1-b]; an isotropic sinc is 8-fold symmetric; bit for bit
    sym = [TD.gaussian(13, 2.0, 0.7, 0.5), TD.generalized(21, 0.6, 2.5, -1.0, 0.7), TD.plateau(9, 1.0, 3.0, 0.2, 2.0), TD.sinc(PI / 5, 21),
           TD.sinc(PI, 21), TD.sinc(2.0, 13), TD.gaussian(21, 0.2, 0.2)]
    dev = _launch([d.row() for d in sym], 21)
    for k, d in zip(dev, sym):
        assert _same(k, k[::-1, ::-1]), d
        if d.kind == 4 or d.s1 == d.s2:
            assert _same(k, k.T) and _same(k, k[::-1]) and _same(k, k[:, ::-1]) and _same(k, k.T[::-1]), d
    # the same descriptor at different positions of a batch gives equal words
    rep = [TD.sinc(2.0, 13), TD.gaussian(7, 1.0, 2.0, 0.3), TD.delta(3), TD.sinc(2.0, 13), TD.plateau(5, 1, 2, 0.1, 1.5), TD.gaussian(7, 1.0, 2.0, 0.3),
           TD.sinc(2.0, 13)]
    dev = _launch([d.row() for d in rep], 15)
    assert _same(dev[0], dev[3]) and _same(dev[0], dev[6]) and _same(dev[1], dev[5])
    assert _same(dev[0], _launch([TD.sinc(2.0, 13).row()], 15)[0])


def test_garbage_descriptors_stay_inside():
    """Containment: for any descriptor bits the kernel stays inside desc, bank and tab (include/srk.h) -- the clamps are exercised, the
    run ends normally, the guards keep their bits."""
    bk = _bk()
    rng = np.random.RandomState(5)
    bank = _bank(5)
    garbage = rng.randint(0, 2 ** 63 - 1, size=(24, 8), dtype=np.int64) * rng.choice([-1, 1], size=(24, 8))
    _launch(garbage.view(np.float64), 21, bank)
    _launch(garbage.view(np.float64), 5, bank)
    nan, inf = float("nan"), float("inf")
    g = bk.TableDesc.gaussian(7, 1.0, 2.0, 0.3).row()
    rows = [(nan,) * 8, (1.0, 23.0) + g[2:], (1.0, -1.0) + g[2:], (1.0, 1e300) + g[2:], (1.0, nan) + g[2:], (1.0, 6.0) + g[2:], (1.0, 7.5) + g[2:],
            (5.0, 5.0, 0, 0, 0, 1.0, 0.0, -5.0), (5.0, 5.0, 0, 0, 0, 1.0, 0.0, 1e300), (5.0, 5.0, 0, 0, 0, 1.0, 0.0, nan), (5.0, 99.0, 0, 0, 0, 1.0, 0.0, 2.0),
            (6.0, 7.0) + g[2:], (-1.0, 7.0) + g[2:], (inf, 7.0) + g[2:], (1.0, 7.0, nan, 0.0, 1.0, 1.0, 0.0, 0.0), (4.0, 7.0, 0, 0, 0, 1.0, nan, 0.0),
            (4.0, 7.0, 0, 0, 0, 1.0, 1e300, 0.0), (2.0, 7.0, 1.0, 0.0, 1.0, -inf, 0.0, 0.0), (3.0, 21.0, -1.0, 0.0, -1.0, 0.5, 0.0, 0.0)]
    dev = _launch(rows, 9, bank)
    d9 = bk.pad_to(bk.delta(1), 9)
    assert _same(dev[0], d9)                                                     # kind NaN: a delta of side 1 (ks_own NaN)
    want7 = bk.pad_to(bk.gaussian(7, 1.0, 2.0, 0.3), 9)
    assert TR.within(dev[1], bk.gaussian(9, 1.0, 2.0, 0.3), 1)[0]                # ks_own 23 -> 9
    assert TR.within(dev[2], d9, 1)[0] and TR.within(dev[4], d9, 1)[0]           # ks_own -1 / NaN -> 1: the one tap, normalised
    assert TR.within(dev[3], bk.gaussian(9, 1.0, 2.0, 0.3), 1)[0]                # ks_own 1e300 -> 9
    assert TR.within(dev[5], bk.pad_to(bk.gaussian(5, 1.0, 2.0, 0.3), 9), 1)[0]  # even 6 -> 5
    assert TR.within(dev[6], want7, 1)[0]                                        # 7.5 -> 7
    assert _same(dev[7], np.pad(bank[0], 2)) and _same(dev[8], np.pad(bank[2], 2)) and _same(dev[9], np.pad(bank[0], 2))          # bank_index clamped
    assert _same(dev[10], np.pad(bank[2], 2))                                    # kind 5 takes the bank's side, whatever ks_own says
    for i in (11, 12, 13):
        assert _same(dev[i], bk.pad_to(bk.delta(7), 9))                          # kind outside 0..5: delta
    for i in (14, 15):
        inner = dev[i][1:8, 1:8]
        assert np.isnan(inner).all() and not dev[i].view(np.uint32)[0].any()     # a NaN parameter: a NaN table inside +0 padding
    # kind 5 with a null bank is a delta; a bank too small for the index never is read past
    dev = _launch([(5.0, 5.0, 0, 0, 0, 1.0, 0.0, 1.0), (5.0, nan, nan, nan, nan, nan, nan, nan)], 7)
    assert _same(dev[0], bk.pad_to(bk.delta(5), 7)) and _same(dev[1], bk.pad_to(bk.delta(1), 7))


def test_refusals():
    from tpu_superresolution_amd import ops
    bk, L = _bk(), _lib()
    TD = bk.TableDesc
    P = 4096                                                     # a non-null address; never read or written: every call is refused
    for args, code in (((None, None, 0, 0, P, 1, 7), E_NULL), ((P, None, 0, 0, None, 1, 7), E_NULL), ((P, None, 0, 0, P * 64, 0, 7), E_SHAPE),
                       ((P, None, 0, 0, P * 64, -3, 7), E_SHAPE), ((P, None, 0, 0, P * 64, 1, 8), E_SHAPE), ((P, None, 0, 0, P * 64, 1, 23), E_SHAPE),
                       ((P, None, 0, 0, P * 64, 1, 0), E_SHAPE), ((P, None, 0, 0, P * 64, 1, -7), E_SHAPE), ((P, None, 1, 5, P * 64, 1, 7), E_SHAPE),
                       ((P, None, 0, 5, P * 64, 1, 7), E_SHAPE), ((P, P * 32, 0, 5, P * 64, 1, 7), E_SHAPE), ((P, P * 32, 2, 4, P * 64, 1, 7), E_SHAPE),
                       ((P, P * 32, 2, 9, P * 64, 1, 7), E_SHAPE), ((P, P * 32, 2, 0, P * 64, 1, 7), E_SHAPE), ((P, P * 32, -1, 5, P * 64, 1, 7), E_SHAPE),
                       ((P, None, 0, 0, P + 8, 1, 7), E_SHAPE), ((P, P * 64 + 4, 1, 3, P * 64, 1, 7), E_SHAPE)):          # the last two: overlaps
        rc = L.srk_kernel_tables_f32(*args, None)
        assert rc == code, (args, rc, L.srk_last_error())
        assert L.srk_last_error(), "no message"
    for bad in (lambda: ops.kernel_tables([TD.gaussian(7, 1, 1)], ks=8), lambda: ops.kernel_tables([TD.gaussian(7, 1, 1)], ks=5),
                lambda: ops.kernel_tables([TD.gaussian(7, 1, 1), TD.delta(9)], ks=7), lambda: ops.kernel_tables([TD(1, 7, 0.0, 1.0)]),
                lambda: ops.kernel_tables([TD(1, 7, 1.0, -2.0)]), lambda: ops.kernel_tables([TD(4, 7, cutoff=3.2)]),
                lambda: ops.kernel_tables([TD(4, 7, cutoff=0.0)]), lambda: ops.kernel_tables([TD.sinc(1.0, 7)], signed=False),
                lambda: ops.kernel_tables([TD.gaussian(7, 1, 1), TD.sinc(1.0, 7)], signed=False), lambda: ops.kernel_tables([]),
                lambda: ops.kernel_tables([bk.gaussian(7, 1, 1)]), lambda: ops.kernel_tables([TD.bank(0, 5)]),
                lambda: ops.kernel_tables([TD.bank(3, 5)], bank=_bank(5)), lambda: ops.kernel_tables([TD.bank(0, 7)], bank=_bank(5)),
                lambda: ops.kernel_tables([TD(2, 7, 1.0, 1.0, 0.0, 0.0)]), lambda: ops.kernel_tables([TD(9, 7)])):
        with pytest.raises(ValueError):
            bad()
    x = torch.rand(2, 3, 24, 40, device="cuda")
    signed = ops.kernel_tables([TD.sinc(1.0, 7), TD.delta()])
    with pytest.raises(ValueError, match="sinc"):
        ops.blur2d(x, signed)
    with pytest.raises(ValueError):
        ops.filter2d(x, ops.kernel_tables([TD.delta()]))                       # one table for two samples
    with pytest.raises(ValueError, match="does not exceed"):
        ops.filter2d(x[:, :, :6], ops.kernel_tables([TD.sinc(1.0, 13), TD.delta()]))
    g, d = bk.gaussian(5, 1, 1), TD.gaussian(5, 1, 1)
    mixed = [ops.SecondOrder(g, 1.0, (0.0, 0.0), False, 50, d, 1.0, (0.0, 0.0), False, 50, False, d, 1),
             ops.SecondOrder(d, 1.0, (0.0, 0.0), False, 50, d, 1.0, (0.0, 0.0), False, 50, False, d, 2)]
    with pytest.raises(ValueError, match="mixes"):
        ops.degrade_second_order(torch.rand(2, 3, 48, 48, device="cuda"), 2, mixed)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_filter2d_and_blur2d_take_device_tables_bitwise():
    from tpu_superresolution_amd import ops
    bk = _bk()
    TD = bk.TableDesc
    x = torch.from_numpy(np.random.RandomState(2).rand(2, 3, 24, 40).astype(np.float32)).cuda()
    t = ops.kernel_tables([TD.sinc(2.0, 13), TD.gaussian(7, 1.5, 0.6, 0.4)])
    assert t.ks == 13 and t.own == (13, 7) and t.signed and tuple(t.tab.shape) == (2, 13, 13)
    assert torch.equal(ops.filter2d(x, t), ops.filter2d(x, t.tab.cpu().numpy()))
    assert torch.equal(ops.filter2d(x, t, quant_bits=8), ops.filter2d(x, t.tab.cpu().numpy(), quant_bits=8))
    ext = [(24, 33), (9, 40)]
    got, want = ops.filter2d(x, t, ext), ops.filter2d(x, t.tab.cpu().numpy(), ext)
    for b, (h, w) in enumerate(ext):
        assert torch.equal(got[b, :, :h, :w], want[b, :, :h, :w])
    u = ops.kernel_tables([TD.plateau(9, 1.0, 2.0, 0.5, 1.5), TD.generalized(5, 0.8, 0.8, 0.0, 0.7)], ks=11, signed=False)
    assert u.ks == 11 and u.own == (9, 5) and not u.signed
    assert torch.equal(ops.blur2d(x, u), ops.blur2d(x, u.tab.cpu().numpy()))
    lr, hr = ops.degrade_psf(x, 2, u, noise=(0.01, 0.0))
    lr2, _ = ops.degrade_psf(x, 2, u.tab.cpu().numpy(), noise=(0.01, 0.0))
    assert torch.equal(lr, lr2)
    # a bank on the device, uploaded once, and as an array
    bank = _bank(5)
    bt = torch.from_numpy(bank).cuda()
    v = ops.kernel_tables([TD.bank(1, 5), TD.bank(0, 5)], bank=bt, signed=False)
    assert _same(v.tab.cpu().numpy(), bank[[1, 0]]) and _same(ops.kernel_tables([TD.bank(1, 5), TD.bank(0, 5)], bank=bank[:2]).tab.cpu().numpy(), bank[[1, 0]])


def test_second_order_chain_takes_descriptors_bitwise():
    from tpu_superresolution_amd import ops
    bk = _bk()
    TD = bk.TableDesc
    ps = [ops.SecondOrder(TD.gaussian(9, 1.2, 0.7, 0.3), 1.3, (0.02, 0.0), False, 60, TD.sinc(1.8, 7), 0.9, (0.03, 0.01), True, 45, False, TD.sinc(2.2, 13), 11),
          ops.SecondOrder(TD.sinc(1.5, 11), 0.4, (0.01, 0.02), True, 90, TD.delta(), 1.2, (0.05, 0.0), False, 30, True, TD.delta(), 12)]
    x = torch.from_numpy(np.random.RandomState(61).rand(2, 3, 48, 48).astype(np.float32)).cuda()
    got = ops.degrade_second_order(x, 2, ps)
    back = []
    for p in ps:          # the tables the device built, read back, through the array path
        ks = {k: ops.kernel_tables([getattr(p, k)]).tab[0].cpu().numpy() for k in ("k1", "k2", "k3")}
        back.append(p._replace(**ks))
    assert got.shape == (2, 3, 24, 24) and torch.equal(got, ops.degrade_second_order(x, 2, back))


P_, S_, M_ = 16, 2, 8


def _images():
    rng = np.random.RandomState(71)
    return [rng.randint(0, 256, size=(96, 96, 3), dtype=np.uint8), rng.randint(0, 256, size=(96, 96, 3), dtype=np.uint8)]


def _level_report(a, b, what):
    d = (a - b).abs().mul(255.0)
    n = int((d > 0).sum())
    print(f"{what}: {n} of {d.numel()} LR pixels differ, max {float(d.max()):.3f} 8-bit levels")
    return float(d.max())


def test_hr2_pool_with_device_tables_matches_the_host_pool():
    """Equal seeds: bitwise equal HR patches, LR patches within one 8-bit level (the tables agree to an fp32 spacing; the only
    amplifier is the chain's quantisations)."""
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHR2Pool, PsfSpec, SecondOrderSpec
    idx = [0, 1, 1, 0]
    worst = 0.0
    for psf in (None, PsfSpec(mode="mixed", seed=4)):
        pools = [DeviceHR2Pool(_images(), P_, S_, SecondOrderSpec(seed=4, sinc_p=0.5), DegradeSpec(seed=4), margin=M_, psf=psf, augment="d4", tables=t)
                 for t in ("host", "device")]
        for step in range(3):
            res = []
            for pool in pools:
                random.seed(200 + step)
                res.append(pool.sample(idx))
            (lr_h, hr_h), (lr_d, hr_d) = res
            assert torch.equal(hr_h, hr_d)
            worst = max(worst, _level_report(lr_h, lr_d, f"HR2 pool psf={'mixed' if psf else 'none'} step {step}"))
    assert worst <= 1.0 + 1e-3


def test_hr_pool_with_device_tables_matches_the_host_pool(tmp_path):
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool, PsfSpec
    bk = _bk()
    f = tmp_path / "psf.npy"
    np.save(f, np.stack([bk.gaussian(7, 1.0, 2.0, 0.3), bk.plateau(7, 1.2, 0.7, 1.0, 1.5)]))
    idx = [0, 1, 1, 0, 0]
    for psf in (PsfSpec(mode="rotated", seed=6), PsfSpec(mode="mixed", seed=6), PsfSpec(mode="file", file=str(f), seed=6)):
        pools = [DeviceHRPool(_images(), P_, S_, degrade=DegradeSpec(seed=6), psf=psf, tables=t) for t in ("host", "device")]
        for step in range(2):
            res = []
            for pool in pools:
                random.seed(300 + step)
                res.append(pool.sample(idx))
            (lr_h, hr_h), (lr_d, hr_d) = res
            assert torch.equal(hr_h, hr_d)
            worst = _level_report(lr_h, lr_d, f"HR pool psf={psf.mode} step {step}")
            assert worst <= 1.0 + 1e-3
            if psf.mode == "file":
                assert torch.equal(lr_h, lr_d)          # a bank is copied: the same words, the same patches
    with pytest.raises(ValueError, match="tables"):
        DeviceHRPool(_images(), P_, S_, tables="gpu")
