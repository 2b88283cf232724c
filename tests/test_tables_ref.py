"""Descriptors beside tables (blur_kernels.TableDesc; PsfSpec.draw / SecondOrderSpec.draw / stage1_table with as_desc=True) and the
restatement of tests/tables_ref.py: what the host hands the device describes exactly the tables the host would have built, and the
bound that tests/test_gpu_tables.py holds the kernel to catches the mistakes a kernel could make.  No GPU."""
import math
import random

import numpy as np
import pytest

import tables_ref as TR
from tpu_superresolution_amd import blur_kernels as bk

TD = bk.TableDesc


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == np.float32 == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _bank():
    b = np.stack([bk.gaussian(5, 0.9, 1.7, 0.4), bk.plateau(5, 1.1, 0.6, -0.8, 1.5), bk.delta(5)])
    b[2, 0, 0], b[2, 4, 4] = -0.0, 1e-40          # words a copy must keep
    return b


def test_table_is_the_blur_kernels_function_for_each_kind():
    bank = _bank()
    cases = [(TD.delta(), bk.delta()), (TD.delta(7), bk.delta(7)),
             (TD.gaussian(13, 1.3, 0.4, 0.7), bk.gaussian(13, 1.3, 0.4, 0.7)), (TD.gaussian(21, 0.2, 0.2), bk.gaussian(21, 0.2, 0.2)),
             (TD.generalized(9, 2.0, 0.9, -1.1, 0.5), bk.generalized(9, 2.0, 0.9, -1.1, 0.5)),
             (TD.plateau(15, 1.5, 2.5, 0.2, 1.7), bk.plateau(15, 1.5, 2.5, 0.2, 1.7)),
             (TD.sinc(math.pi / 3, 7), bk.sinc(math.pi / 3, 7)), (TD.sinc(math.pi, 21), bk.sinc(math.pi, 21))]
    for d, t in cases:
        assert _same(d.table(), t), d
    for i in range(3):
        assert _same(TD.bank(i, 5).table(bank), bank[i])
    assert [d.kind for d, _ in cases] == [0, 0, 1, 1, 2, 3, 4, 4] and TD.bank(1, 5).kind == 5


def test_row_carries_the_coefficients_of_quad_bitwise():
    rng = random.Random(3)
    for _ in range(100):
        ks = rng.choice([1, 3, 7, 13, 21])
        s1, s2, th, beta = rng.uniform(1e-3, 4), rng.uniform(1e-3, 4), rng.uniform(-2, 2), rng.uniform(0.5, 4)
        for d in (TD.gaussian(ks, s1, s2, th), TD.generalized(ks, s1, s2, th, beta), TD.plateau(ks, s1, s2, th, beta)):
            row = d.row()
            assert len(row) == 8 and all(type(v) is float for v in row) and row[:2] == (float(d.kind), float(ks))
            c, s = math.cos(th), math.sin(th)
            i1, i2 = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
            assert row[2:5] == (c * c * i1 + s * s * i2, 2.0 * c * s * (i1 - i2), s * s * i1 + c * c * i2)
            assert row[2:5] == bk._quad_coef(s1, s2, th) and row[5] == (1.0 if d.kind == 1 else beta)
            # the quadratic form the device rebuilds from the row IS _quad's, bit for bit
            xx, xy, yy = bk._grid(ks)
            assert np.array_equal((row[2] * xx + row[3] * xy) + row[4] * yy, bk._quad(ks, s1, s2, th))
    assert TD.sinc(1.25, 9).row() == (4.0, 9.0, 0.0, 0.0, 0.0, 1.0, 1.25, 0.0)
    assert TD.delta(3).row() == (0.0, 3.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0) and TD.bank(2, 5).row() == (5.0, 5.0, 0.0, 0.0, 0.0, 1.0, 0.0, 2.0)


def test_constructors_refuse_what_the_functions_refuse_with_their_errors():
    pairs = [(lambda: TD.gaussian(8, 1, 1), lambda: bk.gaussian(8, 1, 1)), (lambda: TD.gaussian(23, 1, 1), lambda: bk.gaussian(23, 1, 1)),
             (lambda: TD.gaussian(7, 0.0, 1), lambda: bk.gaussian(7, 0.0, 1)), (lambda: TD.gaussian(7, 1, -1), lambda: bk.gaussian(7, 1, -1)),
             (lambda: TD.gaussian(7, 1, 1, math.inf), lambda: bk.gaussian(7, 1, 1, math.inf)),
             (lambda: TD.generalized(7, 1, 1, 0, 0.0), lambda: bk.generalized(7, 1, 1, 0, 0.0)),
             (lambda: TD.plateau(7, 1, math.nan, 0, 1.0), lambda: bk.plateau(7, 1, math.nan, 0, 1.0)),
             (lambda: TD.plateau(7, 1, 1, 0, math.inf), lambda: bk.plateau(7, 1, 1, 0, math.inf)),
             (lambda: TD.sinc(3.2, 7), lambda: bk.sinc(3.2, 7)), (lambda: TD.sinc(0.0, 7), lambda: bk.sinc(0.0, 7)),
             (lambda: TD.sinc(1.0, 4), lambda: bk.sinc(1.0, 4)), (lambda: TD.delta(2), lambda: bk.delta(2)), (lambda: TD.delta(True), lambda: bk.delta(True))]
    for mine, theirs in pairs:
        with pytest.raises(ValueError) as a:
            mine()
        with pytest.raises(ValueError) as b:
            theirs()
        assert str(a.value) == str(b.value)
    with pytest.raises(ValueError):
        TD.bank(-1, 5)
    with pytest.raises(ValueError):
        TD.bank(0, 5).table()          # no bank given
    with pytest.raises(ValueError):
        TD(7, 3).row()                 # a kind that does not exist


def _psf_file(tmp_path):
    f = tmp_path / "psf.npy"
    np.save(f, np.stack([bk.gaussian(7, 1.0, 2.0, 0.3), bk.gaussian(7, 0.8, 0.8), bk.plateau(7, 1.2, 0.7, 1.0, 1.5)]))
    return str(f)


@pytest.mark.parametrize("mode", ["rotated", "mixed", "file"])
def test_psf_draws_as_descriptors_are_the_same_draws(mode, tmp_path):
    from tpu_superresolution_amd.sr_datasets import PsfSpec
    spec = PsfSpec(mode=mode, seed=5, file=_psf_file(tmp_path) if mode == "file" else None)
    ra, rb, blur_rng = spec.rng(), spec.rng(), random.Random(1)
    kinds = set()
    for i in range(200):
        blur = (blur_rng.choice([0.0, blur_rng.uniform(0.2, 2.5)]), blur_rng.uniform(0.0, 2.5))
        t, d = spec.draw(ra, blur), spec.draw(rb, blur, as_desc=True)
        assert isinstance(d, TD) and _same(d.table(spec.tables), t), (i, d)
        kinds.add(d.kind)
    assert ra.getstate() == rb.getstate()
    assert kinds == {"rotated": {1}, "mixed": {1, 2, 3}, "file": {5}}[mode]


@pytest.mark.parametrize("sinc_p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("extent", [96, 12])          # 12: R >= an extent drops tables to the delta / to table1
def test_second_order_draws_as_descriptors_are_the_same_draws(sinc_p, extent):
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, PsfSpec, SecondOrderSpec, stage1_table
    spec, deg, psf = SecondOrderSpec(sinc_p=sinc_p, final_sinc_p=0.5, seed=2), DegradeSpec(seed=2), PsfSpec(mode="mixed", seed=2)
    ra, rb, da, pa, pb = spec.rng(), spec.rng(), deg.rng(), psf.rng(), psf.rng()
    seen = {k: set() for k in ("k1", "k2", "k3")}
    for i in range(200):
        blur, noise, nid, gray = deg.draw(da, colour=True)
        if i % 2:
            t1, d1 = psf.draw(pa, blur), psf.draw(pb, blur, as_desc=True)
        else:
            t1, d1 = stage1_table(blur), stage1_table(blur, as_desc=True)
        a = spec.draw(ra, t1, noise, nid, gray, True, extent, 2)
        b = spec.draw(rb, d1, noise, nid, gray, True, extent, 2, as_desc=True)
        for k in ("k1", "k2", "k3"):
            d = getattr(b, k)
            assert isinstance(d, TD) and _same(d.table(), getattr(a, k)), (i, k, d)
            seen[k].add(d.kind)
        assert a._replace(k1=0, k2=0, k3=0) == b._replace(k1=0, k2=0, k3=0)
    assert ra.getstate() == rb.getstate() and pa.getstate() == pb.getstate()
    assert 0 in seen["k2"] and 0 in seen["k3"]
    if extent == 96:
        assert (4 in seen["k1"]) == (sinc_p > 0) and (4 in seen["k2"]) == (sinc_p > 0) and 4 in seen["k3"] and (1 in seen["k2"]) == (sinc_p < 1)
    else:
        assert seen["k3"] <= {0, 4} and 0 in seen["k3"]


# ---- the restatement and the bound -------------------------------------------------------------------------------------------------
def _random_desc(rng):
    ks = rng.choice([3, 7, 13, 21])
    s1, s2 = (rng.choice([rng.uniform(0.2, 0.5), rng.uniform(0.5, 3.0)]) for _ in range(2))
    th, beta = rng.uniform(-math.pi / 2, math.pi / 2), rng.uniform(0.5, 4.0)
    return rng.choice([TD.gaussian(ks, s1, s2, th), TD.generalized(ks, s1, s2, th, beta), TD.plateau(ks, s1, s2, th, beta)])


def test_restatement_is_inside_the_bound_on_host_tables():
    rng = random.Random(11)
    descs = [_random_desc(rng) for _ in range(120)] + [TD.gaussian(21, 0.2, 0.2), TD.gaussian(21, 0.2, 0.31, 0.4), TD.gaussian(1, 1, 1)]
    descs += [TD.sinc(c, ks) for ks in (3, 7, 13, 21) for c in (math.pi / 5, 1.7, math.pi)]
    differ = taps = denormal = 0
    for d in descs:
        host = d.table()
        ok, n = TR.within(TR.restate(d.row(), d.ks), host, d.kind)
        assert ok, d
        differ, taps = differ + n, taps + host.size
        denormal += int(((host != 0) & (np.abs(host) < 2.0 ** -126)).sum())
    print(f"restatement vs blur_kernels: {differ} of {taps} taps differ in any bit ({denormal} fp32 denormals among them)")
    assert denormal > 100          # the denormal range is exercised


def test_restatement_pads_and_copies():
    bank = _bank()
    assert _same(TR.restate(TD.delta(3).row(), 7), bk.pad_to(bk.delta(3), 7))
    assert _same(TR.restate(TD.bank(2, 5).row(), 9, bank), np.pad(bank[2], 2)) and np.signbit(TR.restate(TD.bank(2, 5).row(), 9, bank)[2, 2])
    d = TD.gaussian(7, 1.0, 0.5, 0.3)
    ok, _ = TR.within(TR.restate(d.row(), 13), bk.pad_to(d.table(), 13), 1)
    assert ok


def test_bound_catches_each_fault():
    """Each deliberate mistake of `restate` leaves the bound on a table where it matters."""
    aniso, small, sinc = TD.gaussian(13, 2.0, 0.6, 0.5), TD.gaussian(21, 0.2, 0.2), TD.sinc(math.pi / 2, 21)

    def fails(d, ks, fault):
        return not TR.within(TR.restate(d.row(), ks, fault=fault), bk.pad_to(d.table(), ks), d.kind)[0]

    assert fails(sinc, 21, "j1_16")
    assert fails(small, 21, "ftz")
    assert fails(aniso, 13, "transpose")
    assert fails(aniso, 21, "uncentred") and fails(TD.delta(3), 5, "uncentred")
    for d, ks in ((sinc, 21), (small, 21), (aniso, 13), (aniso, 21)):
        assert not fails(d, ks, None)


def test_reciprocal_multiply_is_an_fp64_fault_that_one_fp32_spacing_admits():
    """Multiplying by 1 / S instead of dividing moves an fp64 quotient by at most one ulp; after the single fp32 rounding a tap then moves
    by at most ONE fp32 spacing, and only when the quotient sits within 2^-52 of a rounding boundary (about one tap in 2^29).  So this
    control cannot leave a bound that admits one spacing, on any table: it is measured where it shows, in the fp64 quotients -- they do
    change, which is why srk.h fixes the division -- and the fp32 words are checked to stay inside the bound.  (Recorded run: 1260 of
    6728 fp64 quotients change, 0 of the fp32 words.)"""
    rng = random.Random(4)
    changed64 = changed32 = total = 0
    for _ in range(40):
        d = _random_desc(rng)
        a, b = TR.restate(d.row(), d.ks), TR.restate(d.row(), d.ks, fault="recip")
        a64, b64 = TR.restate(d.row(), d.ks, as_f64=True), TR.restate(d.row(), d.ks, fault="recip", as_f64=True)
        changed64 += int((a64 != b64).sum())
        changed32 += int((a.view(np.uint32) != b.view(np.uint32)).sum())
        total += a.size
        assert np.array_equal(a64.astype(np.float32).view(np.uint32), a.view(np.uint32))
        assert TR.within(b, a, d.kind)[0] and float(np.abs(a64 - b64).max()) <= float(np.spacing(np.abs(a64)).max())
    print(f"1 / S multiply: {changed64} of {total} fp64 quotients change, {changed32} of the fp32 words")
    assert changed64 > total // 10
