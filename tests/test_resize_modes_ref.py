"""tests/resize_modes_ref.py pinned: bilinear against F.interpolate(size=, mode='bilinear', align_corners=False) and area against
F.adaptive_avg_pool2d, both in fp64, and negative controls -- what srk_resize_ragged_mode_f32 must NOT compute.  Also the
undecided-level cap of the quantised GPU cases, from the reference alone.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import filter2d_ref as Fr
import resize_modes_ref as Mr

SIZES = [((40, 72), (60, 108)), ((40, 72), (20, 36)), ((33, 50), (50, 75)), ((33, 50), (11, 17)), ((12, 11), (24, 22)), ((12, 11), (4, 5)),
         ((23, 64), (23, 96)), ((23, 64), (12, 8)), ((40, 72), (29, 47)), ((33, 50), (40, 41)), ((12, 11), (7, 13)), ((23, 64), (31, 50)),
         ((12, 11), (12, 11)), ((64, 9), (8, 72))]
TARGETS = {"up": [(60, 108), (50, 75), (24, 22), (23, 96)], "down": [(20, 36), (11, 17), (4, 5), (12, 8)], "identity": list(Fr.RAGGED_EXT),
           "noninteger": [(29, 47), (40, 41), (7, 13), (31, 50)]}


def _x(shape, seed=0):
    return np.random.RandomState(seed).rand(2, *shape).astype(np.float32)


def _tol(x):
    # the reference rounds its weights to fp32 as the kernel does; torch does not: at most two weights per axis off by u each
    return 8.0 * Mr.U * np.abs(x).max()


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_bilinear_is_interpolate(size):
    (h, w), (ho, wo) = size
    x = _x((h, w))
    want = F.interpolate(torch.from_numpy(x.astype(np.float64))[None], size=(ho, wo), mode="bilinear", align_corners=False)[0].numpy()
    assert np.max(np.abs(Mr.resize(x, ho, wo, Mr.BILINEAR) - want)) <= _tol(x)


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_area_is_adaptive_avg_pool(size):
    (h, w), (ho, wo) = size
    x = _x((h, w), 1)
    want = F.adaptive_avg_pool2d(torch.from_numpy(x.astype(np.float64))[None], (ho, wo))[0].numpy()
    assert np.max(np.abs(Mr.resize(x, ho, wo, Mr.AREA) - want)) <= _tol(x)
    lo, hi, ws = Mr.tables(Mr.AREA, h, ho)
    assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all() and max(len(v) for v in ws) <= 33


def test_mode_0_is_the_cubic_reference():
    import resize_ref as Rr
    x = _x((33, 50), 2)
    assert np.max(np.abs(Mr.resize(x, 11, 17, 0) - Rr.resize(x, 11, 17))) <= Rr.bound(33, 50, 11, 17, 1.0)


@pytest.mark.parametrize("mode,control", [(Mr.BILINEAR, dict(align_corners=True)), (Mr.BILINEAR, dict(antialias=True)), (Mr.AREA, dict(rounded_area=True)),
                                          (Mr.BILINEAR, dict(vertical_first=True)), (Mr.AREA, dict(vertical_first=True))],
                         ids=lambda v: str(v))
def test_negative_controls_differ(mode, control):
    x = _x((33, 50), 3)
    ho, wo = (13, 19)          # not an integer factor: at 3x the bilinear weights are (1, 0) and nothing rounds
    right, bnd = Mr.resize(x, ho, wo, mode), Mr.bound(x, ho, wo, mode)
    wrong = Mr.resize(x, ho, wo, mode, **control)
    if "vertical_first" in control:
        # the two orders agree in exact arithmetic (the fp64 results differ by rounding alone): the order shows in the kernel's own fp32
        # chains, where it changes bits -- which is what the bit-exact "sample alone" and "mode 0" device cases hold still
        assert np.max(np.abs(wrong - right)) <= 1e-14
        a, b = Mr.resize_f32(x, ho, wo, mode), Mr.resize_f32(x, ho, wo, mode, vertical_first=True)
        assert (a != b).mean() > 0.05 and (np.abs(a - right) <= bnd).all() and (np.abs(b - right) <= bnd).all()
        return
    assert (np.abs(wrong - right) > bnd).mean() > 0.05, f"the control {control} lies inside the bound"


def test_limits_rs_filter_relies_on():
    for n_in, n_out in ((72, 9), (64, 8), (71, 9), (40, 5), (9, 72), (50, 50)):
        for mode in (Mr.BILINEAR, Mr.AREA):
            lo, hi, ws = Mr.tables(mode, n_in, n_out)
            assert max(len(w) for w in ws) <= (2 if mode == Mr.BILINEAR else 9)
            assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all() and lo.min() >= 0 and hi.max() <= n_in
            assert all(abs(w.sum() - 1.0) < 1e-6 for w in ws)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("case", list(TARGETS))
def test_undecided_cap_of_the_quantised_gpu_cases(case, C):
    """At most 1 % of the levels of every quantised sample of tests/test_gpu_resize_modes.py are undecided: from the reference alone."""
    _, samples = Fr.ragged_batch(31 + C, C, lo=0.0, hi=1.0)
    for modes in ([0, 1, 2, 1], [2, 2, 0, 1]):
        for b, s in enumerate(samples):
            if modes[b] == 0:
                continue
            ho, wo = TARGETS[case][b]
            und = Fr.near_half(Mr.resize(s, ho, wo, modes[b]), Mr.bound(s, ho, wo, modes[b]))
            assert und.mean() <= 0.01, f"{case} sample {b} mode {modes[b]}: {und.mean():.3%} undecided"
