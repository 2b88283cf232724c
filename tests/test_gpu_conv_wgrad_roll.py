"""The rolling X-row window of the 3x3 conv weight-gradient kernels (csrc/convwgrad.hip, option conv_wgrad_roll) against the per-run
staging it replaces (conv_wgrad_roll = 0) and against the fp64 restatement of tests/wgrad_ref.py.

  conv_wgrad_roll = 1 (default)  conv_wgrad_taps_dma_kernel streams image rows into an LDS row ring (W = 64 and W = 128), and
                                 smallconv_wgrad_mfma_kernel streams the rows of its 64-pixel column the same way
  conv_wgrad_roll = 0            the per-run staging: every run fetches its own 3 x 66-pixel halo; also what every other width of the
                                 180-channel kernel runs

At W = 64 the M-splits, the run order of a split and the MFMA order are the same in both, so with the split partials (a fixed-order
sum) dW must agree BIT FOR BIT; at W = 128 the splits move to whole image rows, so only the exact class (integer sums: order-free) is
compared for equality there, the random class against the derived bound plus repeatability.  db goes through fp32 atomics in both.

The operands sit in NaN-padded buffers and the outputs between NaN guard rows (the call pattern of tests/test_gpu_wgrad.py): a row
fetched from outside the tensor or a tap that selects the wrong slot shows as NaN or as a wrong integer."""
import ctypes as C

import pytest
import torch

import test_gpu_wgrad as W
import wgrad_ref as R

gpu = pytest.mark.gpu

# (B, H, W, CinP, N[, r, Cs])
ROLL64 = ((3, 5, 64, 64, 64),            # splits of one row each, every y of an image
          (2, 1, 64, 64, 64),            # H = 1: both neighbour rows are outside the image
          (2, 2, 64, 64, 64),
          (4, 64, 64, 192, 192),         # nine tiles, 28 splits of 10 rows: splits start mid-image and cross image boundaries
          (2, 4, 64, 64, 256, 2, 64))    # conv + PixelShuffle (SHUF)
ROLL128 = ((1, 5, 128, 192, 192), (2, 3, 128, 64, 256, 2, 64))
UNCOVERED = (1, 2, 256, 64, 64)          # W = 256: the row ring does not hold it
HEADS = ((64, 64, 3, 4), (60, 64, 12, 16))                     # (Cin, CinP, Co, CoP)
HEAD_GEO = ((2, 7, 128), (1, 1, 64), (3, 4, 64))


def conv(cls, s, seed=0):
    return R.conv_case(cls, *s[:5], r=s[5] if len(s) > 5 else 1, Cs=s[6] if len(s) > 5 else 0, seed=seed)


def sid(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib


@pytest.fixture(scope="module")
def workspace(L):
    assert int(L.lib().srk_wgrad_workspace_bytes()) == R.WS_FULL
    return torch.empty(R.WS_FULL, dtype=torch.uint8, device="cuda")


_cache = {}


def prepared(c):
    """(inputs, expectation, device operands) of a case: computed once, shared by the tests, never modified."""
    if c.id not in _cache:
        inp = R.make_inputs(c)
        _cache[c.id] = (inp, R.expected(c, inp), W.upload(c, inp))
    return _cache[c.id]


def run(L, workspace, c, roll, repeat=1):
    """One call (or `repeat`) under the default options of tests/wgrad_ref.py (LDS-DMA taps kernel, split partials) with the full
    workspace and conv_wgrad_roll = roll -> the outputs the reference names.  The guard rows are checked on the way."""
    inp, exp, dev = prepared(c)
    h = L.lib()
    was = W.get_option(L, "conv_wgrad_roll")
    try:
        L.check(h.srk_set_option(b"conv_wgrad_roll", roll))
        bufs = W.run(L, workspace, c, inp, dev, {}, R.WS_FULL, repeat=repeat)
    finally:
        L.check(h.srk_set_option(b"conv_wgrad_roll", was))
    for k, b in bufs.items():
        b.assert_guards(f"{c.id} roll={roll} {k}")
    return W.read(c, bufs, exp)


def check(c, got, what):
    ok, ratios = R.accepts(c, got, prepared(c)[1])
    print(f"[roll] {c.id} {what}: max(err / tol) " + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))
    assert ok, f"{c.id} {what}: max(err / tol) {ratios}"


@gpu
@pytest.mark.parametrize("s", ROLL64, ids=sid)
def test_w64_rolling_window_gives_the_bits_of_the_per_run_staging(L, workspace, s):
    c = conv("random", s, seed=60)
    new, old = run(L, workspace, c, 1), run(L, workspace, c, 0)
    assert torch.equal(W.bits(new["dw"]), W.bits(old["dw"])), f"{c.id}: {int((W.bits(new['dw']) != W.bits(old['dw'])).sum())} elements differ"
    db = {"db": prepared(c)[1]["db"]}                            # db goes through fp32 atomics: the derived bound, not the bits
    for roll, got in ((1, new), (0, old)):
        ok, ratios = R.accepts(c, {"db": got["db"]}, db)
        assert ok, f"{c.id} db roll={roll}: {ratios}"


@gpu
@pytest.mark.parametrize("roll", (1, 0))
@pytest.mark.parametrize("cls", ("exact", "random"))
@pytest.mark.parametrize("s", ROLL64, ids=sid)
def test_w64_against_the_fp64_reference(L, workspace, s, cls, roll):
    c = conv(cls, s, seed=60)
    check(c, run(L, workspace, c, roll), f"roll={roll}")


@gpu
@pytest.mark.parametrize("s", ROLL128, ids=sid)
def test_w128_exact_equals_reference_and_staging(L, workspace, s):
    c = conv("exact", s)
    new, old = run(L, workspace, c, 1), run(L, workspace, c, 0)
    check(c, new, "roll=1")
    check(c, old, "roll=0")
    for k in new:
        assert torch.equal(W.bits(new[k]), W.bits(old[k])), (c.id, k)


@gpu
@pytest.mark.parametrize("s", ROLL128, ids=sid)
def test_w128_random_within_bound_and_repeatable(L, workspace, s):
    c = conv("random", s, seed=61)
    first = run(L, workspace, c, 1)
    check(c, first, "roll=1")
    check(c, run(L, workspace, c, 0), "roll=0")
    again = run(L, workspace, c, 1)
    assert torch.equal(W.bits(again["dw"]), W.bits(first["dw"])), f"{c.id}: a second call gave other dW bits"


@gpu
def test_a_width_the_ring_does_not_cover_runs_the_same_code(L, workspace):
    c = conv("random", UNCOVERED, seed=62)
    new, old = run(L, workspace, c, 1), run(L, workspace, c, 0)
    check(c, new, "roll=1")
    assert torch.equal(W.bits(new["dw"]), W.bits(old["dw"]))


@gpu
@pytest.mark.parametrize("roll", (1, 0))
@pytest.mark.parametrize("cls", ("exact", "dyadic", "random"))
@pytest.mark.parametrize("geo", HEAD_GEO, ids=sid)
@pytest.mark.parametrize("head", HEADS, ids=sid)
def test_smallconv_wgrad(L, workspace, head, geo, cls, roll):
    c = R.head_case("smallw", cls, *geo, *head, seed=63)
    check(c, run(L, workspace, c, roll), f"roll={roll}")


def both_stagings(L, workspace, c):
    """(roll = 1, roll = 0) outputs of a case WITHOUT the fp64 reference: for shapes whose im2col in fp64 would not fit a quick test.
    In the exact class every summation order gives the same fp32 bits, so the per-run staging -- checked against the reference on the
    small shapes above -- is the expectation."""
    inp = R.make_inputs(c)
    dev = W.upload(c, inp)
    h = L.lib()
    out = []
    was = W.get_option(L, "conv_wgrad_roll")
    try:
        for roll in (1, 0):
            L.check(h.srk_set_option(b"conv_wgrad_roll", roll))
            bufs = W.run(L, workspace, c, inp, dev, {}, R.WS_FULL)
            for k, b in bufs.items():
                b.assert_guards(f"{c.id} roll={roll} {k}")
            out.append({k: b.data() for k, b in bufs.items()})
    finally:
        L.check(h.srk_set_option(b"conv_wgrad_roll", was))
    return out


@gpu
def test_w128_splits_of_several_rows_exact(L, workspace):
    """Nine tiles, 28 splits of five image rows = ten runs: the row ring wraps, splits start mid-image and cross the image boundary."""
    new, old = both_stagings(L, workspace, conv("exact", (2, 64, 128, 192, 192)))
    for k in new:
        assert torch.equal(W.bits(new[k]), W.bits(old[k])), k


@gpu
def test_smallconv_wgrad_six_runs_per_workgroup_exact(L, workspace):
    """3072 chunks on 512 workgroups: six runs each, so the row ring and the dY ring wrap; a column of 64 runs and an image of 1024
    are no multiples of six, so workgroups cross column and image boundaries; W = 1024: both halo pixels are data for most runs."""
    new, old = both_stagings(L, workspace, R.head_case("smallw", "exact", 3, 64, 1024, 64, 64, 3, 4))
    for k in new:
        assert torch.equal(W.bits(new[k]), W.bits(old[k])), k


def test_option_round_trip():
    """Host only: conv_wgrad_roll is an option of srk_set_option / srk_get_option, 1 by default, any non-zero value reads back as 1."""
    from tpu_superresolution_amd._lib import check as ok, lib
    h = lib()

    def get():
        v = C.c_int(-1)
        ok(h.srk_get_option(b"conv_wgrad_roll", C.byref(v)))
        return v.value

    assert get() == 1
    try:
        ok(h.srk_set_option(b"conv_wgrad_roll", 0))
        assert get() == 0
        ok(h.srk_set_option(b"conv_wgrad_roll", 7))
        assert get() == 1
        taps = C.c_int(-1)
        ok(h.srk_get_option(b"conv_wgrad_taps", C.byref(taps)))
        assert taps.value == 2                                    # its neighbour keeps its values and its default
    finally:
        ok(h.srk_set_option(b"conv_wgrad_roll", 1))
