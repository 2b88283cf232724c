"""Direct parity of srk_gemm_ex (include/srk.h) through the C ABI: every (loader, epilogue) pair that srk_launch_gemm instantiates, on
the tile-per-workgroup kernel and on the persistent streaming kernel, against the fp64 restatement in tests/gemm_ex_ref.py.

Each case checks
  1. values, with the DERIVED tolerance of gemm_ex_ref (2 K u S accumulation bound, bf16 rounding, first-order propagation through the
     LayerNorm backward; no tuned constant) -- the log line of every case carries max(err / tol) per output;
  2. for the delta-weight cases, bit equality with a gather of the integer input (tap order, sub-pixel orders, crop);
  3. that nothing else is written: 256 guard rows before and after every output (and the guard columns of ldo > N) keep their NaN
     payload, bit for bit;
  4. the accumulate / in-place contracts (EP_LNBWD twice adds twice; EP_RES with outf aliasing res).

The comparator's ability to fail is shown on the CPU (tests/test_gemm_ex_ref.py, negative controls)."""
import ctypes as C

import pytest
import torch

import gemm_ex_ref as R
from guarded import DT, PAT, Guarded

pytestmark = pytest.mark.gpu

SRK_E_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib


def out_specs(c):
    """name -> (kind, rows, cols, ld, prefill key) of every output of the case."""
    M, N, LDO = c.M, c.N, c.LDO
    ep = c.ep
    s = {}
    if ep in (R.EP_BF16, R.EP_LRELU, R.EP_RES_BF16, R.EP_DGELU, R.EP_DLRELU):
        s["outb"] = ("bf16", M, N, LDO, None)
    elif ep == R.EP_GELU:
        s["outb2"] = ("bf16", M, N, LDO, None)
        if c.outb:
            s["outb"] = ("bf16", M, N, LDO, None)
    elif ep == R.EP_RES:
        s["outf"] = ("f32", M, N, LDO, None)
        if c.outb:
            s["outb"] = ("bf16", M, N, LDO, None)
        if c.xn_C:
            s["xn_out"] = ("bf16", M, N, N, None)
            s["xn_mean"] = ("f32", M, 1, 1, None)
            s["xn_rstd"] = ("f32", M, 1, 1, None)
    elif ep == R.EP_PS:
        B, H, Wd, _ = c.conv
        s["outb"] = ("bf16", B * H * c.r * Wd * c.r, c.Cs, c.Cs, None)
    elif ep in (R.EP_IMG, R.EP_PS_IMG):
        Hc, Wc = c.img_hw
        s["outf"] = ("f32", c.conv[0] * c.Cimg * Hc, Wc, Wc, None)
    elif ep == R.EP_F32_BF16:
        s["outf"] = ("f32", M, N, LDO, None)
        if c.outb:
            s["outb"] = ("bf16", M, N, LDO, None)
    elif ep == R.EP_LNBWD:
        s["outf"] = ("f32", M, N, LDO, "outf0")
        if c.outb:
            s["outb"] = ("bf16", M, N, LDO, None)
        s["ln_dgamma"] = ("f32", 1, c.ln_C, N, "dgamma0")        # entries >= ln_C are guard columns
        s["ln_dbeta"] = ("f32", 1, c.ln_C, N, "dbeta0")
    return s


def execute(L, c, inp, repeat=1, alias_res=False):
    """One (or `repeat`) srk_gemm_ex call(s) on guarded buffers -> (rc, {name: Guarded})."""
    dev = {k: v.cuda() for k, v in inp.items()}
    bufs = {}
    for name, (kind, rows, cols, ld, pre) in out_specs(c).items():
        fill = None
        if pre is not None:
            fill = inp[pre][None, :cols] if inp[pre].dim() == 1 else inp[pre][:, :cols]
        if alias_res and name == "outf":
            fill = inp["res"][:, :cols]
        bufs[name] = Guarded(kind, rows, cols, ld, fill)
    a = L.GemmArgs()
    a.loader, a.epilogue = c.loader, c.ep
    a.A, a.lda, a.W = dev["A"].data_ptr(), (c.LDA if c.loader == R.LD_ROWS else 0), dev["W"].data_ptr()
    a.M, a.N, a.K = c.M, c.N, c.K
    if c.conv is not None:
        a.B, a.H, a.Wd, a.CinP = c.conv
    a.r, a.Cs = c.r, c.Cs
    a.ldo, a.scale = c.LDO, c.scale
    ptr = lambda n: dev[n].data_ptr() if n in dev else None
    a.bias, a.aux, a.rowscale, a.rows_per_sample = ptr("bias"), ptr("aux"), ptr("rowscale"), c.rps
    a.res = bufs["outf"].ptr if alias_res else ptr("res")
    for name in ("outf", "outb", "outb2", "xn_out", "xn_mean", "xn_rstd", "ln_dgamma", "ln_dbeta"):
        setattr(a, name, bufs[name].ptr if name in bufs else None)
    if c.ep in (R.EP_IMG, R.EP_PS_IMG):
        inv, mean = R.img_params(c)
        a.inv_range, a.Cimg = inv, c.Cimg
        a.Hc, a.Wc = c.img_hw
        for i in range(4):
            a.mean[i] = mean[i]
    if c.xn_C:
        a.xn_gamma, a.xn_beta, a.xn_C = ptr("xn_gamma"), ptr("xn_beta"), c.xn_C
    if c.ep == R.EP_LNBWD:
        a.ln_x, a.ln_mean, a.ln_rstd, a.ln_gamma, a.ln_C = ptr("ln_x"), ptr("ln_mean"), ptr("ln_rstd"), ptr("ln_gamma"), c.ln_C
    st = torch.cuda.current_stream().cuda_stream
    rc = 0
    for _ in range(repeat):
        rc = L.lib().srk_gemm_ex(C.byref(a), st)
        if rc != 0:
            break
    torch.cuda.synchronize()
    return rc, bufs


_cache = {}


def inputs_and_reference(c):
    """The fp64 reference is built once per shape (a streaming case runs twice: streaming kernel and tile kernel)."""
    if c.id not in _cache:
        _cache.clear()                                   # the streaming references are large: keep one
        inp = R.make_inputs(c)
        _cache[c.id] = (inp, R.reference(c, inp))
    return _cache[c.id]


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_values(L, c, stream_on):
    inp, ref = inputs_and_reference(c)
    rc, bufs = execute(L, c, inp)
    assert rc == 0, (rc, L.lib().srk_last_error().decode())
    for name, b in bufs.items():
        b.assert_guards(f"{c.id} {name}")
    ratios = {}
    for name, o in ref.items():
        ok, ratios[name] = R.compare(bufs[name].data(), o)
    if c.xn_C:
        # stage 2: the fused LayerNorm against the fp64 LayerNorm of the device's own outf
        for name, o in R.ln_stage2(c, inp, bufs["outf"].data()).items():
            ok, ratios[name] = R.compare(bufs[name].data(), o)
        pad = bufs["xn_out"].data()[:, c.xn_C:]
        assert pad.numel() == 0 or bool((pad.view(torch.int16) == 0).all()), "pad columns of xn_out must be exactly 0"
    if c.ep == R.EP_LNBWD and c.ln_C < c.N:
        assert torch.equal(bufs["outf"].data()[:, c.ln_C:], inp["outf0"][:, c.ln_C:]), "pad columns of the gradient stream changed"
    print(f"[gemm_ex] {c.id} path={R.stream_path(c, n_cus(), stream_on)} " + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"max(err / tol) > 1: {bad}"


def get_option(L, name):
    v = C.c_int()
    L.check(L.lib().srk_get_option(name, C.byref(v)))
    return v.value


@pytest.mark.parametrize("c", R.value_cases(), ids=lambda c: c.id)
def test_values_and_guards(L, c):
    check_values(L, c, bool(get_option(L, b"gemm_stream")))


@pytest.mark.parametrize("mode", ["stream", "tile"])
@pytest.mark.parametrize("c", R.stream_cases(), ids=lambda c: c.id)
def test_streaming_shapes_on_both_implementations(L, c, mode):
    """The same fp64 reference at the same shape for the persistent streaming kernel and (gemm_stream = 0) the tile kernel."""
    was = get_option(L, b"gemm_stream")
    try:
        L.check(L.lib().srk_set_option(b"gemm_stream", 1 if mode == "stream" else 0))
        check_values(L, c, mode == "stream")
    finally:
        L.check(L.lib().srk_set_option(b"gemm_stream", was))


@pytest.mark.parametrize("c", R.exact_cases(), ids=lambda c: c.id)
def test_delta_weight_outputs_are_bit_equal_to_a_gather(L, c):
    inp = R.make_inputs(c)
    exp = R.exact_expected(c, inp)
    rc, bufs = execute(L, c, inp)
    assert rc == 0, (rc, L.lib().srk_last_error().decode())
    (name, b), = bufs.items()
    b.assert_guards(f"{c.id} {name}")
    got = b.data()
    want = exp.to(DT[b.kind])
    assert want.double().equal(exp)
    ity = PAT[b.kind][0]
    diff = got.view(ity) != want.view(ity)
    assert not bool(diff.any()), f"{int(diff.sum())} / {diff.numel()} elements differ, first at {[int(v) for v in diff.nonzero()[0]]}: " \
                                 f"got {float(got[diff][0])}, gather gives {float(want[diff][0])}"
    print(f"[gemm_ex] {c.id} bit-equal ({got.numel()} elements)")


def test_coverage_matrix_and_unsupported_pairs(L):
    """Every pair of the table has a value case (each value case is also a guard case: check_values asserts the guards) and, where it
    has an index map, a bit-exact case; every other pair of the two enums returns SRK_E_UNSUPPORTED with a message and writes nothing."""
    vals = R.value_cases() + R.stream_cases()
    for ld, eps in R.SUPPORTED.items():
        for ep in eps:
            assert any(c.loader == ld and c.ep == ep for c in vals), (ld, ep)
    for ld, ep in R.INDEX_MAP_PAIRS:
        assert any(c.loader == ld and c.ep == ep for c in R.exact_cases()), (ld, ep)
    n = 0
    for ld in R.LOADERS:
        for ep in R.EPILOGUES:
            if ep in R.SUPPORTED[ld]:
                continue
            c = R.unsupported_case(ld, ep)
            rc, bufs = execute(L, c, R.make_inputs(c))
            msg = L.lib().srk_last_error().decode()
            assert rc == SRK_E_UNSUPPORTED and msg, (c.id, rc, msg)
            for name, b in bufs.items():
                b.assert_untouched(f"{c.id}: {name}")
            n += 1
    assert n == 3 * 12 - sum(len(v) for v in R.SUPPORTED.values())
    # an epilogue number outside the enum
    c = R.unsupported_case(R.LD_ROWS, R.EP_F32_BF16)
    a = L.GemmArgs()
    a.loader, a.epilogue = R.LD_ROWS, 100
    assert L.lib().srk_gemm_ex(C.byref(a), None) == SRK_E_UNSUPPORTED


@pytest.mark.parametrize("c", [R.Case(R.LD_ROWS, R.EP_LNBWD, M=351, N=192, K=192, ln_C=180, rps=100, seed=70),
                               R.Case(R.LD_ROWS, R.EP_LNBWD, M=16384, N=192, K=576, ln_C=180, rps=64, seed=71)], ids=lambda c: c.id)
def test_lnbwd_accumulates(L, c):
    """Two calls on pre-filled outf / ln_dgamma / ln_dbeta add the same contribution twice."""
    inp = R.make_inputs(c)
    ref = R.reference(c, inp)
    rc, bufs = execute(L, c, inp, repeat=2)
    assert rc == 0, (rc, L.lib().srk_last_error().decode())
    ratios = {}
    f = inp["rowscale"].double()[torch.arange(c.M) // c.rps][:, None]
    for name, old in (("outf", inp["outf0"].double()), ("ln_dgamma", inp["dgamma0"].double()[None, :c.ln_C]),
                      ("ln_dbeta", inp["dbeta0"].double()[None, :c.ln_C])):
        twice = R.Out(2 * ref[name].ref - old, 2 * ref[name].tol, "f32")
        ok, ratios[name] = R.compare(bufs[name].data(), twice)
        if name == "outf":
            yb = twice.ref * f
            ok, ratios["outb"] = R.compare(bufs["outb"].data(), R.Out(yb, R.Tol.scaled_bf16(yb, f, twice.tol), "bf16"))
    for name, b in bufs.items():
        b.assert_guards(f"{c.id} {name}")
    print(f"[gemm_ex] twice {c.id} path={R.stream_path(c, n_cus(), True)} " + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("c", [R.Case(R.LD_ROWS, R.EP_RES, M=351, N=192, K=384, xn_C=180, rps=100, seed=72),
                               R.Case(R.LD_ROWS, R.EP_RES, M=1000, N=384, K=192, ldo=448, seed=73),
                               R.Case(R.LD_ROWS, R.EP_RES, M=16384, N=192, K=192, xn_C=180, seed=74),
                               R.conv_case(R.LD_CONV3, R.EP_RES, 3, 13, 9, 64, 192, xn_C=180, seed=75)], ids=lambda c: c.id)
def test_res_in_place_equals_separate_buffers(L, c):
    """outf aliasing res (the way the models call it) gives bit for bit what separate buffers give."""
    inp = R.make_inputs(c)
    rc, sep = execute(L, c, inp)
    assert rc == 0, (rc, L.lib().srk_last_error().decode())
    rc, ali = execute(L, c, inp, alias_res=True)
    assert rc == 0, (rc, L.lib().srk_last_error().decode())
    for name in sep:
        ali[name].assert_guards(f"{c.id} {name} (in place)")
        ity = PAT[sep[name].kind][0]
        assert torch.equal(sep[name].data().view(ity), ali[name].data().view(ity)), name
    assert torch.isfinite(ali["outf"].data()).all()

