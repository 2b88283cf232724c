"""Direct parity of the fused per-block Swin kernels in the form the SwinIR executor launches them, through the C ABI
(srk_mlp_fused_fwd_ex, srk_mlp_fused_bwd_ex, srk_qkv_window_attention_fwd, srk_proj_residual_fwd, srk_qkv_dgrad_lnbwd) against the fp64
restatements of tests/block_ref.py.

Each case checks
  1. values STAGE BY STAGE with the derived tolerances of block_ref.BTol: an exposed intermediate against the fp64 value from the bf16
     operands, the stage behind it against the fp64 evaluation from the device's own intermediate -- the log line of every case carries
     max(err / tol) per output;
  2. exact zeros in every pad column, out == res bit for bit where the DropPath factor is 0;
  3. that nothing else is written: 256 guard rows before and after every output keep their NaN payload;
  4. bit equality of the runs that store no intermediate with the storing run, of attn_fused 1 with 2, of the fused MLP forward with
     srk_gemm_ex(EP_GELU) + srk_gemm_ex(EP_RES), and of out / h between the two u_dgelu variants;
  5. which kernel ran and which GEMM path ran where predicted (launch counters);
  6. the accumulate contracts and that every refusal leaves its outputs untouched.

The comparator's ability to fail is shown on the CPU (tests/test_block_ref.py, negative controls)."""
import ctypes as C

import pytest
import torch

import block_ref as R
import gemm_ex_ref as G
from guarded import PAT, Guarded

pytestmark = pytest.mark.gpu

SRK_E_UNSUPPORTED = -3
CP, HP, CA = R.CP, R.HP, R.CA


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cases(kind):
    """The ids are those of the 256-CU matrix (no device is touched at collection); `shape_inputs` maps a case to the device's CU count."""
    return [c for c in R.all_cases(256) if c.kind == kind]


_cache = {}


def shape_inputs(c):
    """-> (case for this device, inputs on the host, on the device, the GEMM core); a shape's operands and stage results are built once
    and left unchanged."""
    c = R.for_device(c, n_cus())
    if _cache.get("key") != c.shape_key:
        _cache.clear()
        inp = R.make_inputs(c)
        _cache.update(key=c.shape_key, inp=inp, dev={k: v.cuda() for k, v in inp.items()}, core=R.CORES[c.kind](inp))
    return c, _cache["inp"], _cache["dev"], _cache["core"]


def memo(name, fn):
    if name not in _cache:
        _cache[name] = fn()
    return _cache[name]


def geom(L, c):
    return C.byref(L.WinGeom(c.H, c.W, c.shift))


def stream():
    return torch.cuda.current_stream().cuda_stream


def rowscale_dev(c):
    f = R.rowscale(c)
    return None if f is None else f.cuda()


def err(L):
    return L.lib().srk_last_error().decode()


def get_option(L, name):
    v = C.c_int()
    L.check(L.lib().srk_get_option(name, C.byref(v)))
    return v.value


class option:
    """Set a kernel option for the duration of a block and restore the previous value."""

    def __init__(self, L, name, value):
        self.L, self.name, self.value = L, name, value

    def __enter__(self):
        self.was = get_option(self.L, self.name)
        self.L.check(self.L.lib().srk_set_option(self.name, self.value))

    def __exit__(self, *a):
        self.L.check(self.L.lib().srk_set_option(self.name, self.was))


def bits_equal(a: Guarded, b: Guarded):
    ity = PAT[a.kind][0]
    return torch.equal(a.data().view(ity), b.data().view(ity))


def check(ratios, name, got: Guarded, out: R.Out):
    ratios[name] = R.compare(got.data(), out)[1]


def finish(tag, c, bufs, ratios, extra=""):
    for name, b in bufs.items():
        b.assert_guards(f"{c.id} {name}")
    print(f"[block] {tag} {c.id} {extra}" + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"max(err / tol) > 1: {bad}"


def assert_zero_pads(b: Guarded, first, what, period=None):
    d = b.data().view(PAT[b.kind][0])
    pad = d[:, first:] if period is None else d.view(d.shape[0], -1, period)[..., first:]
    assert bool((pad == 0).all()), f"{what}: pad columns must be exactly 0"


# ---- fused MLP forward ---------------------------------------------------------------------------------------------------------------
def run_mlp_fwd(L, c, dev, store=True, dg=None, window=True, M=None, rps=None, no_u=False):
    M = c.M if M is None else M
    bufs = {"out": Guarded("f32", M, CP, CP), "outb": Guarded("bf16", M, CP, CP), "xn_out": Guarded("bf16", M, CP, CP),
            "xn_mean": Guarded("f32", M, 1, 1), "xn_rstd": Guarded("f32", M, 1, 1)}
    if store:
        bufs.update(u=Guarded("bf16", M, HP, HP), h=Guarded("bf16", M, HP, HP))
    f = rowscale_dev(c)
    p = lambda n: bufs[n].ptr if n in bufs else None
    rc = L.lib().srk_mlp_fused_fwd_ex(dev["xn"].data_ptr(), dev["w1"].data_ptr(), dev["b1"].data_ptr(), dev["w2"].data_ptr(), dev["b2"].data_ptr(),
                                      dev["res"].data_ptr(), p("out"), p("outb"), None if no_u else p("u"), p("h"), c.dg if dg is None else dg,
                                      p("xn_out"), p("xn_mean"), p("xn_rstd"), dev["gamma"].data_ptr(), dev["beta"].data_ptr(), R.C,
                                      geom(L, c) if window else None, None if f is None else f.data_ptr(), c.rps if rps is None else rps, M, stream())
    torch.cuda.synchronize()
    return rc, bufs


def mlp_launches(L):
    return [[int(L.lib().srk_mlp_fused_launches(b, d)) for d in (0, 1)] for b in (0, 1)]


@pytest.mark.parametrize("c", cases("mlp_fwd"), ids=lambda c: c.id)
def test_mlp_fused_forward(L, c):
    c, inp, dev, core = shape_inputs(c)
    before = mlp_launches(L)
    rc, bufs = run_mlp_fwd(L, c, dev)
    assert rc == 0, (rc, err(L))
    after = mlp_launches(L)
    assert after[0][c.dg] == before[0][c.dg] + 1 and after[0][1 - c.dg] == before[0][1 - c.dg], "the other u_dgelu variant ran"
    ratios = {}
    s1 = memo(("s1", c.dg), lambda: R.mlp_fwd_stage1(c, inp, core))
    check(ratios, "u", bufs["u"], s1["u"])
    check(ratios, "h", bufs["h"], s1["h"])
    s2 = R.mlp_fwd_stage2(c, inp, bufs["h"].data())                       # from the device's own h
    check(ratios, "out", bufs["out"], s2["out"])
    out_dev = bufs["out"].data()
    assert torch.equal(bufs["outb"].data().view(torch.int16), out_dev.to(torch.bfloat16).view(torch.int16)), "out_bf16 is not bf16(out)"
    for name, o in R.ln_rows(c, inp, out_dev, True).items():            # from the device's own fp32 rows
        check(ratios, name, bufs[name], o)
    f = R.row_factor(c, torch.arange(c.M))[:, 0]
    if bool((f == 0).any()):
        assert torch.equal(out_dev[f == 0].view(torch.int32), inp["res"][f == 0].view(torch.int32)), "a dropped sample's out must be res, bit for bit"
    for name in ("out", "outb", "xn_out"):
        assert_zero_pads(bufs[name], R.C, f"{c.id} {name}")
    if not c.dg:
        assert_zero_pads(bufs["u"], R.HID, f"{c.id} u")
    assert_zero_pads(bufs["h"], R.HID, f"{c.id} h")
    finish("mlp_fwd", c, bufs, ratios)


@pytest.mark.parametrize("c", [c for c in cases("mlp_fwd") if c.rs == "mix" and c.dg], ids=lambda c: c.id)
def test_mlp_fused_forward_variants_are_bit_equal(L, c):
    """Only the stores differ: the inference run (no u / h) and the u_dgelu = 0 run give bit for bit the out / out_bf16 / xn_next /
    statistics (and h) of the u_dgelu = 1 run."""
    c, inp, dev, core = shape_inputs(c)
    rc, full = run_mlp_fwd(L, c, dev)
    assert rc == 0, (rc, err(L))
    rc, plain = run_mlp_fwd(L, c, dev, dg=0)
    assert rc == 0, (rc, err(L))
    rc, infer = run_mlp_fwd(L, c, dev, store=False, dg=0)
    assert rc == 0, (rc, err(L))
    for name in ("out", "outb", "xn_out", "xn_mean", "xn_rstd"):
        assert bits_equal(full[name], plain[name]), f"{name}: u_dgelu 1 vs 0"
        assert bits_equal(full[name], infer[name]), f"{name}: storing vs inference run"
        infer[name].assert_guards(f"{c.id} {name} (inference)")
    assert bits_equal(full["h"], plain["h"]), "h: u_dgelu 1 vs 0"


def test_mlp_fused_forward_equals_the_two_gemms(L):
    """Token-order form with a row scale: bit equal to srk_gemm_ex(EP_GELU) followed by srk_gemm_ex(EP_RES) (as the model-level tests
    assert for the whole network)."""
    c = [c for c in cases("mlp_fwd") if c.rs == "mix" and not c.dg and c.H != c.W][0]
    c, inp, dev, core = shape_inputs(c)
    rc, fused = run_mlp_fwd(L, c, dev, window=False)
    assert rc == 0, (rc, err(L))
    sep = {"out": Guarded("f32", c.M, CP, CP), "outb": Guarded("bf16", c.M, CP, CP), "xn_out": Guarded("bf16", c.M, CP, CP),
           "xn_mean": Guarded("f32", c.M, 1, 1), "xn_rstd": Guarded("f32", c.M, 1, 1), "u": Guarded("bf16", c.M, HP, HP), "h": Guarded("bf16", c.M, HP, HP)}
    a = L.GemmArgs()
    a.loader, a.epilogue, a.A, a.lda, a.W, a.M, a.N, a.K = G.LD_ROWS, G.EP_GELU, dev["xn"].data_ptr(), CP, dev["w1"].data_ptr(), c.M, HP, CP
    a.bias, a.outb, a.outb2, a.ldo = dev["b1"].data_ptr(), sep["u"].ptr, sep["h"].ptr, HP
    L.check(L.lib().srk_gemm_ex(C.byref(a), stream()))
    f = rowscale_dev(c)
    a = L.GemmArgs()
    a.loader, a.epilogue, a.A, a.lda, a.W, a.M, a.N, a.K = G.LD_ROWS, G.EP_RES, sep["h"].ptr, HP, dev["w2"].data_ptr(), c.M, CP, HP
    a.bias, a.res, a.outf, a.outb, a.ldo = dev["b2"].data_ptr(), dev["res"].data_ptr(), sep["out"].ptr, sep["outb"].ptr, CP
    a.xn_out, a.xn_mean, a.xn_rstd, a.xn_gamma, a.xn_beta, a.xn_C = (sep["xn_out"].ptr, sep["xn_mean"].ptr, sep["xn_rstd"].ptr, dev["gamma"].data_ptr(),
                                                                    dev["beta"].data_ptr(), R.C)
    a.rowscale, a.rows_per_sample = f.data_ptr(), c.rps
    L.check(L.lib().srk_gemm_ex(C.byref(a), stream()))
    torch.cuda.synchronize()
    for name in sep:
        assert bits_equal(fused[name], sep[name]), name
    # the token-order LayerNorm against the fp64 one of the device's rows
    ratios = {}
    for name, o in R.ln_rows(c, inp, fused["out"].data(), False).items():
        check(ratios, name, fused[name], o)
    finish("mlp_fwd token-order", c, fused, ratios)


# ---- fused MLP backward --------------------------------------------------------------------------------------------------------------
def run_mlp_bwd(L, c, inp, dev, repeat=1, window=True, M=None, rps=None):
    M = c.M if M is None else M
    bufs = {"du": Guarded("bf16", M, HP, HP), "gx": Guarded("f32", M, CP, CP, inp["gx0"][:M]), "gxb": Guarded("bf16", M, CP, CP),
            "dgamma": Guarded("f32", 1, R.C, CP, inp["dgamma0"][None]), "dbeta": Guarded("f32", 1, R.C, CP, inp["dbeta0"][None])}
    f = rowscale_dev(c)
    rc = 0
    for _ in range(repeat):
        rc = L.lib().srk_mlp_fused_bwd_ex(dev["g"].data_ptr(), dev["w2t"].data_ptr(), dev["udg" if c.dg else "u"].data_ptr(), c.dg, bufs["du"].ptr,
                                          dev["w1t"].data_ptr(), dev["ln_x"].data_ptr(), dev["ln_mean"].data_ptr(), dev["ln_rstd"].data_ptr(),
                                          dev["ln_gamma"].data_ptr(), bufs["gx"].ptr, bufs["gxb"].ptr, geom(L, c) if window else None,
                                          None if f is None else f.data_ptr(), c.rps if rps is None else rps, bufs["dgamma"].ptr, bufs["dbeta"].ptr,
                                          R.C, M, stream())
        if rc:
            break
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize("c", cases("mlp_bwd"), ids=lambda c: c.id)
def test_mlp_fused_backward(L, c):
    c, inp, dev, core = shape_inputs(c)
    before = mlp_launches(L)
    rc, bufs = run_mlp_bwd(L, c, inp, dev)
    assert rc == 0, (rc, err(L))
    after = mlp_launches(L)
    assert after[1][c.dg] == before[1][c.dg] + 1 and after[1][1 - c.dg] == before[1][1 - c.dg], "the other u_dgelu variant ran"
    ratios = {}
    check(ratios, "du", bufs["du"], memo(("s1", c.dg), lambda: R.mlp_bwd_stage1(c, inp, core))["du"])
    for name, o in R.mlp_bwd_stage2(c, inp, bufs["du"].data()).items():   # from the device's own d u
        check(ratios, name, bufs[name], o)
    assert torch.equal(bufs["gx"].data()[:, R.C:], inp["gx0"][:, R.C:]), "pad columns of the gradient stream changed"
    assert_zero_pads(bufs["gxb"], R.C, f"{c.id} gxb")
    assert_zero_pads(bufs["du"], R.HID, f"{c.id} du")
    f = R.row_factor(c, R.win_to_token(c.B, c.H, c.W, c.shift))[:, 0]
    if bool((f == 0).any()):
        assert bool((bufs["gxb"].data()[f == 0].view(torch.int16) & 0x7FFF == 0).all()), "gxb of a dropped sample must be 0"
    finish("mlp_bwd", c, bufs, ratios)


@pytest.mark.parametrize("c", [c for c in cases("mlp_bwd") if c.rs == "mix" and c.shift == 4 and c.H != c.W and c.B > 1], ids=lambda c: c.id)
def test_mlp_fused_backward_accumulates(L, c):
    """Two calls on pre-filled gx / d_gamma / d_beta add the same contribution twice."""
    c, inp, dev, core = shape_inputs(c)
    rc, bufs = run_mlp_bwd(L, c, inp, dev, repeat=2)
    assert rc == 0, (rc, err(L))
    once = R.mlp_bwd_stage2(c, inp, bufs["du"].data())
    ratios = {}
    f = R.row_factor(c, torch.arange(c.M))
    tok = R.win_to_token(c.B, c.H, c.W, c.shift)
    for name, old in (("gx", inp["gx0"].double()), ("dgamma", inp["dgamma0"].double()[None]), ("dbeta", inp["dbeta0"].double()[None])):
        twice = R.Out(2 * once[name].ref - old, 2 * once[name].tol, "f32")
        check(ratios, name, bufs[name], twice)
        if name == "gx":
            yb = (twice.ref * f)[tok]
            check(ratios, "gxb", bufs["gxb"], R.Out(yb, R.Tol.scaled_bf16(yb, f[tok], twice.tol[tok]), "bf16"))
    finish("mlp_bwd twice", c, bufs, ratios)


# ---- qkv projection + window attention forward -------------------------------------------------------------------------------------------
def run_attn(L, c, dev, mode, store=True, B_=None, nH=R.NH):
    B_ = c.B_ if B_ is None else B_
    bufs = {"ao": Guarded("bf16", B_ * 64, CA, CA)}
    if store:
        bufs["qkv"] = Guarded("bf16", 3 * B_ * R.NH * 64, R.DP, R.DP)
    lib = L.lib()
    before = (int(lib.srk_qkv_attn_fwd8_launches()), int(lib.srk_qkv_attn_fwd3_launches()))
    with option(L, b"attn_fused", mode):
        rc = lib.srk_qkv_window_attention_fwd(dev["xn"].data_ptr(), c.lda, dev["wqkv"].data_ptr(), dev["bqkv"].data_ptr(), R.SCALE,
                                              bufs["qkv"].ptr if store else None, dev["biasd"].data_ptr(), bufs["ao"].ptr, B_, nH, geom(L, c), stream())
    torch.cuda.synchronize()
    ran = (int(lib.srk_qkv_attn_fwd8_launches()) - before[0], int(lib.srk_qkv_attn_fwd3_launches()) - before[1])
    return rc, bufs, ran


def attn_inputs(L, c):
    c, inp, dev, core = shape_inputs(c)
    if "biasd" not in dev:
        dev["biasd"] = R.dense_bias(inp["table"]).cuda()
        got = torch.empty_like(dev["biasd"])
        L.check(L.lib().srk_rel_pos_bias_expand(dev["table"].data_ptr(), got.data_ptr(), R.NH, stream()))
        assert torch.equal(got, dev["biasd"]), "srk_rel_pos_bias_expand is not table[relative_position_index]"
    return c, inp, dev, core


@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("c", cases("attn"), ids=lambda c: c.id)
def test_qkv_window_attention_forward(L, c, mode):
    c, inp, dev, core = attn_inputs(L, c)
    rc, bufs, ran = run_attn(L, c, dev, mode)
    assert rc == 0, (rc, err(L))
    assert ran == ((0, 1) if mode == 2 else (1, 0)), f"attn_fused = {mode} ran (8-wave, 4-wave) = {ran}"
    ratios = {}
    check(ratios, "qkv", bufs["qkv"], memo("qkv", lambda: R.attn_qkv(c, inp, R.SCALE, core)))
    check(ratios, "ao", bufs["ao"], R.attn_out(c, inp, bufs["qkv"].data()))      # from the device's own q / k / v
    assert_zero_pads(bufs["qkv"], R.D, f"{c.id} qkv")
    assert_zero_pads(bufs["ao"], R.D, f"{c.id} ao", period=R.DP)
    # the run that stores no q / k / v: only the stores differ
    rc, bare, ran = run_attn(L, c, dev, mode, store=False)
    assert rc == 0, (rc, err(L))
    assert bits_equal(bufs["ao"], bare["ao"]), "ao with and without qkv_out"
    bare["ao"].assert_guards(f"{c.id} ao (no qkv_out)")
    if mode == 1:                                                            # ... and the two kernels agree bit for bit
        rc, other, ran2 = run_attn(L, c, dev, 2)
        assert rc == 0 and ran2 == (0, 1), (rc, ran2)
        assert bits_equal(bufs["ao"], other["ao"]) and bits_equal(bufs["qkv"], other["qkv"]), "attn_fused 1 vs 2"
    finish(f"attn mode={mode} kernels(8w,4w)={ran}", c, bufs, ratios)


# ---- proj + window reverse + un-roll + residual + DropPath + norm2 -----------------------------------------------------------------------
def run_proj(L, c, dev, ln=True):
    M = c.M
    bufs = {"out": Guarded("f32", M, CP, CP)}
    if ln:
        bufs.update(xn_out=Guarded("bf16", M, CP, CP), xn_mean=Guarded("f32", M, 1, 1), xn_rstd=Guarded("f32", M, 1, 1))
    f = rowscale_dev(c)
    p = lambda n: bufs[n].ptr if n in bufs else None
    rc = L.lib().srk_proj_residual_fwd(dev["ao"].data_ptr(), dev["w"].data_ptr(), dev["b"].data_ptr(), dev["res"].data_ptr(), bufs["out"].ptr,
                                       None if f is None else f.data_ptr(), c.rps, p("xn_out"), p("xn_mean"), p("xn_rstd"), dev["gamma"].data_ptr(),
                                       dev["beta"].data_ptr(), R.C, c.B_, geom(L, c), stream())
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize("path", ["stream", "tile"])
@pytest.mark.parametrize("c", cases("proj"), ids=lambda c: c.id)
def test_proj_residual_forward(L, c, path):
    c, inp, dev, core = shape_inputs(c)
    before = int(L.lib().srk_gemm_stream_launches())
    with option(L, b"gemm_stream", 1 if path == "stream" else 0):
        rc, bufs = run_proj(L, c, dev)
    assert rc == 0, (rc, err(L))
    predicted = R.stream_path(c, n_cus(), path == "stream")
    ran = "stream" if int(L.lib().srk_gemm_stream_launches()) == before + 1 else "tile"
    assert ran == predicted, f"the {ran} kernel ran where the {predicted} kernel was predicted"
    ratios = {}
    check(ratios, "out", bufs["out"], memo(("out", c.rs, c.shift), lambda: R.proj_residual(c, inp, core))["out"])
    out_dev = bufs["out"].data()
    for name, o in R.ln_rows(c, inp, out_dev, False).items():
        check(ratios, name, bufs[name], o)
    f = R.row_factor(c, torch.arange(c.M))[:, 0]
    if bool((f == 0).any()):
        assert torch.equal(out_dev[f == 0].view(torch.int32), inp["res"][f == 0].view(torch.int32)), "a dropped sample's out must be res, bit for bit"
    assert_zero_pads(bufs["out"], R.C, f"{c.id} out")
    assert_zero_pads(bufs["xn_out"], R.C, f"{c.id} xn_out")
    finish(f"proj path={predicted}", c, bufs, ratios)


# ---- qkv dgrad + norm1 backward + window reverse + un-roll (+ RSTB skip fold) -------------------------------------------------------------
def run_lnbwd(L, c, inp, dev, repeat=1):
    M = c.M
    bufs = {"gx": Guarded("f32", M, CP, CP, inp["gx0"]), "gxb": Guarded("bf16", M, CP, CP),
            "dgamma": Guarded("f32", 1, R.C, CP, inp["dgamma0"][None]), "dbeta": Guarded("f32", 1, R.C, CP, inp["dbeta0"][None])}
    if c.skip:
        bufs["skip"] = Guarded("f32", M, CP, CP, inp["skip0"])
    f = rowscale_dev(c)
    rc = 0
    for _ in range(repeat):
        rc = L.lib().srk_qkv_dgrad_lnbwd(dev["dqkv"].data_ptr(), dev["wt"].data_ptr(), dev["ln_x"].data_ptr(), dev["ln_mean"].data_ptr(),
                                         dev["ln_rstd"].data_ptr(), dev["ln_gamma"].data_ptr(), bufs["gx"].ptr, bufs["gxb"].ptr,
                                         None if f is None else f.data_ptr(), c.rps, bufs["skip"].ptr if c.skip else None, bufs["dgamma"].ptr,
                                         bufs["dbeta"].ptr, R.C, c.B_, geom(L, c), stream())
        if rc:
            break
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize("path", ["stream", "tile"])
@pytest.mark.parametrize("c", cases("lnbwd"), ids=lambda c: c.id)
def test_qkv_dgrad_lnbwd(L, c, path):
    c, inp, dev, core = shape_inputs(c)
    before = int(L.lib().srk_gemm_stream_launches())
    with option(L, b"gemm_stream", 1 if path == "stream" else 0):
        rc, bufs = run_lnbwd(L, c, inp, dev)
    assert rc == 0, (rc, err(L))
    predicted = R.stream_path(c, n_cus(), path == "stream")
    ran = "stream" if int(L.lib().srk_gemm_stream_launches()) == before + 1 else "tile"
    assert ran == predicted, f"the {ran} kernel ran where the {predicted} kernel was predicted"
    ratios = {}
    for name, o in memo(("ref", c.rs, c.shift, c.skip), lambda: R.qkv_dgrad_lnbwd(c, inp, core)).items():
        check(ratios, name, bufs[name], o)
    if c.skip:
        assert bufs["gx"].data().view(torch.int32).equal(inp["gx0"].view(torch.int32)), "ln_skip form: outf must stay untouched"
    assert_zero_pads(bufs["gxb"], R.C, f"{c.id} gxb")
    f = R.row_factor(c, torch.arange(c.M))[:, 0]
    if bool((f == 0).any()):
        assert bool((bufs["gxb"].data()[f == 0].view(torch.int16) & 0x7FFF == 0).all()), "gxb of a dropped sample must be 0"
    finish(f"lnbwd path={predicted}", c, bufs, ratios)


@pytest.mark.parametrize("c", [c for c in cases("lnbwd") if c.rs == "mix" and c.H != c.W and c.B > 1], ids=lambda c: c.id)
def test_qkv_dgrad_lnbwd_accumulates(L, c):
    """Two calls add the same contribution twice: to gx, or in the ln_skip form to ln_skip (gx + dx enters twice), and to d_gamma / d_beta."""
    c, inp, dev, core = shape_inputs(c)
    rc, bufs = run_lnbwd(L, c, inp, dev, repeat=2)
    assert rc == 0, (rc, err(L))
    once = R.qkv_dgrad_lnbwd(c, inp, core)
    target = "skip" if c.skip else "gx"
    old = (inp["skip0"] if c.skip else inp["gx0"]).double()
    ratios = {}
    f = R.row_factor(c, torch.arange(c.M))
    twice = R.Out(2 * once[target].ref - old, 2 * once[target].tol, "f32")
    check(ratios, target, bufs[target], twice)
    yb = twice.ref * f
    check(ratios, "gxb", bufs["gxb"], R.Out(yb, R.Tol.scaled_bf16(yb, f, twice.tol), "bf16"))
    for name, o0 in (("dgamma", inp["dgamma0"]), ("dbeta", inp["dbeta0"])):
        check(ratios, name, bufs[name], R.Out(2 * once[name].ref - o0.double()[None], 2 * once[name].tol, "f32"))
    finish("lnbwd twice", c, bufs, ratios)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def refused(L, rc, bufs, what):
    msg = err(L)
    assert rc == SRK_E_UNSUPPORTED and msg, (what, rc, msg)
    for name, b in bufs.items():
        b.assert_untouched(f"{what}: {name}")


def test_refusals_leave_every_output_untouched(L):
    """Host-side returns before any launch: M % 64 != 0, M < 64 n, rows_per_sample % 64 != 0 with a rowscale, u_dgelu without u_out
    (fused MLP pair); B_ < n, nH != 6, attn_fused = 0 (attention)."""
    n = n_cus()
    full = 64 * (n & ~7)

    def fwd(c, **kw):
        c, inp, dev, core = shape_inputs(c)
        return run_mlp_fwd(L, c, dev, **kw)

    def bwd(c, **kw):
        c, inp, dev, core = shape_inputs(c)
        return run_mlp_bwd(L, c, inp, dev, **kw)

    for kind, run in (("mlp_fwd", fwd), ("mlp_bwd", bwd)):
        c = [c for c in cases(kind) if c.H == c.W == 64 and c.rs == "mix" and c.dg][0]
        rc, bufs = run(R.with_(c, rs="none"), window=False, M=full - 32)
        refused(L, rc, bufs, f"{kind} M % 64 != 0")
        rc, bufs = run(R.with_(c, rs="none"), window=False, M=full - 64)
        refused(L, rc, bufs, f"{kind} M < 64 n")
        rc, bufs = run(c, rps=32)
        refused(L, rc, bufs, f"{kind} rows_per_sample % 64 != 0")
    c = [c for c in cases("mlp_fwd") if c.H == c.W == 64 and c.rs == "none" and c.dg][0]
    rc, bufs = fwd(c, no_u=True)
    assert rc == -2 and err(L), "u_out without h_out is a null-pointer error"
    rc, bufs = fwd(c, store=False, dg=1)
    refused(L, rc, bufs, "mlp_fwd u_dgelu without u_out")
    c = [c for c in cases("attn") if c.H == c.W == 8 and c.shift == 0][0]
    c, inp, dev, core = attn_inputs(L, c)
    rc, bufs, ran = run_attn(L, c, dev, 2, B_=n - 1)
    refused(L, rc, bufs, "attention B_ < n")
    rc, bufs, ran = run_attn(L, c, dev, 2, nH=3)
    refused(L, rc, bufs, "attention nH != 6")
    rc, bufs, ran = run_attn(L, c, dev, 0)
    refused(L, rc, bufs, "attention attn_fused = 0")
    assert ran == (0, 0)


def test_host_checks_of_the_new_entry_points(L):
    """Null pointers, alignment, geometry: errors before any launch."""
    c = [c for c in cases("proj") if c.small][0]
    c, inp, dev, core = shape_inputs(c)
    lib = L.lib()
    out = Guarded("f32", c.M, CP, CP)
    args = lambda **kw: [kw.get("ao", dev["ao"].data_ptr()), dev["w"].data_ptr(), dev["b"].data_ptr(), dev["res"].data_ptr(), kw.get("out", out.ptr), None, 0,
                         None, None, None, None, None, 0, kw.get("B_", c.B_), kw.get("geom", geom(L, c)), stream()]
    assert lib.srk_proj_residual_fwd(*args(ao=None)) == -2
    assert lib.srk_proj_residual_fwd(*args(ao=dev["ao"].data_ptr() + 2)) == -5
    assert lib.srk_proj_residual_fwd(*args(geom=C.byref(L.WinGeom(8, 12, 0)))) == -1 and b"multiples of 8" in lib.srk_last_error()
    assert lib.srk_proj_residual_fwd(*args(geom=C.byref(L.WinGeom(8, 8, 2)))) == -1 and b"shift" in lib.srk_last_error()
    assert lib.srk_proj_residual_fwd(*args(geom=C.byref(L.WinGeom(16, 16, 0)))) == -1 and b"multiple of H*W" in lib.srk_last_error()
    assert lib.srk_proj_residual_fwd(*args(out=dev["res"].data_ptr())) == -1
    out.assert_untouched("proj_residual_fwd host checks")


# ---- d beta on integer operands: exact in ANY summation order ---------------------------------------------------------------------------
def _sparse_signs(rows, cols, live_rows, live_cols, period):
    """{-1, 0, 1} weights: entry (r, c) is non-zero where (r + c) % period == 0, signs scrambled; pads zero."""
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    w = torch.where((r + c) % period == 0, torch.where((7 * r + 13 * c) % 11 < 6, 1.0, -1.0), 0.0)
    w[live_rows:] = 0.0
    w[:, live_cols:] = 0.0
    return w


def _small_ints(rows, cols, live_cols, lim, salt):
    idx = torch.arange(rows * cols, dtype=torch.int64) + 7919 * salt
    v = (((idx * 2654435761) >> 7) % (2 * lim + 1) - lim).reshape(rows, cols).float()
    v[:, live_cols:] = 0.0
    return v


@pytest.mark.parametrize("kind,path", [("lnbwd", "stream"), ("lnbwd", "tile"), ("mlp_bwd", "stream")])
def test_dbeta_of_integer_operands_is_exact(L, kind, path):
    """The derived bound of d gamma / d beta (M u sum|dy| for M atomic additions in any order) is about the weight of ONE 16-row tile at
    these M, so it cannot see a dropped tile.  With small-integer operands every GEMM result and every partial sum of d beta = sum_m dy[m]
    is an integer below 2^24: the fp32 result is the same in every order, and the assertion is equality -- one missing, doubled or
    misplaced row fails.  (The same rows feed d gamma and the gradient stream.)"""
    c = [c for c in cases(kind) if c.H != c.W and c.B > 1 and c.shift == 4 and c.rs == "none" and (kind != "mlp_bwd" or c.dg)][0]
    c = R.for_device(c, n_cus())
    _cache.clear()
    inp = R.make_inputs(c)
    inp["dbeta0"] = _small_ints(1, R.C, R.C, 50, 3)[0]
    if kind == "lnbwd":
        inp["dqkv"] = R._heads(_small_ints(c.M, 3 * CA, 3 * CA, 3, 1)).to(torch.bfloat16)
        inp["wt"] = R._heads(_sparse_signs(CP, 3 * CA, R.C, 3 * CA, 5)).to(torch.bfloat16)
        acc = inp["dqkv"].double() @ inp["wt"].double().t()
        bound = float((inp["dqkv"].double().abs() @ inp["wt"].double().abs().t()).sum(0).max())
    else:
        inp["g"] = _small_ints(c.M, CP, R.C, 1, 1).to(torch.bfloat16)
        inp["w2t"] = _sparse_signs(HP, CP, R.HID, R.C, 16).to(torch.bfloat16)
        inp["w1t"] = _sparse_signs(CP, HP, R.C, R.HID, 16).to(torch.bfloat16)
        inp["udg"] = torch.ones(c.M, HP).to(torch.bfloat16)                 # gelu'(u) = 1: d u = d h
        du = inp["g"].double() @ inp["w2t"].double().t()
        assert float(du.abs().max()) <= 256                                # integers that bf16 holds exactly
        acc = du @ inp["w1t"].double().t()
        bound = float((du.abs() @ inp["w1t"].double().abs().t()).sum(0).max())
    assert bound + 50 < 2 ** 24
    assert bool((acc[:, :R.C].view(-1, 16, R.C).sum(1) != 0).any(1).all()), "every 16-row tile must contribute to some column"
    want = inp["dbeta0"].double() + acc[:, :R.C].sum(0)
    dev = {k: v.cuda() for k, v in inp.items()}
    with option(L, b"gemm_stream", 1 if path == "stream" else 0):
        rc, bufs = (run_lnbwd if kind == "lnbwd" else run_mlp_bwd)(L, c, inp, dev)
    assert rc == 0, (rc, err(L))
    got = bufs["dbeta"].data()[0].double()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {R.C} columns differ, max |diff| {float((got - want).abs().max())}"
    if kind == "mlp_bwd":
        assert torch.equal(bufs["du"].data().double(), du), "d u of integer operands"
    for name, b in bufs.items():
        b.assert_guards(f"{c.id} {name}")
    print(f"[block] dbeta exact {kind} path={path} {c.id} ({c.M} rows, |sum| <= {bound:.0f})")
