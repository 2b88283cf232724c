"""CPU pins of tests/wgrad_ref.py: the fp64 restatement of the weight-gradient entry points equals torch.autograd, an fp32 emulation of
the kernels' summation stays inside the derived tolerance (and is bit-equal on the exact class), every negative control FAILS the
comparator, and the restated dispatch reaches every kernel of the family."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ex_ref as G
import wgrad_ref as R

D = torch.float64


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _grads(out, wrt, dout):
    return torch.autograd.grad(out, wrt, dout)


def test_case_ids_are_unique_and_every_random_or_dyadic_case_has_an_exact_twin():
    ids = [c.id for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for c in R.CASES:
        assert c.kind in R.KINDS and c.cls in ("exact", "dyadic", "random")
        assert c.cls != "dyadic" or c.kind in R.FP32_DY
        if c.cls != "exact" and c.kind != "imgprep":
            t = R.twin(c)
            assert t is not None and t.cls == "exact" and t.M == c.M, c.id
    # what the issue's matrix names
    lin = [c for c in R.CASES if c.kind == "linear" and not c.multi]
    assert {R._tile_class(c.probs[0].N, c.probs[0].K) for c in lin} == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    assert {c.M for c in lin if (c.probs[0].N, c.probs[0].K) == (192, 192)} >= set(R.LINEAR_M)
    assert any(c.M % 64 and R._tile_class(c.probs[0].N, c.probs[0].K) == (3, 3) for c in lin)
    assert {(c.geo + (c.CinP, c.N)) for c in R.CASES if c.kind == "conv"} >= set(R.CONV_SHAPES)
    assert max(c.M for c in R.CASES) <= 32768 and max(c.M for c in R.CASES if c.kind != "linear") <= 16384


# ---- autograd pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [R.linear_case("random", 130, (64, 128)),
                               R.linear_case("exact", 100, R.Prob(192, 64, ldy=256, ldx=128, yoff=64, xoff=64), R.Prob(64, 64, db=False)),
                               R.linear_case("random", 70, *R._wide(R.BLOCK[:2]))], ids=lambda c: c.id)
def test_linear_reference_is_autograd_of_f_linear(c):
    inp = R.make_inputs(c)
    ref = R.reference(c, inp)
    for i, p in enumerate(c.probs):
        x, y = inp[f"x{i}"].double(), inp[f"y{i}"].double()
        # the operands as the device sees them: column slices of wider buffers
        xb, yb = R.embed(x, p.LDX, p.xoff, before=3, after=5), R.embed(y, p.LDY, p.yoff, before=3, after=5)
        assert torch.equal(xb[3:3 + c.M, p.xoff:p.xoff + p.K], x) and torch.equal(yb[3:3 + c.M, p.yoff:p.yoff + p.N], y)
        assert torch.isnan(xb).sum() == xb.numel() - x.numel()
        w = torch.zeros(p.N, p.K, dtype=D, requires_grad=True)
        b = torch.zeros(p.N, dtype=D, requires_grad=True)
        dw, db = _grads(F.linear(x, w, b), (w, b), y)
        torch.testing.assert_close(ref[f"dw{i}"] - inp[f"dw{i}_0"].double(), dw, rtol=1e-12, atol=1e-12)
        if p.db:
            torch.testing.assert_close(ref[f"db{i}"] - inp[f"db{i}_0"].double(), db, rtol=1e-12, atol=1e-12)
        else:
            assert f"db{i}" not in ref


@pytest.mark.parametrize("c", [R.conv_case("random", 2, 5, 7, 64, 64), R.conv_case("exact", 1, 1, 9, 64, 128),
                               R.conv_case("random", 2, 3, 4, 64, 256, r=2, Cs=64), R.conv_case("exact", 1, 4, 3, 64, 576, r=3, Cs=64)],
                         ids=lambda c: c.id)
def test_conv_reference_is_autograd_of_conv2d_and_pixel_shuffle(c):
    B, H, W = c.geo
    inp = R.make_inputs(c)
    ref = R.reference(c, inp)
    x = _nchw(inp["x"].double())
    r, Cs = c.r, c.Cs or c.N
    wt = torch.zeros(c.N, c.CinP, 3, 3, dtype=D, requires_grad=True)
    b = torch.zeros(c.N, dtype=D, requires_grad=True)
    out = F.conv2d(x, wt, b, padding=1)
    if c.kind == "convps":
        out = F.pixel_shuffle(out, r)                        # torch channel c * r * r + i * r + j
        dout = _nchw(inp["y"].double())                      # the stored gradient: NHWC [B][H * r][W * r][Cs]
    else:
        dout = _nchw(inp["y"].double().reshape(B, H, W, c.N))
    dw, db = _grads(out, (wt, b), dout)
    ours_n = torch.arange(c.N)
    if c.kind == "convps":                                   # our row n = (i * r + j) * Cs + ch  <->  torch row ch * r * r + i * r + j
        ij, ch = ours_n // Cs, ours_n % Cs
        torch_n = ch * r * r + ij
    else:
        torch_n = ours_n
    got = R._dw_layout(ref["dw"] - inp["dw_0"].double(), c.N, c.CinP, c.CinP)
    torch.testing.assert_close(got, dw[torch_n], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["db"] - inp["db_0"].double(), db[torch_n], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", [R.prep_case(2, 5, 9, 1, 3, 4), R.prep_case(2, 5, 9, 1, 1, 4), R.prep_case(2, 5, 9, 2, 3, 16),
                               R.prep_case(2, 5, 9, 2, 3, 16, crop=(1, 3)), R.prep_case(1, 3, 4, 3, 1, 16, crop=(2, 1)),
                               R.prep_case(1, 4, 6, 2, 3, 16, crop=(1, 3), cls="random")], ids=lambda c: c.id)
def test_img_grad_prep_reference_is_autograd_of_the_image_head(c):
    """The forward image head is pixel_shuffle(v) * inv_range (+ mean), cropped to Hc x Wc (gemm_ex_ref.ps_img_store)."""
    B, H, W = c.geo
    inp = R.make_inputs(c)
    inv = float(torch.tensor(R.EXACT_INV_RANGE if c.cls == "exact" else R.IMG_INV_RANGE, dtype=torch.float32))
    v = torch.zeros(B, c.CoP, H, W, dtype=D, requires_grad=True)
    Hc, Wc = c.img_hw
    img = F.pixel_shuffle(v[:, :c.Cimg * c.r * c.r], c.r)[:, :, :Hc, :Wc] * inv
    gv, = _grads(img, (v,), inp["d_pred"].double())
    got = R.reference(c, inp)["gy"].reshape(B, H, W, c.CoP)
    torch.testing.assert_close(_nchw(got), gv, rtol=1e-7, atol=0.0)
    if c.cls == "exact":
        assert torch.equal(_nchw(got), gv)
    # and it is the inverse of the forward store of gemm_ex_ref
    fwd = G.ps_img_store(got.reshape(c.M, c.CoP), B, H, W, c.r, c.Cimg)[:, :, :Hc, :Wc]
    assert torch.equal(fwd, (inp["d_pred"] * torch.tensor(inv, dtype=torch.float32)).double())


@pytest.mark.parametrize("c", [R.head_case(k, cls, 2, 5, 7, *h) for k in ("smallw", "smalld")
                               for cls, h in (("random", (64, 64, 3, 4)), ("exact", (64, 64, 1, 4)), ("dyadic", (60, 64, 12, 16)),
                                              ("random", (180, 192, 12, 16)))] +
                              [R.stem_case("random", 2, 5, 7, 3, 60, 64), R.stem_case("exact", 1, 4, 9, 1, 180, 192),
                               R.stem_case("dyadic", 1, 6, 5, 3, 96, 128)], ids=lambda c: c.id)
def test_image_head_and_stem_references_are_autograd_of_conv2d(c):
    B, H, W = c.geo
    inp = R.make_inputs(c)
    ref = R.reference(c, inp)
    gy = _nchw(inp["gy"].double().reshape(B, H, W, c.CoP)[..., :c.Co])
    assert not inp["gy"][:, c.Co:].any(), "pad channels of gy are zero"
    if c.kind == "smalld":
        x = torch.zeros(B, c.Cin, H, W, dtype=D, requires_grad=True)
        dx, = _grads(F.conv2d(x, inp["weight"].double(), padding=1), (x,), gy)
        got = ref["dx"].reshape(B, H, W, c.CinP)
        torch.testing.assert_close(_nchw(got[..., :c.Cin]), dx, rtol=1e-12, atol=1e-12)
        assert not got[..., c.Cin:].any(), "pad channels of dx are zero"
        return
    src = inp["x"] if c.kind == "smallw" else inp["img4"]
    x = _nchw(src.double()[..., :c.Cin])
    wt = torch.zeros(c.Co, c.Cin, 3, 3, dtype=D, requires_grad=True)
    b = torch.zeros(c.Co, dtype=D, requires_grad=True)
    dw, db = _grads(F.conv2d(x, wt, b, padding=1), (wt, b), gy)
    torch.testing.assert_close(ref["dw"] - inp["dw_0"].double(), dw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["db"] - inp["db_0"].double(), db, rtol=1e-12, atol=1e-12)


def test_input_classes_are_what_they_claim():
    v = R.dyadic((64, 33), 7)
    hi = v.to(torch.bfloat16).float()
    lo = v - hi
    assert bool((lo > 0).all()) and bool((lo.to(torch.bfloat16).float() == lo).all())      # not one bf16; hi + lo IS the value
    assert float((lo / v).min()) > 2.0 ** -11
    p = R.pow2((64, 33), 3)
    assert bool((torch.log2(p) == torch.log2(p).round()).all())
    e = R.ints((100, 70), 2, 1)
    assert float(e.abs().max()) == 2 and len({tuple(r.tolist()) for r in e}) == 100          # no two rows alike
    assert not bool((R.ints((100, 70), 5, 2, nonzero=True) == 0).any())
    for c in R.CASES:
        if c.cls == "exact" and c.kind in ("smallw", "smalld", "stem") and c.M <= 512:
            inp = R.make_inputs(c)
            for k in ("gy", "weight", "img4"):
                if k in inp:
                    assert torch.equal(inp[k].to(torch.bfloat16).float(), inp[k]), (c.id, k)   # bf16-exact: hi + lo is exact too


# ---- the reference alone satisfies the conditions: fp32 emulation of the kernels' summation -----------------------------------------
_cache = {}


def _expected(c):
    if c.id not in _cache:
        _cache.clear()
        inp = R.make_inputs(c)
        _cache[c.id] = (inp, R.expected(c, inp))
    return _cache[c.id]


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_fp32_emulation_of_the_summation_is_inside_the_bound_and_exact_on_the_exact_class(c):
    inp, exp = _expected(c)
    for m_per in (256, 64 * 7):                              # two different splits: the exact class does not depend on it
        got = R.emulate(c, inp, m_per)
        assert set(got) == set(exp)
        ok, ratios = R.accepts(c, got, exp)
        assert ok, (m_per, ratios)
        if c.cls == "exact" or c.kind == "imgprep":
            for k, o in exp.items():
                assert torch.equal(got[k].double(), o.ref) and torch.equal(o.rounded(), o.ref), k
            if c.M > 4096:
                break
    if c.cls != "exact":
        print(f"[wgrad_ref] {c.id} " + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))


# ---- negative controls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in R.CASES if c.cls == "exact" or c.kind == "imgprep"], ids=lambda c: c.id)
def test_every_mutation_fails_the_comparator_on_the_exact_class(c):
    inp, exp = _expected(c)
    ctl = R.controls_for(c)
    if c.kind in R.ACCUMULATING:
        assert {"dW0 overwritten"} <= set(ctl) and (c.M < 2 or {"row dropped at a split boundary", "row counted twice"} <= set(ctl))
        assert ("tail rows dropped" in ctl) == (c.M % 64 != 0 and c.M > 64)
    if c.kind in ("conv", "convps", "smallw", "smalld", "stem"):
        assert "taps swapped" in ctl
    if c.r > 1:
        assert "(i, j) swapped" in ctl
    if c.crop != (0, 0):
        assert "crop ignored" in ctl
    assert ctl or (c.kind == "imgprep" and c.r == 1 and c.crop == (0, 0))
    for name, m in ctl.items():
        ok, ratios = R.accepts(c, R.reference(c, inp, m), exp)
        assert not ok, f"the comparator accepted '{name}': {ratios}"


@pytest.mark.parametrize("c", [c for c in R.CASES if c.cls == "dyadic"], ids=lambda c: c.id)
def test_omitting_the_lo_half_fails_the_comparator_on_the_dyadic_class(c):
    inp, exp = _expected(c)
    ctl = R.controls_for(c)
    ok, ratios = R.accepts(c, R.reference(c, inp, ctl["lo half omitted"]), exp)
    assert not ok, f"a result without the lo halves was accepted: {ratios}"
    ok, ratios = R.accepts(c, R.reference(c, inp, ctl["taps swapped"]), exp)
    assert not ok, ratios


def test_tolerance_cannot_see_a_missing_row_at_large_m_but_the_exact_twin_can():
    """The argument for the exact class, in numbers: at M = 16384 + 64 * 37 a dropped row is inside the derived bound of the random
    case and fails the exact twin."""
    c = next(c for c in R.CASES if c.id == "linear-M18752-192x192-random")
    inp = R.make_inputs(c)
    ok, ratios = R.accepts(c, R.reference(c, inp, R.Mut(drop_row=256)), R.expected(c, inp))
    assert ok and 0.0 < max(ratios.values()) < 1.0, ratios
    t = R.twin(c)
    inp = R.make_inputs(t)
    ok, _ = R.accepts(t, R.reference(t, inp, R.Mut(drop_row=256)), R.expected(t, inp))
    assert not ok


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------
def test_dispatch_table_reaches_every_kernel_of_the_family():
    seen = {}
    for c in R.CASES:
        for name, (opts, ws) in R.option_sets(c).items():
            for k in R.EXPECTED_KERNEL(c, opts, ws):
                seen.setdefault(k, f"{c.id} [{name}]")
    missing = [k for k in R.KERNELS if k not in seen]
    assert not missing, missing
    assert set(seen) <= set(R.KERNELS), set(seen) - set(R.KERNELS)


def test_dispatch_table_restates_the_launcher_conditions():
    K = R.EXPECTED_KERNEL
    lin = lambda M, *nk: R.linear_case("exact", M, *nk)
    assert K(lin(4096, (192, 192))) == ["wgrad_stream_kernel<32, true, true>", "wgrad_reduce_kernel"]
    assert K(lin(4096, (192, 192)), workspace=0) == ["wgrad_stream_kernel<32, true, true>"]
    assert K(lin(4096, (192, 192)), workspace=1024) == ["wgrad_stream_kernel<32, true, true>"]
    assert K(lin(4096, (192, 192)), {"wgrad_partials": 0}) == ["wgrad_stream_kernel<32, true, true>"]
    assert K(lin(256, (192, 192))) == ["wgrad_stream_kernel<32, true, true>"]                  # one split: nothing to reduce
    assert K(lin(4096 + 17, (192, 192))) == ["wgrad_kernel<3, 3, false>"]                      # M % 64 != 0 leaves the streaming kernel
    assert K(lin(4096, (192, 192)), {"wgrad_stream": 0}) == ["wgrad_kernel<3, 3, false>"]
    assert K(lin(4096, (384, 576)), {"wgrad_stream_rows": 64, "wgrad_stream_nt": 0, "wgrad_stream_w8": 0}) == [
        "wgrad_stream_kernel<64, false, false>", "wgrad_reduce_kernel"]
    assert K(lin(700, (256, 320))) == ["wgrad_kernel<2, 1, false>"]
    assert K(lin(4096, *R.BLOCK)) == ["wgrad_stream_kernel<32, true, true>", "wgrad_reduce_kernel"]      # one launch
    assert K(lin(1000, *R.MIXED)) == ["wgrad_kernel<3, 3, false>", "wgrad_kernel<1, 2, false>", "wgrad_kernel<2, 1, false>",
                                      "wgrad_kernel<3, 1, false>"]                                   # one by one
    assert K(lin(4096, (576, 64), (192, 64))) == ["wgrad_kernel<3, 1, false>"]                       # same class: together
    cv = lambda *a, **kw: R.conv_case("exact", *a, **kw)
    assert K(cv(4, 64, 64, 192, 192)) == ["conv_wgrad_taps_dma_kernel<false>", "conv_wgrad_taps_reduce_kernel"]
    assert K(cv(4, 64, 64, 192, 192), workspace=0) == ["conv_wgrad_taps_dma_kernel<false>"]
    assert K(cv(1, 1, 64, 64, 64)) == ["conv_wgrad_taps_dma_kernel<false>"]                    # one run of 64 pixels: one split
    assert K(cv(2, 8, 64, 64, 256, r=2, Cs=64), {"conv_wgrad_taps": 1}) == ["conv_wgrad_taps_kernel<true>"]
    assert K(cv(2, 8, 64, 64, 64), {"conv_wgrad_taps": 0}) == ["wgrad_kernel<*, *, true>"]
    assert K(cv(2, 16, 16, 64, 64)) == ["wgrad_kernel<*, *, true>"]                            # W % 64 != 0
    hd = lambda kind, geo, h, **kw: R.head_case(kind, "exact", *geo, *h)
    assert K(hd("smallw", (2, 4, 64), (64, 64, 3, 4))) == ["smallconv_wgrad_mfma_kernel<4>"]
    assert K(hd("smallw", (2, 4, 64), (180, 192, 12, 16))) == ["smallconv_wgrad_mfma_kernel<16>"]
    assert K(hd("smallw", (1, 6, 24), (64, 64, 3, 4))) == ["smallconv_wgrad_kernel<4>"]
    assert K(hd("smallw", (2, 4, 64), (64, 64, 3, 4)), {"conv_wgrad_taps": 0}) == ["smallconv_wgrad_kernel<4>"]
    assert K(hd("smalld", (2, 4, 64), (64, 64, 3, 4))) == ["imghead_dgrad_mfma_kernel"]
    assert K(hd("smalld", (1, 7, 9), (64, 64, 3, 4))) == ["smallconv_dgrad_kernel"]
    assert K(hd("smalld", (2, 4, 64), (60, 64, 12, 16))) == ["smallconv_dgrad_kernel"]         # CoP == 16: VALU
    assert R.smalld_lds_bytes(hd("smalld", (2, 4, 64), (180, 192, 12, 16))) > 64 * 1024 >= R.smalld_lds_bytes(hd("smalld", (2, 4, 64), (60, 64, 12, 16)))
    st = lambda *a: R.stem_case("exact", *a)
    assert K(st(4, 64, 64, 3, 180, 192)) == ["stem_wgrad_mfma_kernel", "stem_wgrad_reduce_kernel"]
    assert K(st(4, 64, 64, 3, 180, 192), workspace=0) == ["stem_wgrad_kernel"]
    assert K(st(1, 32, 511, 3, 180, 192)) == ["stem_wgrad_kernel"]
    assert K(st(4, 64, 64, 3, 96, 128)) == ["stem_wgrad_kernel"]
