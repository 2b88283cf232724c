"""CPU-only checks: the C-ABI library builds/loads and exports every symbol include/srk.h declares, the
plan bookkeeping (pure host code) matches the reference's parameter schema, and the product path
fails loudly without a GPU."""
import ctypes as C
import os

import pytest
import torch

from oracle import swinir_oracle as O


@pytest.fixture(scope="module")
def lib():
    from tpu_superresolution_amd import build
    build.build(verbose=False)
    from tpu_superresolution_amd import _lib
    return _lib


def test_library_exports_every_declared_symbol(lib):
    names = lib.declared_symbols()
    assert len(names) >= 35
    handle = lib.lib()
    missing = [n for n in names if not hasattr(handle, n)]
    assert not missing, missing
    undeclared = [n for n in lib._SIGNATURES if n not in names]
    assert not undeclared, undeclared
    assert b"gfx950" in handle.srk_version()


def test_lds_limits_are_raised_in_one_place():
    """Launchers reserve dynamic LDS through srk_reserve_lds (csrc/api.hip): the two HIP runtime calls behind it are written
    in exactly one .hip file, so a hand-written copy of the reserve-once-per-device block fails here."""
    from tpu_superresolution_amd import build
    users = {call: [] for call in ("hipFuncSetAttribute", "hipFuncGetAttributes")}
    for name in sorted(os.listdir(build.CSRC)):
        if name.endswith(".hip"):
            with open(os.path.join(build.CSRC, name)) as f:
                text = f.read()
            for call in users:
                if call in text:
                    users[call].append(name)
    assert users == {"hipFuncSetAttribute": ["api.hip"], "hipFuncGetAttributes": ["api.hip"]}, users


@pytest.mark.parametrize("cfg", [O.SwinIRConfig.classical_x4(), O.SwinIRConfig.light_x2()])
def test_plan_parameter_table_matches_reference_schema(lib, cfg):
    from tpu_superresolution_amd.engine import SwinIRPlan
    plan = SwinIRPlan(img_size=cfg.img_size, in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, depths=cfg.depths,
                      num_heads=cfg.num_heads, window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio, upscale=cfg.upscale,
                      img_range=cfg.img_range, upsampler=cfg.upsampler)
    schema = [(k, tuple(s)) for k, s, kind in O.state_dict_schema(cfg) if kind == "param"]
    assert [(p.name, p.shape) for p in plan.params] == schema
    offs = [p.offset for p in plan.params]
    assert all(o % 64 == 0 for o in offs) and offs == sorted(offs)
    assert plan.param_floats >= sum(p.numel for p in plan.params)
    # backward segments tile the flat buffer back to front
    rs = plan.segment_ranges
    assert rs[0][1] == plan.param_floats and rs[-1][0] == 0
    assert all(rs[i][0] == rs[i + 1][1] for i in range(len(rs) - 1))
    assert len(rs) == len(cfg.depths) + 2


def test_module_state_dict_schema_and_loud_failure(lib):
    import tpu_superresolution_amd as T
    cfg = O.SwinIRConfig.light_x2()
    m = T.SwinIR(**cfg.kwargs())
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s, _ in O.state_dict_schema(cfg)]
    sd = O.random_state_dict(cfg, 1)
    m.load_state_dict(sd, strict=True)
    assert m.state_dict()["layers.0.residual_group.blocks.1.attn_mask"].shape == (64, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(1, 3, 16, 16))
    with pytest.raises(NotImplementedError):
        m.layers[0].residual_group.blocks[0](torch.rand(1, 64, 60), (8, 8))


def test_unsupported_configs_are_refused_by_the_c_api(lib):
    from tpu_superresolution_amd.engine import SwinIRPlan
    base = dict(img_size=64, in_chans=3, embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, window_size=8, mlp_ratio=2, upscale=4,
                img_range=1.0, upsampler="pixelshuffle")
    with pytest.raises(NotImplementedError, match="window_size == 8"):
        SwinIRPlan(**{**base, "window_size": 7})
    with pytest.raises(NotImplementedError, match="head_dim <= 32"):
        SwinIRPlan(**{**base, "num_heads": [3] * 6})
    with pytest.raises(ValueError, match="scale 5 is not supported"):
        SwinIRPlan(**{**base, "upscale": 5})
    with pytest.raises(NotImplementedError, match="upsamples by 2 or 4"):
        SwinIRPlan(**{**base, "upsampler": "nearest+conv", "upscale": 3})
    with pytest.raises(NotImplementedError, match="upscale must be 1"):
        SwinIRPlan(**{**base, "upsampler": "", "upscale": 2})
    with pytest.raises(ValueError, match="resi_connection"):
        SwinIRPlan(**{**base, "resi_connection": "2conv"})
    # every head / residual connection of the reference constructor has a plan, with the reference's parameter names
    for ups, s in (("nearest+conv", 4), ("nearest+conv", 2), ("", 1), ("pixelshuffledirect", 2)):
        for resi in ("1conv", "3conv"):
            names = [q.name for q in SwinIRPlan(**{**base, "upsampler": ups, "upscale": s, "resi_connection": resi,
                                                   "depths": [2, 2], "num_heads": [6, 6]}).params]
            assert ("conv_up2.weight" in names) == (ups == "nearest+conv" and s == 4)
            assert ("conv_hr.bias" in names) == (ups == "nearest+conv")
            assert ("layers.0.conv.2.weight" in names) == (resi == "3conv") == ("conv_after_body.4.bias" in names)


def test_index_entry_points_validate_arguments_without_a_gpu(lib):
    h = lib.lib()
    assert h.srk_window_partition(None, None, 1, 8, 8, 3, 8, 4, None) == -2
    assert h.srk_shift_mask(C.c_void_p(16), 64, 64, 8, 8, None) == -1
    assert b"shift_size must in 0-window_size" in h.srk_last_error()
    assert h.srk_window_partition(C.c_void_p(16), C.c_void_p(16), 1, 13, 8, 3, 8, 4, None) == -1


def test_gemm_ex_refuses_bad_argument_blocks_without_a_gpu(lib):
    """srk_gemm_ex returns on the host, before any launch, for a missing output, an image head / PixelShuffle / fused-LayerNorm
    geometry it cannot honour, and a loader the epilogue does not go with.  The addresses are dummies that are never dereferenced:
    every block here is one the entry point rejects."""
    h = lib.lib()
    P = 4096                                                     # a non-null address; never read or written

    def block(loader, ep, **kw):
        a = lib.GemmArgs()
        a.loader, a.epilogue = loader, ep
        a.A, a.W, a.lda = P, P, 64
        a.M, a.N, a.K, a.ldo = 64, 64, 64, 64
        a.bias, a.outf, a.outb, a.outb2, a.res, a.aux = P, P, P, P, P, P
        if loader != lib.LD_ROWS:
            a.B, a.H, a.Wd, a.CinP, a.K = 2, 4, 8, 64, 576
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, code):
        rc = h.srk_gemm_ex(C.byref(a), None)
        assert rc == code, (rc, code, h.srk_last_error())
        assert h.srk_last_error(), "no message"

    E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3
    R_, C3 = lib.LD_ROWS, lib.LD_CONV3
    # a null where the epilogue stores
    for ep, field in ((lib.EP_BF16, "outb"), (lib.EP_LRELU, "outb"), (lib.EP_GELU, "outb2"), (lib.EP_RES, "outf"), (lib.EP_RES, "res"),
                      (lib.EP_RES_BF16, "outb"), (lib.EP_RES_BF16, "res"), (lib.EP_DGELU, "outb"), (lib.EP_DLRELU, "aux")):
        refused(block(R_, ep, **{field: None}), E_NULL)
    refused(block(C3, lib.EP_PS, N=256, r=2, Cs=64, outb=None), E_NULL)
    refused(block(C3, lib.EP_F32_BF16, outf=None), E_NULL)
    img = dict(N=16, Cimg=3, Hc=4, Wc=8, inv_range=1.0)
    refused(block(C3, lib.EP_IMG, **{**img, "outf": None}), E_NULL)
    refused(block(C3, lib.EP_PS_IMG, **{**img, "r": 2, "outf": None}), E_NULL)
    # image heads
    refused(block(C3, lib.EP_IMG, **{**img, "N": 64}), E_SHAPE)
    refused(block(C3, lib.EP_IMG, **{**img, "Cimg": 0}), E_SHAPE)
    refused(block(C3, lib.EP_IMG, **{**img, "Cimg": 5}), E_SHAPE)            # mean[4] is indexed by channel
    refused(block(C3, lib.EP_IMG, **{**img, "Hc": 0}), E_SHAPE)
    refused(block(C3, lib.EP_IMG, **{**img, "Hc": 5}), E_SHAPE)              # H = 4
    refused(block(C3, lib.EP_IMG, **{**img, "Wc": 9}), E_SHAPE)              # Wd = 8
    refused(block(C3, lib.EP_PS_IMG, **{**img, "r": 0}), E_SHAPE)
    refused(block(C3, lib.EP_PS_IMG, **{**img, "r": 3}), E_SHAPE)            # 3 * 9 > 16 columns: channels would be dropped silently
    assert b"Cimg * r * r <= 16" in h.srk_last_error()
    refused(block(C3, lib.EP_PS_IMG, **{**img, "r": 2, "Hc": 9, "Wc": 16}), E_SHAPE)
    refused(block(C3, lib.EP_PS_IMG, **{**img, "r": 2, "Hc": 8, "Wc": 17}), E_SHAPE)
    # conv + PixelShuffle
    refused(block(C3, lib.EP_PS, N=256, r=0, Cs=64), E_SHAPE)
    refused(block(C3, lib.EP_PS, N=128, r=2, Cs=32), E_SHAPE)
    refused(block(C3, lib.EP_PS, N=192, r=2, Cs=64), E_SHAPE)
    # fused LayerNorm of EP_RES
    ln = dict(xn_out=P, xn_mean=P, xn_rstd=P, xn_gamma=P, xn_beta=P)
    refused(block(R_, lib.EP_RES, **ln, xn_C=0), E_SHAPE)
    refused(block(R_, lib.EP_RES, **ln, xn_C=65), E_SHAPE)
    refused(block(R_, lib.EP_RES, **ln, xn_C=60, ldo=128), E_SHAPE)
    # a row scale without its epilogue / without rows_per_sample
    refused(block(R_, lib.EP_BF16, rowscale=P, rows_per_sample=64), E_SHAPE)
    refused(block(R_, lib.EP_RES, rowscale=P, rows_per_sample=0), E_SHAPE)
    # loaders and epilogues outside the exposed surface
    lnb = dict(ln_x=P, ln_mean=P, ln_rstd=P, ln_gamma=P, ln_dgamma=P, ln_dbeta=P, ln_C=60, bias=None)
    refused(block(C3, lib.EP_LNBWD, **lnb), E_UNSUPPORTED)
    refused(block(R_, lib.EP_LNBWD, **{**lnb, "ln_dbeta": None}), E_NULL)
    refused(block(R_, lib.EP_LNBWD, **{**lnb, "ln_C": 65}), E_SHAPE)
    refused(block(3, lib.EP_BF16), E_UNSUPPORTED)
    refused(block(R_, 100), E_UNSUPPORTED)
    refused(block(R_, 1), E_UNSUPPORTED)
    assert h.srk_gemm_ex(None, None) == E_NULL


def test_weight_gradient_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """The weight-gradient family returns on the host, before any launch, for the shapes, strides and alignments its kernels cannot
    honour (include/srk.h states each rule at its entry point).  The addresses are dummies that are never dereferenced: every call here
    differs from a valid one in exactly the argument under test, and is rejected."""
    h = lib.lib()
    P = 4096                                                     # a non-null, 16-byte aligned address; never read or written
    E_SHAPE, E_NULL, E_ALIGN = -1, -2, -5

    def refused(rc, code):
        assert rc == code, (rc, code, h.srk_last_error())
        assert h.srk_last_error(), "no message"

    def variants(base, changes):
        """base: name -> valid value (in argument order); changes: (name, bad value, code)."""
        for name, bad, code in changes:
            yield [bad if k == name else v for k, v in base.items()], code, name

    # srk_linear_wgrad_bf16(y, x, dw, db, M, N, K, stream)
    base = dict(y=P, x=P, dw=P, db=None, M=64, N=64, K=64)
    for a, code, _ in variants(base, [("y", None, E_NULL), ("x", None, E_NULL), ("dw", None, E_NULL), ("y", P + 2, E_ALIGN), ("x", P + 8, E_ALIGN),
                                      ("M", 0, E_SHAPE), ("M", -64, E_SHAPE), ("N", 96, E_SHAPE), ("K", 100, E_SHAPE)]):
        refused(h.srk_linear_wgrad_bf16(*a, None), code)

    # srk_linear_wgrad_multi_bf16(problems, count, M, stream)
    def problems(n=2, **kw):
        arr = (lib.WgradProblem * 4)()
        for i in range(4):
            arr[i].y, arr[i].x, arr[i].dw, arr[i].db = P, P, P, None
            arr[i].N, arr[i].K, arr[i].ldy, arr[i].ldx = 192, 64, 256, 128
        for k, v in kw.items():
            setattr(arr[n - 1], k, v)                            # the LAST problem of the list carries the fault
        return arr

    refused(h.srk_linear_wgrad_multi_bf16(None, 1, 64, None), E_NULL)
    for count in (0, -1, 5):
        refused(h.srk_linear_wgrad_multi_bf16(problems(), count, 64, None), E_SHAPE)
    for M in (0, -64):
        refused(h.srk_linear_wgrad_multi_bf16(problems(), 2, M, None), E_SHAPE)
    for n in (1, 2, 3, 4):
        for kw, code in ((dict(N=100), E_SHAPE), (dict(K=32), E_SHAPE), (dict(N=0), E_SHAPE), (dict(ldy=128), E_SHAPE), (dict(ldx=56), E_SHAPE),
                         (dict(ldy=196), E_ALIGN), (dict(ldx=68), E_ALIGN), (dict(ldy=193), E_ALIGN), (dict(y=None), E_NULL), (dict(x=None), E_NULL),
                         (dict(dw=None), E_NULL), (dict(y=P + 4), E_ALIGN), (dict(x=P + 8), E_ALIGN)):
            refused(h.srk_linear_wgrad_multi_bf16(problems(n, **kw), n, 64, None), code)
    assert b"multiples of 8" in (h.srk_linear_wgrad_multi_bf16(problems(1, ldx=68), 1, 64, None), h.srk_last_error())[1]

    # srk_conv3x3_wgrad_bf16(y, x, dw, db, B, H, W, CinP, N, stream)  /  srk_conv3x3_wgrad_ps_bf16(..., N, r, Cs, stream)
    base = dict(y=P, x=P, dw=P, db=None, B=2, H=4, W=8, CinP=64, N=64)
    for a, code, _ in variants(base, [("y", None, E_NULL), ("x", None, E_NULL), ("dw", None, E_NULL), ("y", P + 2, E_ALIGN), ("x", P + 8, E_ALIGN),
                                      ("B", 0, E_SHAPE), ("H", -4, E_SHAPE), ("W", 0, E_SHAPE), ("CinP", 60, E_SHAPE), ("N", 16, E_SHAPE)]):
        refused(h.srk_conv3x3_wgrad_bf16(*a, None), code)
    base = dict(y=P, x=P, dw=P, db=None, B=2, H=4, W=8, CinP=64, N=256, r=2, Cs=64)
    for a, code, _ in variants(base, [("y", None, E_NULL), ("x", None, E_NULL), ("dw", None, E_NULL), ("y", P + 2, E_ALIGN), ("x", P + 8, E_ALIGN),
                                      ("B", 0, E_SHAPE), ("H", 0, E_SHAPE), ("W", -8, E_SHAPE), ("CinP", 60, E_SHAPE), ("N", 192, E_SHAPE),
                                      ("r", 0, E_SHAPE), ("r", 3, E_SHAPE), ("Cs", 32, E_SHAPE), ("Cs", 0, E_SHAPE)]):
        refused(h.srk_conv3x3_wgrad_ps_bf16(*a, None), code)
    refused(h.srk_conv3x3_wgrad_ps_bf16(P, P, P, None, 2, 4, 8, 64, 64, 4, 4, None), E_SHAPE)       # N == r*r*Cs but Cs % 8 != 0

    # srk_img_grad_prep(d_pred, gy, B, Cimg, Hc, Wc, H, W, r, CoP, inv_range, stream)
    base = dict(d_pred=P, gy=P, B=2, Cimg=3, Hc=8, Wc=16, H=4, W=8, r=2, CoP=16, inv_range=1.0)
    for a, code, _ in variants(base, [("d_pred", None, E_NULL), ("gy", None, E_NULL), ("B", 0, E_SHAPE), ("H", 0, E_SHAPE), ("W", -1, E_SHAPE),
                                      ("r", 0, E_SHAPE), ("r", 3, E_SHAPE), ("Cimg", 0, E_SHAPE), ("Cimg", 5, E_SHAPE), ("CoP", 8, E_SHAPE),
                                      ("CoP", 4, E_SHAPE), ("Hc", 9, E_SHAPE), ("Wc", 17, E_SHAPE), ("Hc", 0, E_SHAPE), ("Wc", 0, E_SHAPE)]):
        refused(h.srk_img_grad_prep(*a, None), code)

    # srk_smallconv_wgrad(x, gy, dw, db, B, H, W, Cin, CinP, Co, CoP, stream)  /  srk_smallconv_dgrad(gy, weight, dx, B, ..., stream)
    shape_faults = [("B", 0, E_SHAPE), ("H", 0, E_SHAPE), ("W", -3, E_SHAPE), ("Co", 5, E_SHAPE), ("Co", 0, E_SHAPE), ("CoP", 8, E_SHAPE),
                    ("CoP", 32, E_SHAPE), ("Cin", 65, E_SHAPE), ("Cin", 0, E_SHAPE), ("CinP", 60, E_SHAPE), ("CinP", 320, E_SHAPE)]
    base = dict(x=P, gy=P, dw=P, db=P, B=1, H=4, W=8, Cin=60, CinP=64, Co=3, CoP=4)
    for a, code, _ in variants(base, shape_faults + [("x", None, E_NULL), ("gy", None, E_NULL), ("dw", None, E_NULL), ("db", None, E_NULL),
                                                     ("x", P + 2, E_ALIGN), ("gy", P + 4, E_ALIGN)]):
        refused(h.srk_smallconv_wgrad(*a, None), code)
    base = dict(gy=P, weight=P, dx=P, B=1, H=4, W=8, Cin=60, CinP=64, Co=3, CoP=4)
    for a, code, _ in variants(base, shape_faults + [("gy", None, E_NULL), ("weight", None, E_NULL), ("dx", None, E_NULL), ("gy", P + 4, E_ALIGN),
                                                     ("dx", P + 8, E_ALIGN)]):
        refused(h.srk_smallconv_dgrad(*a, None), code)

    # srk_stem_wgrad(img4, gy, dw, db, B, H, W, Cin, C, CP, stream)
    base = dict(img4=P, gy=P, dw=P, db=P, B=1, H=4, W=8, Cin=3, C=60, CP=64)
    for a, code, _ in variants(base, [("img4", None, E_NULL), ("gy", None, E_NULL), ("dw", None, E_NULL), ("db", None, E_NULL), ("img4", P + 4, E_ALIGN),
                                      ("gy", P + 8, E_ALIGN), ("B", 0, E_SHAPE), ("H", 0, E_SHAPE), ("W", 0, E_SHAPE), ("Cin", 5, E_SHAPE),
                                      ("Cin", 0, E_SHAPE), ("C", 65, E_SHAPE), ("C", 0, E_SHAPE), ("CP", 62, E_SHAPE)]):
        refused(h.srk_stem_wgrad(*a, None), code)
    refused(h.srk_stem_wgrad(P, P, P, P, 1, 4, 8, 3, 260, 320, None), E_SHAPE)                      # C > 256: one thread per channel


def test_glue_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """LayerNorm, the image stem and the element-wise helpers of the host-orchestrated training paths return on the host, before any
    launch, for null pointers (SRK_E_NULL), shapes their kernels cannot honour (SRK_E_SHAPE) and addresses that their float4 / four-bf16
    accesses cannot take (SRK_E_ALIGN); include/srk.h states each rule at its entry point.  The addresses are dummies that are never
    dereferenced; every call differs from a valid one in exactly the argument under test."""
    h = lib.lib()
    P = 4096
    E_SHAPE, E_NULL, E_ALIGN = -1, -2, -5

    def sweep(fn, base, changes, tail=(None,)):
        for name, bad, code in changes:
            assert name in base, name
            args = [bad if k == name else v for k, v in base.items()]
            rc = fn(*args, *tail)
            assert rc == code, (fn.__name__, name, bad, rc, code, h.srk_last_error())
            assert h.srk_last_error(), "no message"

    # srk_layernorm_fwd(x, gamma, beta, y_bf16, y_f32, mean, rstd, rows, C, CP, geom, stream)
    base = dict(x=P, gamma=P, beta=P, y_bf16=P, y_f32=P, mean=P, rstd=P, rows=16, C=60, CP=64)
    sweep(h.srk_layernorm_fwd, base, [("CP", 320, E_SHAPE), ("CP", 96, E_SHAPE), ("C", 65, E_SHAPE), ("C", 0, E_SHAPE), ("rows", 0, E_SHAPE),
                                      ("mean", None, E_NULL), ("rstd", None, E_NULL), ("x", P + 4, E_ALIGN), ("x", None, E_NULL),
                                      ("gamma", None, E_NULL), ("beta", None, E_NULL)], tail=(None, None))
    assert h.srk_layernorm_fwd(P, P, P, None, None, P, P, 16, 60, 64, None, None) == E_NULL           # no output at all

    # srk_layernorm_bwd(dy, x, mean, rstd, gamma, gx, gx_bf16, dgamma, dbeta, rows, C, CP, accumulate, stream)
    base = dict(dy=P, x=P, mean=P, rstd=P, gamma=P, gx=P, gx_bf16=P, dgamma=P, dbeta=P, rows=16, C=60, CP=64, accumulate=0)
    sweep(h.srk_layernorm_bwd, base, [("CP", 320, E_SHAPE), ("CP", 100, E_SHAPE), ("C", 65, E_SHAPE), ("C", 0, E_SHAPE), ("rows", 0, E_SHAPE),
                                      ("rows", -16, E_SHAPE), ("dy", None, E_NULL), ("x", None, E_NULL), ("mean", None, E_NULL),
                                      ("rstd", None, E_NULL), ("gamma", None, E_NULL), ("gx", None, E_NULL), ("dgamma", None, E_NULL),
                                      ("dbeta", None, E_NULL), ("x", P + 4, E_ALIGN), ("gx", P + 8, E_ALIGN), ("dy", P + 2, E_ALIGN),
                                      ("dy", P + 4, E_ALIGN), ("gx_bf16", P + 2, E_ALIGN), ("gx_bf16", P + 12, E_ALIGN)])

    # srk_stem_conv(img4, weight, bias, out, B, H, W, Cin, C, CP, stream)
    base = dict(img4=P, weight=P, bias=P, out=P, B=1, H=4, W=8, Cin=3, C=60, CP=64)
    sweep(h.srk_stem_conv, base, [("img4", None, E_NULL), ("weight", None, E_NULL), ("bias", None, E_NULL), ("out", None, E_NULL),
                                  ("B", 0, E_SHAPE), ("H", 0, E_SHAPE), ("W", 0, E_SHAPE), ("W", -8, E_SHAPE), ("Cin", 0, E_SHAPE),
                                  ("Cin", 5, E_SHAPE), ("C", 0, E_SHAPE), ("C", 65, E_SHAPE), ("CP", 62, E_SHAPE), ("img4", P + 4, E_ALIGN),
                                  ("out", P + 8, E_ALIGN)])
    assert h.srk_stem_conv(P, P, P, P, 1, 4, 8, 3, 260, 320, None) == E_SHAPE                          # CP > 256: the LDS the kernel stages
    assert h.srk_stem_conv(P, P, P, P, 1, 4, 8, 3, 256, 260, None) == E_SHAPE

    # srk_img_prep(x, out, B, Cimg, H0, W0, H, W, range, mean3, stream)
    mean3 = (C.c_float * 3)(0.4488, 0.4371, 0.4040)
    base = dict(x=P, out=P, B=2, Cimg=3, H0=9, W0=9, H=17, W=16, range=1.0, mean3=C.byref(mean3))
    sweep(h.srk_img_prep, base, [("H", 18, E_SHAPE), ("W", 18, E_SHAPE), ("H", 8, E_SHAPE), ("Cimg", 4, E_SHAPE), ("Cimg", 0, E_SHAPE),
                                 ("B", 0, E_SHAPE), ("x", None, E_NULL), ("out", None, E_NULL), ("mean3", None, E_NULL),
                                 ("out", P + 4, E_ALIGN)])

    # srk_cast_f32_bf16(x, y, n, stream)
    sweep(h.srk_cast_f32_bf16, dict(x=P, y=P, n=64), [("x", None, E_NULL), ("y", None, E_NULL), ("n", 0, E_SHAPE), ("n", -4, E_SHAPE),
                                                      ("n", 66, E_SHAPE), ("x", P + 8, E_ALIGN), ("y", P + 4, E_ALIGN), ("y", P + 2, E_ALIGN)])
    # srk_add_f32_bf16(a, b, ab_bf16, n, stream)
    sweep(h.srk_add_f32_bf16, dict(a=P, b=P, ab=P, n=64), [("a", None, E_NULL), ("b", None, E_NULL), ("ab", None, E_NULL), ("n", 0, E_SHAPE),
                                                           ("n", 6, E_SHAPE), ("a", P + 4, E_ALIGN), ("b", P + 8, E_ALIGN), ("ab", P + 4, E_ALIGN)])
    # srk_add_bf16_into_f32(a, b, n, stream)
    sweep(h.srk_add_bf16_into_f32, dict(a=P, b=P, n=64), [("a", None, E_NULL), ("b", None, E_NULL), ("n", 0, E_SHAPE), ("n", 2, E_SHAPE),
                                                          ("a", P + 8, E_ALIGN), ("b", P + 2, E_ALIGN), ("b", P + 4, E_ALIGN)])
    # srk_add_f32(out, a, b, n, stream)
    sweep(h.srk_add_f32, dict(out=P, a=P, b=P, n=64), [("out", None, E_NULL), ("a", None, E_NULL), ("b", None, E_NULL), ("n", -64, E_SHAPE),
                                                       ("n", 65, E_SHAPE), ("out", P + 4, E_ALIGN), ("a", P + 8, E_ALIGN), ("b", P + 12, E_ALIGN)])
    # srk_rowscale_bf16(src, dst, f, rows, rows_per_sample, CP, stream)
    sweep(h.srk_rowscale_bf16, dict(src=P, dst=P, f=P, rows=100, rps=50, CP=64),
          [("src", None, E_NULL), ("dst", None, E_NULL), ("f", None, E_NULL), ("rows", 0, E_SHAPE), ("rps", 0, E_SHAPE), ("CP", 0, E_SHAPE),
           ("CP", 62, E_SHAPE), ("CP", -64, E_SHAPE), ("src", P + 2, E_ALIGN), ("dst", P + 4, E_ALIGN)])


def test_gate_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """HAT's CAB tail (srk_channel_gate / _act, srk_cab_add_ln, srk_cab_bwd) and DAT's small functions (srk_channel_interaction_fwd / _bwd,
    their frozen forms, srk_chan_attn_matrix_fwd / _bwd) return on the host, before any launch: SRK_E_NULL, SRK_E_SHAPE, SRK_E_UNSUPPORTED
    and SRK_E_ALIGN as include/srk.h states them at each entry point.  The addresses are dummies that are never dereferenced; every call
    differs from a valid one in exactly the argument under test."""
    h = lib.lib()
    P = 4096
    E_SHAPE, E_NULL, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -5

    def sweep(fn, base, changes, tail=(None,)):
        for name, bad, code in changes:
            assert name in base, name
            args = [bad if k == name else v for k, v in base.items()]
            rc = fn(*args, *tail)
            assert rc == code, (fn.__name__, name, bad, rc, code, h.srk_last_error())
            assert h.srk_last_error(), "no message"

    def nulls(base, but=()):
        return [(k, None, E_NULL) for k, v in base.items() if v == P and k not in but]

    gate_shape = [("S", 65, E_SHAPE), ("S", 0, E_SHAPE), ("C", 65, E_SHAPE), ("C", 0, E_SHAPE), ("CP", 96, E_SHAPE), ("CP", 320, E_SHAPE),
                  ("B", 65536, E_SHAPE), ("B", 0, E_SHAPE), ("HW", 0, E_SHAPE)]
    # srk_channel_gate(x, workspace, w1, b1, w2, b2, out_scale, gate, B, HW, C, CP, S, stream)  /  srk_channel_gate_act(..., S, act, stream)
    base = dict(x=P, workspace=P, w1=P, b1=P, w2=P, b2=P, out_scale=0.01, gate=P, B=3, HW=700, C=60, CP=64, S=6)
    faults = nulls(base) + gate_shape + [("x", P + 2, E_ALIGN), ("x", P + 8, E_ALIGN)]
    sweep(h.srk_channel_gate, base, faults)
    sweep(h.srk_channel_gate_act, dict(base, act=1), faults)

    # srk_cab_add_ln(x, conv, gate, gamma, beta, xn, rows, rows_per_sample, C, CP, stream)
    base = dict(x=P, conv=P, gate=P, gamma=P, beta=P, xn=P, rows=21, rps=7, C=60, CP=64)
    sweep(h.srk_cab_add_ln, base, [("x", None, E_NULL), ("conv", None, E_NULL), ("gate", None, E_NULL), ("gamma", None, E_NULL),
                                   ("beta", None, E_NULL), ("rows", 0, E_SHAPE), ("rows", 22, E_SHAPE), ("rps", 0, E_SHAPE), ("rps", 4, E_SHAPE),
                                   ("C", 65, E_SHAPE), ("C", 0, E_SHAPE), ("CP", 320, E_UNSUPPORTED), ("CP", 96, E_UNSUPPORTED),
                                   ("x", P + 4, E_ALIGN), ("x", P + 8, E_ALIGN), ("gate", P + 8, E_ALIGN), ("conv", P + 2, E_ALIGN),
                                   ("conv", P + 4, E_ALIGN), ("xn", P + 2, E_ALIGN), ("xn", P + 12, E_ALIGN)])
    assert h.srk_cab_add_ln(P, P, P, None, None, P, 21, 7, 60, 64, None) == E_NULL                       # xn without gamma / beta
    assert h.srk_cab_add_ln(P, P, P, None, None, None, 21, 7, 60, 320, None) == E_UNSUPPORTED            # the xn == null form reaches the CP switch

    # srk_cab_bwd(conv, g, gate, workspace, w1, b1, w2, b2, out_scale, dw1, db1, dw2, db2, dmean, d_conv, B, HW, C, CP, S, stream)
    base = dict(conv=P, g=P, gate=P, workspace=P, w1=P, b1=P, w2=P, b2=P, out_scale=0.01, dw1=P, db1=P, dw2=P, db2=P, dmean=P, d_conv=P,
                B=3, HW=700, C=60, CP=64, S=6)
    sweep(h.srk_cab_bwd, base, nulls(base) + gate_shape + [("conv", P + 8, E_ALIGN), ("conv", P + 2, E_ALIGN), ("g", P + 4, E_ALIGN),
                                                           ("gate", P + 8, E_ALIGN), ("dmean", P + 4, E_ALIGN), ("d_conv", P + 2, E_ALIGN),
                                                           ("d_conv", P + 4, E_ALIGN)])

    # the largest covered batch at C 180, S 22 and the first refused one (tests/gate_ref.py restates the LDS formula)
    import gate_ref
    bmax = gate_ref.ci_largest_B(180, 22)
    assert h.srk_channel_interaction_covered(bmax, 180, 22) == 1 and h.srk_channel_interaction_covered(bmax + 1, 180, 22) == 0
    assert h.srk_channel_interaction_covered(1, 180, 22) == 0 and h.srk_channel_interaction_frozen_covered(1, 180, 22) == 1
    ci_shape = [("B", bmax + 1, E_SHAPE), ("B", 0, E_SHAPE), ("S", 65, E_SHAPE), ("S", 0, E_SHAPE), ("C", 0, E_SHAPE), ("CA", 179, E_SHAPE)]
    # srk_channel_interaction_fwd(pooled, ldp, inv_hw, pad_of, W1, b1, gamma, beta, eps, W2, b2, running_mean, running_var, momentum, pm_out,
    #                             cgate, B, C, S, CA, stream)
    base = dict(pooled=P, ldp=192, inv_hw=0.01, pad_of=P, W1=P, b1=P, gamma=P, beta=P, eps=1e-5, W2=P, b2=P, running_mean=P, running_var=P,
                momentum=0.1, pm_out=P, cgate=P, B=4, C=180, S=22, CA=192)
    sweep(h.srk_channel_interaction_fwd, base, nulls(base, but=("running_mean", "running_var")) + ci_shape +
          [("ldp", 191, E_SHAPE), ("running_mean", None, E_SHAPE), ("running_var", None, E_SHAPE), ("B", 1, E_SHAPE)])
    # srk_channel_interaction_frozen_fwd(pooled, ..., b2, running_mean, running_var, pm_out, cgate, B, C, S, CA, stream)
    fbase = {k: v for k, v in base.items() if k != "momentum"}
    sweep(h.srk_channel_interaction_frozen_fwd, fbase, nulls(fbase) + ci_shape + [("ldp", 191, E_SHAPE)])
    # srk_channel_interaction_bwd(pm, dcgate, ldg, inv_hw, pad_of, W1, b1, gamma, beta, eps, W2, b2, dW1, db1, dgamma, dbeta, dW2, db2, dpool,
    #                             B, C, S, CA, stream)
    base = dict(pm=P, dcgate=P, ldg=192, inv_hw=0.01, pad_of=P, W1=P, b1=P, gamma=P, beta=P, eps=1e-5, W2=P, b2=P, dW1=P, db1=P, dgamma=P,
                dbeta=P, dW2=P, db2=P, dpool=P, B=4, C=180, S=22, CA=192)
    sweep(h.srk_channel_interaction_bwd, base, nulls(base) + ci_shape + [("ldg", 191, E_SHAPE), ("B", 1, E_SHAPE)])
    # srk_channel_interaction_frozen_bwd(pm, ..., b2, running_mean, running_var, dW1, ..., dpool, B, C, S, CA, stream)
    fbase = {}
    for k, v in base.items():
        fbase[k] = v
        if k == "b2":
            fbase["running_mean"], fbase["running_var"] = P, P
    sweep(h.srk_channel_interaction_frozen_bwd, fbase, nulls(fbase) + ci_shape + [("ldg", 191, E_SHAPE)])

    # srk_chan_attn_matrix_fwd(partial, nchunk, temperature, gram, A, B, num_heads, dh, stream)
    mat_shape = [("B", 0, E_SHAPE), ("nH", 0, E_SHAPE), ("nchunk", 0, E_SHAPE), ("dh", 0, E_SHAPE), ("dh", 33, E_SHAPE)]
    base = dict(partial=P, nchunk=3, temperature=P, gram=P, A=P, B=2, nH=6, dh=30)
    sweep(h.srk_chan_attn_matrix_fwd, base, nulls(base) + mat_shape)
    # srk_chan_attn_matrix_bwd(dpartial, nchunk, gram, A, temperature, dG, dGt, dsq2, dsk2, dtemp, B, num_heads, dh, stream)
    base = dict(dpartial=P, nchunk=3, gram=P, A=P, temperature=P, dG=P, dGt=P, dsq2=P, dsk2=P, dtemp=P, B=2, nH=6, dh=30)
    sweep(h.srk_chan_attn_matrix_bwd, base, nulls(base) + mat_shape)


def test_swin_block_entry_refuses_bad_arguments_without_a_gpu(lib):
    """srk_swin_block_fwd (the whole-block kernel of the SwinIR-light width) returns on the host, before any launch: SRK_E_NULL,
    SRK_E_SHAPE, SRK_E_ALIGN (its kernel issues 16-byte accesses on x, y, every weight, every bias and bias_dense, 8-byte stores on
    y_bf16) and SRK_E_UNSUPPORTED as include/srk.h states them.  The addresses are dummies that are never dereferenced; every call differs
    from a valid one in exactly the argument under test."""
    h = lib.lib()
    P = 4096
    E_SHAPE, E_NULL, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -5
    # srk_swin_block_fwd(x, y, y_bf16, norm1_w, norm1_b, norm2_w, norm2_b, wqkv, bqkv, wproj, bproj, w1, b1, w2, b2, bias_dense, scale,
    #                    C, num_heads, head_dim, hidden, B, H, W, shift, stream)
    base = dict(x=P, y=P, y_bf16=P, n1w=P, n1b=P, n2w=P, n2b=P, wqkv=P, bqkv=P, wproj=P, bproj=P, w1=P, b1=P, w2=P, b2=P, dense=P, scale=0.3,
                C=60, nH=6, dh=10, hid=120, B=2, H=16, W=24, shift=4)
    optional = ("y_bf16", "bqkv", "bproj", "b1", "b2")
    changes = [(k, None, E_NULL) for k, v in base.items() if v == P and k not in optional]
    changes += [("B", 0, E_SHAPE), ("H", 0, E_SHAPE), ("H", 12, E_SHAPE), ("W", 20, E_SHAPE), ("W", -8, E_SHAPE), ("shift", 2, E_SHAPE),
                ("shift", -4, E_SHAPE), ("dh", 9, E_SHAPE), ("nH", 5, E_SHAPE), ("hid", 129, E_SHAPE), ("hid", 0, E_SHAPE), ("C", 68, E_SHAPE),
                ("C", 0, E_SHAPE)]
    for k in ("x", "y", "wqkv", "bqkv", "wproj", "bproj", "w1", "b1", "w2", "b2", "dense"):
        changes += [(k, P + 4, E_ALIGN), (k, P + 8, E_ALIGN)]
    changes += [("y_bf16", P + 2, E_ALIGN), ("y_bf16", P + 4, E_ALIGN), ("y_bf16", P + 12, E_ALIGN)]
    for name, bad, code in changes:
        rc = h.srk_swin_block_fwd(*[bad if k == name else v for k, v in base.items()], None)
        assert rc == code, (name, bad, rc, code, h.srk_last_error())
        assert h.srk_last_error(), "no message"
    # widths without a whole-block kernel: 4 heads x 16, 3 heads x 20
    for C_, nH, dh in ((64, 4, 16), (60, 3, 20)):
        assert h.srk_swin_block_fwd(*dict(base, C=C_, nH=nH, dh=dh).values(), None) == E_UNSUPPORTED
        assert b"light width" in h.srk_last_error()
    # the option that switches the kernel off: the message names it
    lib.check(h.srk_set_option(b"block_light", 0))
    try:
        assert h.srk_swin_block_fwd(*base.values(), None) == E_UNSUPPORTED
        assert b"block_light" in h.srk_last_error()
    finally:
        lib.check(h.srk_set_option(b"block_light", 1))


def test_options_are_process_wide_with_per_plan_values():
    """SURVEY 8b 're-entrant': srk_set_option writes ONE process-wide value per option (every thread sees it -- the autograd engine runs
    the backward on its own thread); a plan carries its own values (srk_swinir_plan_set_option), applied in a thread-private copy of the
    option set around each of its calls, which leaves the process-wide values as they were.  Host-only: no kernel runs."""
    import ctypes as C
    import threading
    from tpu_superresolution_amd import _lib
    from tpu_superresolution_amd._lib import check, lib
    from tpu_superresolution_amd.engine import SwinIRPlan
    L = lib()

    def get(name):
        v = C.c_int()
        check(L.srk_get_option(name.encode(), C.byref(v)))
        return v.value

    base = get("attn_fused")
    assert base == 2 and get("mlp_fused") == 1 and get("wgrad_stream_rows") == 32
    seen = {}

    def other():
        seen["before"] = get("attn_fused")
        check(L.srk_set_option(b"attn_fused", 0))
        seen["other"] = get("attn_fused")
    check(L.srk_set_option(b"attn_fused", 1))
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["before"] == 1 and seen["other"] == 0 and get("attn_fused") == 0      # one value, whichever thread wrote it
    check(L.srk_set_option(b"attn_fused", base))
    plan = SwinIRPlan(img_size=16, in_chans=3, embed_dim=24, depths=(2,), num_heads=(2,), window_size=8, mlp_ratio=2, upscale=2, img_range=1.0,
                      upsampler="pixelshuffle", options={"attn_fused": 1, "gemm_stream_bm": 32})
    assert plan.get_option("attn_fused") == (1, True) and plan.get_option("gemm_stream_bm") == (32, True)
    assert plan.get_option("mlp_fused") == (1, False)
    assert get("attn_fused") == base and get("gemm_stream_bm") == 0        # setting a plan's option does not touch the process-wide value
    n0 = L.srk_swinir_workspace_bytes(plan.handle, 2, 16, 16, 1)            # a plan call applies and restores
    assert n0 > 0 and get("attn_fused") == base and get("gemm_stream_bm") == 0
    with pytest.raises(Exception, match="gemm_stream_bm"):
        plan.set_option("gemm_stream_bm", 7)
    with pytest.raises(_lib.SrkUnsupported, match="unknown option"):
        plan.set_option("no_such_option", 1)
    assert plan.get_option("gemm_stream_bm") == (32, True)


def test_batched_weight_packing_equals_one_tensor_at_a_time():
    """packing.batched_pack: the packed (bf16 / padded / permuted / transposed) weights of HAT, DAT (inference and training subsets) and
    SwinIR (window 16 forward, window 7 transposed) built by one stack + scatter + cast per weight kind are bit-identical to the
    tensor-by-tensor pack (pure torch: runs on the CPU)."""
    import torch
    import tpu_superresolution_amd as T
    from tpu_superresolution_amd import dat_train, hat_train, packing, swinir_small_train, swinir_w16

    class Eager:                      # a context whose helpers run eagerly (no active packer)
        def __enter__(self):
            class R:
                def resolve(self, P):
                    pass
            return R()

        def __exit__(self, *a):
            pass

    def both(fn):
        a = fn()
        real = packing.batched_pack
        packing.batched_pack = Eager
        try:
            b = fn()
        finally:
            packing.batched_pack = real
        assert a.keys() == b.keys()
        for k in a:
            assert isinstance(a[k], torch.Tensor), (k, type(a[k]))
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) and a[k].is_contiguous(), k
        return len(a)

    dev = torch.device("cpu")
    torch.manual_seed(0)
    m = T.HAT(upscale=2, in_chans=3, img_size=32, window_size=16, compress_ratio=3, squeeze_factor=6, conv_scale=0.01, overlap_ratio=0.5,
              img_range=1.0, depths=[2, 2], embed_dim=24, num_heads=[2, 2], mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")
    d = T.DAT(img_size=32, in_chans=3, embed_dim=48, split_size=[8, 32], depth=[3, 2], num_heads=[4, 4], expansion_factor=2.0, upscale=2, img_range=1.0)
    s = T.SwinIR(img_size=32, in_chans=3, embed_dim=24, depths=(2, 2), num_heads=(2, 2), window_size=16, mlp_ratio=2, img_range=1.0, upscale=2,
                 upsampler="pixelshuffle")
    s7 = T.SwinIR(img_size=28, in_chans=3, embed_dim=24, depths=(2, 2), num_heads=(2, 2), window_size=7, mlp_ratio=2, img_range=1.0, upscale=2,
                  upsampler="pixelshuffle")

    def hat_p():
        packing.drop_packs(m)
        return dict(m._pack(dev))

    def hat_pt():
        packing.drop_packs(m)
        return dict(hat_train.pack_transposed(m, dev))

    def dat_p(train):
        def f():
            packing.drop_packs(d)
            return dict(d._pack(dev, train))
        return f

    def dat_pt():
        packing.drop_packs(d)
        return dict(dat_train.pack_train(d, dev))

    def w16_p():
        packing.drop_packs(s)
        return dict(swinir_w16.pack(s, dev))

    def ws_pt():
        packing.drop_packs(s7)
        return dict(swinir_small_train.pack_transposed(s7, dev))

    assert both(hat_p) == 93 and both(hat_pt) == 37 and both(dat_p(False)) == 131 and both(dat_p(True)) == 73 and both(dat_pt) == 58
    assert both(w16_p) == 45 and both(ws_pt) == 21


def test_zero_arena_serves_the_second_pass_from_one_buffer():
    """ops.ZeroArena: the first pass learns the size (torch.zeros fallbacks), the following passes carve every request out of one zeroed
    buffer (256-byte aligned pieces, independent of each other), a larger pass than learnt falls back for the excess, and outside an
    arena_scope zeros_f32 is plain torch.zeros."""
    import torch
    from tpu_superresolution_amd import ops
    dev = torch.device("cpu")
    ar = ops.ZeroArena()
    shapes = [(3, 5), (7,), (2, 2, 9), (64,)]
    with ops.arena_scope(ar, dev):
        first = [ops.zeros_f32(s, dev) for s in shapes]
    assert all(t.shape == torch.Size(s) and float(t.abs().sum()) == 0.0 for t, s in zip(first, shapes))
    assert ar.need == 4 * 64 and ar.buf is None
    with ops.arena_scope(ar, dev):
        second = [ops.zeros_f32(s, dev) for s in shapes]
        extra = ops.zeros_f32((100,), dev)                      # beyond what the first pass asked for
    base = ar.buf.data_ptr()
    assert [t.data_ptr() - base for t in second] == [0, 256, 512, 768]
    assert not (base <= extra.data_ptr() < base + ar.buf.numel() * 4)
    second[0].fill_(1.0)
    assert float(second[1].abs().sum()) == 0.0 and float(ar.buf[15:64].abs().sum()) == 0.0
    assert ar.need == 4 * 64 + 128
    kept = second[2]
    with ops.arena_scope(ar, dev):
        third = ops.zeros_f32((3, 5), dev)
    assert third.data_ptr() != second[0].data_ptr() or float(third.abs().sum()) == 0.0     # a fresh buffer per pass: `kept` is untouched
    assert float(kept.abs().sum()) == 0.0 and float(third.abs().sum()) == 0.0
    assert ops.zeros_f32((4,), dev).shape == (4,)


def test_grad_sink_hands_every_gradient_over_once_in_creation_order():
    """host_pass.GradSink: each segment_done() gives the hook the gradients made since the previous one, in the order they were put; every
    gradient is handed over exactly once, a segment with nothing new is an empty list, and finish() is forwarded once."""
    import torch
    import torch.nn as nn
    from tpu_superresolution_amd.host_pass import GradSink

    class Hook:
        def __init__(self):
            self.segments, self.finished = [], 0

        def segment_done(self, tensors):
            self.segments.append(list(tensors))

        def finish(self):
            self.finished += 1

    m = nn.Sequential(nn.Linear(4, 4), nn.LayerNorm(4))
    lin, ln = m[0], m[1]
    hook = Hook()
    sink = GradSink(m, hook, 0, torch.device("cpu"), 8, 4, 64, 8, None)
    g = {n: torch.full(p.shape, float(i)) for i, (n, p) in enumerate(m.named_parameters())}
    sink.put(lin.weight, g["0.weight"])
    sink.segment_done()
    sink.put(ln.bias, g["1.bias"])
    sink.put(lin.bias, g["0.bias"])
    sink.segment_done()
    sink.segment_done()                                  # nothing new
    sink.put(ln.weight, g["1.weight"])
    sink.segment_done()
    sink.finish()
    order = [["0.weight"], ["1.bias", "0.bias"], [], ["1.weight"]]
    assert len(hook.segments) == len(order)
    for seg, names in zip(hook.segments, order):
        assert len(seg) == len(names) and all(t is g[n] for t, n in zip(seg, names))
    handed = [id(t) for seg in hook.segments for t in seg]
    assert sorted(handed) == sorted(id(t) for t in g.values())          # each exactly once
    assert list(sink.G) == ["0.weight", "1.bias", "0.bias", "1.weight"] and all(sink.G[n] is g[n] for n in g)
    assert hook.finished == 1
    quiet = GradSink(m, None, 0, torch.device("cpu"), 8, 4, 64, 8, None)      # without a hook both calls are no-ops
    quiet.put(lin.weight, g["0.weight"])
    quiet.segment_done()
    quiet.finish()
    assert list(quiet.G) == ["0.weight"]


def test_unpack_inverts_pack_for_linear_and_conv_weights():
    """host_pass._unpack_linear / _unpack_conv give back what packing._pack_linear / _pack_conv packed -- plain, through the head / qkv /
    PixelShuffle index maps and transposed, at a width that is no multiple of 64 (C = 24, 2 heads, r = 3); integer-valued weights, so the
    bf16 packed copy is exact and the comparison is torch.equal."""
    import torch
    from tpu_superresolution_amd import packing as ha
    from tpu_superresolution_amd.host_pass import _unpack_conv, _unpack_linear
    dev = torch.device("cpu")
    gen = torch.Generator().manual_seed(0)

    def ints(*shape):
        return torch.randint(-8, 9, shape, generator=gen).float()

    C_, nH, r = 24, 2, 3
    dh, CA, CP, HP = C_ // nH, nH * 32, 64, 64
    hm, qkv_rows, pm = ha._head_map(nH, dh, dev), ha._qkv_rows(nH, dh, dev), ha._ps_map(r * r * 64, r, 64, dev)
    wqkv, wproj, wfc1 = ints(3 * C_, C_), ints(C_, C_), ints(2 * C_, C_)
    linear_cases = [(wfc1, HP, CP, None, None),                      # plain padding
                    (wqkv, 3 * CA, CP, qkv_rows, None),              # rows through the qkv map
                    (wproj, CP, CA, None, hm),                       # columns through the head map
                    (wqkv.t(), CP, 3 * CA, None, qkv_rows),          # the dgrads' transposed copies
                    (wproj.t(), CA, CP, hm, None)]
    for w, NP, KP, row_map, col_map in linear_cases:
        packed = ha._pack_linear(w, NP, KP, row_map=row_map, col_map=col_map)
        assert packed.shape == (NP, KP) and packed.dtype == torch.bfloat16
        back = _unpack_linear(packed.float(), w.shape[0], w.shape[1], row_map, col_map)
        assert back.is_contiguous() and torch.equal(back, w.contiguous())
    wbody, wup = ints(C_, C_, 3, 3), ints(r * r * 64, 64, 3, 3)
    for w, NP, CinP, row_map in [(wbody, CP, CP, None), (wup, r * r * 64, 64, pm)]:
        packed = ha._pack_conv(w, NP, CinP, row_map=row_map)
        assert packed.shape == (NP, 9 * CinP) and packed.dtype == torch.bfloat16
        back = _unpack_conv(packed.float(), w.shape[0], w.shape[1], CinP, row_map)
        assert back.is_contiguous() and torch.equal(back, w)
