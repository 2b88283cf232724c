"""CPU checks behind the wide one-step head's backward (tests/wide_head_ref.py, tests/test_gpu_wide_head_train.py):

  * the fp64 restatement the GPU test compares with (wgrad_ref.reference at CoP 32 / 48 / 64) is torch.nn.functional.conv2d under
    autograd, for every case, and the exact classes are what they claim (integers that fp32 / bf16 hold);
  * the comparator rejects every negative control: a dropped tap, a transposed (co, ci), a dropped lo half, a pad column of gy that
    leaks, a halo read one pixel off;
  * the CPU oracle under autograd reproduces the reference's train-mode loss and gradients of fixture G21 (27 / 48 / 64 head channels);
  * the C ABI: the three entry points are declared and exported and refuse, on the host, what their kernels cannot honour; the plan
    option is known and unknown names are still refused.
No GPU is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_ref as R
import wide_head_ref as WH
from oracle import swinir_oracle as O

CONV_CASES = [c for c in WH.CASES if c.kind in ("smallw", "smalld")]
PREP_CASES = [c for c in WH.CASES if c.kind == "imgprep"]


def test_case_ids_are_unique_and_cover_the_matrix():
    ids = [c.id for c in WH.CASES]
    assert len(set(ids)) == len(ids)
    for kind in ("smallw", "smalld"):
        for h in WH.HEADS:
            geos = {c.geo for c in CONV_CASES if c.kind == kind and (c.Cin, c.CinP, c.Co, c.CoP) == h and c.cls == "exact"}
            assert set(WH.GEO[:4]) <= geos, (kind, h)
            assert {c.cls for c in CONV_CASES if c.kind == kind and (c.Cin, c.CinP, c.Co, c.CoP) == h} == {"exact", "dyadic", "random"}
    assert all(c.CoP in (32, 48, 64) for c in WH.CASES)


@pytest.mark.parametrize("c", CONV_CASES, ids=lambda c: c.id)
def test_reference_is_autograd_of_conv2d_and_the_exact_class_is_exact(c):
    inp = WH.make_inputs(c)
    ref = WH.reference(c, inp)
    auto = WH.autograd_reference(c, inp)
    assert set(ref) == set(auto)
    for k in ref:
        scale = float(ref[k].abs().max()) + 1.0
        assert float((ref[k] - auto[k]).abs().max()) <= 1e-11 * scale, k
    if c.kind == "smalld":
        assert bool((ref["dx"][:, c.Cin:] == 0).all())
        assert bool((inp["gy"][:, c.Co:] != 0).all()), "the pad columns of gy carry values"
    if c.cls == "exact":
        for k, v in ref.items():
            assert torch.equal(v, v.round()) and float(v.abs().max()) < 2 ** 24, k
        if c.kind == "smalld":
            assert float(ref["dx"].abs().max()) <= 256 and torch.equal(ref["dx"].to(torch.bfloat16).double(), ref["dx"])
            w = inp["weight"]
            assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and bool((w != 0).reshape(c.Co, c.Cin, 9).any(1).all())


@pytest.mark.parametrize("c", PREP_CASES, ids=lambda c: c.id)
def test_prep_cases_are_accepted_by_the_reference(c):
    inp = WH.make_inputs(c)
    ref = WH.reference(c, inp)["gy"]
    n = c.Cimg * c.r * c.r
    assert n <= c.CoP and bool((ref[:, n:] == 0).all()) and float(ref[:, :n].abs().max()) > 0
    assert torch.equal(ref.float().double(), ref)               # one fp32 multiply: the reference is an fp32 value


@pytest.mark.parametrize("c", CONV_CASES, ids=lambda c: c.id)
def test_every_negative_control_fails_the_comparator(c):
    inp = WH.make_inputs(c)
    exp = WH.expected(c, inp)
    good = {k: o.rounded() for k, o in exp.items()}
    ok, ratios = WH.accepts(c, good, exp)
    assert ok, ratios
    for name in WH.controls_for(c):
        wrong = WH.autograd_reference(c, inp, name)
        wrong = {k: v.to(torch.bfloat16 if k == "dx" else torch.float32) for k, v in wrong.items()}
        ok, ratios = WH.accepts(c, wrong, exp)
        assert not ok, f"{name}: a wrong result was accepted: {ratios}"


def test_split_term_of_the_tolerance_is_zero_for_the_fp32_mfma():
    """N_SPLIT = 0: the bound is wgrad_ref's without its hi + lo terms, so it is never wider than the narrow family's."""
    assert WH.N_SPLIT == 0
    c = next(c for c in CONV_CASES if c.cls == "random" and c.kind == "smallw")
    inp = WH.make_inputs(c)
    mine, theirs = WH.tolerance(c, inp), R.tolerance(c, inp)
    for k in mine:
        assert bool((mine[k] <= theirs[k]).all()) and bool((mine[k] > 0).all())


# ---- G21 --------------------------------------------------------------------------------------------------------------------------
# fp64 oracle against the reference's fp32 run: the same function in exact arithmetic, so the difference is the reference's own fp32
# rounding.  An element of the widest gradient sum (a conv weight) adds N = 512 pixels x 9 taps x 64 channels = 3e5 terms through
# the chain; rounding errors of u = 2^-24 per addition accumulate like a random walk, sqrt(N) u = 3.3e-5 of the sum S of the absolute
# terms, and S / |sum| (cancellation) is taken as 3: 1e-4 relative L2 per tensor.  That is three orders below the GPU test's 0.1; a
# wrong formula (a missing tap, a transposed head) is a relative error of order 1.  The loss is one mean of <= 2e4 terms: 1e-5.
G21_REL_L2 = 1e-4
G21_LOSS_REL = 1e-5


@pytest.mark.parametrize("tag", WH.G21_TAGS)
@pytest.mark.parametrize("hw", WH.G21_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_oracle_autograd_reproduces_the_reference_train_gradients(tag, hw):
    g, cfg, sd = WH.g21_checked_weights(tag)
    key = f"{tag}.{hw[0]}x{hw[1]}"
    x, t = torch.from_numpy(g[f"{key}.x"]), torch.from_numpy(g[f"{key}.target"])
    assert torch.equal(x, WH.g21_input(tag, hw)) and torch.equal(t, WH.g21_target(tag, hw))
    assert cfg.upscale ** 2 * cfg.in_chans == {"psd3": 27, "psd4": 48, "psd8g": 64}[tag]
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    loss = torch.nn.functional.l1_loss(O.swinir_forward(sd64, cfg, x.double()), t.double())
    loss.backward()
    assert abs(float(loss.detach()) - float(g[f"{key}.loss"])) <= G21_LOSS_REL * float(g[f"{key}.loss"])
    names = [k[len(key) + 6:] for k in g.files if k.startswith(key + ".grad.")]
    assert set(names) == set(O.param_keys(cfg)) and "upsample.0.weight" in names
    worst = ("", 0.0)
    for n in names:
        ref = torch.from_numpy(g[f"{key}.grad.{n}"]).double()
        assert sd64[n].grad is not None and sd64[n].grad.shape == ref.shape, n
        rel = float((sd64[n].grad - ref).norm() / (ref.norm() + 1e-30))
        worst = max(worst, (n, rel), key=lambda p: p[1])
        assert rel <= G21_REL_L2, f"{n}: relative L2 {rel:.3e}"
    print(f"[g21] {key}: loss {float(loss.detach()):.6f}, worst tensor {worst[0]} rel L2 {worst[1]:.3e}")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tpu_superresolution_amd import build
    build.build(verbose=False)
    from tpu_superresolution_amd import _lib
    return _lib


def test_wide_head_entry_points_are_declared_and_exported(lib):
    names = lib.declared_symbols()
    for n in ("srk_widehead_grad_prep", "srk_widehead_wgrad", "srk_widehead_dgrad"):
        assert n in names and n in lib._SIGNATURES and hasattr(lib.lib(), n), n


def test_wide_head_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """Every call differs from a valid one in exactly the argument under test and returns on the host; the addresses are dummies."""
    h = lib.lib()
    P = 4096
    E_SHAPE, E_NULL, E_ALIGN = -1, -2, -5
    BIG = 0x7fffffff

    def refused(rc, code, what):
        assert rc == code, (what, rc, code, h.srk_last_error())
        assert h.srk_last_error(), "no message"

    def variants(base, changes):
        for name, bad, code in changes:
            yield [bad if k == name else v for k, v in base.items()], code, (name, bad)

    base = dict(d_pred=P, gy=P, B=2, Cimg=3, Hc=16, Wc=32, H=4, W=8, r=4, CoP=48, inv_range=1.0)
    for a, code, what in variants(base, [("d_pred", None, E_NULL), ("gy", None, E_NULL), ("gy", P + 4, E_ALIGN), ("B", 0, E_SHAPE), ("H", 0, E_SHAPE),
                                         ("W", -1, E_SHAPE), ("r", 0, E_SHAPE), ("r", 5, E_SHAPE), ("r", 9, E_SHAPE), ("r", BIG, E_SHAPE),
                                         ("Cimg", 0, E_SHAPE), ("Cimg", 4, E_SHAPE), ("Cimg", BIG, E_SHAPE), ("CoP", 16, E_SHAPE),
                                         ("CoP", 4, E_SHAPE), ("CoP", 40, E_SHAPE), ("CoP", 80, E_SHAPE), ("CoP", 0, E_SHAPE), ("Hc", 17, E_SHAPE),
                                         ("Wc", 33, E_SHAPE), ("Hc", 0, E_SHAPE), ("Wc", -2, E_SHAPE), ("B", BIG, E_SHAPE), ("H", BIG, E_SHAPE)]):
        refused(h.srk_widehead_grad_prep(*a, None), code, what)

    shape_faults = [("B", 0, E_SHAPE), ("H", 0, E_SHAPE), ("W", -3, E_SHAPE), ("B", BIG, E_SHAPE), ("Co", 49, E_SHAPE), ("Co", 0, E_SHAPE),
                    ("CoP", 16, E_SHAPE), ("CoP", 4, E_SHAPE), ("CoP", 56, E_SHAPE), ("CoP", 128, E_SHAPE), ("Cin", 65, E_SHAPE), ("Cin", 0, E_SHAPE),
                    ("CinP", 60, E_SHAPE), ("CinP", 320, E_SHAPE), ("CinP", 0, E_SHAPE)]
    base = dict(x=P, gy=P, dw=P, db=P, B=1, H=4, W=8, Cin=60, CinP=64, Co=48, CoP=48)
    for a, code, what in variants(base, shape_faults + [("x", None, E_NULL), ("gy", None, E_NULL), ("dw", None, E_NULL), ("db", None, E_NULL),
                                                        ("x", P + 2, E_ALIGN), ("gy", P + 4, E_ALIGN)]):
        refused(h.srk_widehead_wgrad(*a, None), code, what)
    base = dict(gy=P, weight=P, dx=P, B=1, H=4, W=8, Cin=60, CinP=64, Co=48, CoP=48)
    for a, code, what in variants(base, shape_faults + [("gy", None, E_NULL), ("weight", None, E_NULL), ("dx", None, E_NULL), ("gy", P + 4, E_ALIGN),
                                                        ("dx", P + 8, E_ALIGN)]):
        refused(h.srk_widehead_dgrad(*a, None), code, what)
    # the narrow entry points keep their contract
    refused(h.srk_smallconv_dgrad(P, P, P, 1, 4, 8, 60, 64, 12, 32, None), E_SHAPE, "narrow dgrad at CoP 32")
    refused(h.srk_img_grad_prep(P, P, 2, 3, 16, 32, 4, 8, 4, 48, 1.0, None), E_SHAPE, "narrow prep at CoP 48")


def test_wide_head_option_is_known_and_unknown_names_are_refused(lib):
    from tpu_superresolution_amd.engine import SwinIRPlan
    h = lib.lib()
    v = C.c_int(-1)
    assert h.srk_get_option(b"wide_head_train", C.byref(v)) == 0 and v.value == 0          # default off
    assert h.srk_get_option(b"wide_head_trains", C.byref(v)) == -3 and h.srk_set_option(b"wide_head", 1) == -3
    cfg = O.SwinIRConfig(img_size=16, in_chans=3, embed_dim=24, depths=(2,), num_heads=(2,), window_size=8, mlp_ratio=2, upscale=4,
                         img_range=1.0, upsampler="pixelshuffledirect", resi_connection="1conv")
    kw = dict(img_size=cfg.img_size, in_chans=cfg.in_chans, embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
              window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio, upscale=cfg.upscale, img_range=cfg.img_range, upsampler=cfg.upsampler)
    off, on = SwinIRPlan(**kw), SwinIRPlan(**kw, options={"wide_head_train": 1})
    assert on.get_option("wide_head_train") == (1, True) and off.get_option("wide_head_train") == (0, False)
    assert h.srk_get_option(b"wide_head_train", C.byref(v)) == 0 and v.value == 0          # a plan's value is the plan's own
    with pytest.raises(Exception):
        off.set_option("wide_head_training", 1)
    # the option widens gyimg: 48 instead of 16 fp32 columns per token of the padded 16 x 16 grid
    b_off = h.srk_swinir_workspace_bytes(off.handle, 2, 11, 13, 1)
    b_on = h.srk_swinir_workspace_bytes(on.handle, 2, 11, 13, 1)
    assert b_on - b_off == 2 * 16 * 16 * (48 - 16) * 4
    assert h.srk_swinir_workspace_bytes(on.handle, 2, 11, 13, 0) == h.srk_swinir_workspace_bytes(off.handle, 2, 11, 13, 0)
