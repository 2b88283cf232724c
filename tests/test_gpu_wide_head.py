"""The engine's one-step upsample head ('pixelshuffledirect') with 16 < upscale^2 * in_chans <= 64, and the scales the command lines
did not reach (x3, x8), on the device.

Whole model: the tiny G20 fixtures of the reference (tools/make_golden_scales.py) through the HIP path at the project's whole-model
tolerance, 1.2e-2 * max|ref| ('1conv' SwinIR: tests/test_gpu_model.py; HAT: tests/test_gpu_hat.py; DAT: tests/test_gpu_dat.py).

The head alone: a light-width SwinIR (embed 60, one RSTB of two blocks).  The head's input is read back from the engine's workspace
(buffer 'fb': bf16 [T][64]) and conv + bias + pixel shuffle + / range + mean is computed from it in fp64.  The operands are exact bf16
values on both sides, so the tolerance is the derived one of tests/gemm_ex_ref.py -- 2 K u S for the fp32 accumulation in any order, plus
2 u |ref| for the epilogue's roundings, u = 2^-24, K = 9 * 64, S the absolute terms of the sum -- per output element, no tuned constant.
"""
import numpy as np
import pytest
import torch

import golden_scales as GS
import wide_head_case as W
from conftest import load_golden
from gemm_ex_ref import Tol
from guarded import Guarded

pytestmark = pytest.mark.gpu


# ---- whole model ------------------------------------------------------------------------------------------------------------------------------
def _build(tag, cfg, sd):
    import tpu_superresolution_amd as T
    family = GS.CASES[tag][0]
    if family == "swinir":
        m = T.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
    else:
        m = {"hat": T.HAT, "dat": T.DAT}[family](**cfg.kwargs())
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m.cuda().eval()


@pytest.mark.parametrize("tag", list(GS.CASES))
def test_g20_forward_vs_reference_golden(tag):
    g, cfg, sd = GS.checked_weights(tag)
    m = _build(tag, cfg, sd)
    for hw in GS.SIZES:          # an exact multiple of the window / reflect-pad + crop (DAT: padded inside its attention)
        x = torch.from_numpy(g[f"{tag}.x_{hw[0]}x{hw[1]}"])
        with torch.no_grad():
            y = m(x.cuda()).cpu()
        ref = torch.from_numpy(g[f"{tag}.y_{hw[0]}x{hw[1]}"])
        assert y.shape == ref.shape and y.dtype == torch.float32
        err = float((y - ref).abs().max())
        print(f"G20 {tag} {hw}: max err {err:.3e} ({err / float(ref.abs().max()):.2e} of range)")
        assert err <= 1.2e-2 * float(ref.abs().max()), f"{tag} {hw}: max err {err:.3e} vs ref max {float(ref.abs().max()):.3e}"


# ---- the head alone ---------------------------------------------------------------------------------------------------------------------------
def _forward_into(m, x, out_ptr):
    """srk_swinir_forward of the bound engine with the output at out_ptr (engine.forward with the caller's buffer)"""
    from tpu_superresolution_amd._lib import check, lib
    from tpu_superresolution_amd.engine import _stream
    eng = m._engine
    B, _, H, Wd = x.shape
    ws = eng._workspace(B, H, Wd, False)
    with torch.cuda.device(eng.device):
        check(lib().srk_swinir_forward(eng.plan.handle, eng.flat.data_ptr(), eng.packed.data_ptr(), x.data_ptr(), out_ptr, ws.data_ptr(), B, H, Wd, 0,
                                       None, _stream(eng.device)))


def _head_reference(m, s, c, B, H0, W0):
    """fp64 conv + bias + shuffle + / range + mean of the workspace's 'fb', cropped -> (ref, tol) [B][c][H0 s][W0 s]"""
    Hp, Wp = (H0 + 7) // 8 * 8, (W0 + 7) // 8 * 8
    fb = m._engine.activation("fb", torch.bfloat16).view(B, Hp, Wp, 64).double().cpu()
    assert float(fb[..., 60:].abs().max()) == 0.0          # the pad columns of the 60-channel rows
    a = fb[..., :60].permute(0, 3, 1, 2).contiguous()
    w, b = m.upsample[0].weight.detach().double().cpu(), m.upsample[0].bias.detach().double().cpu()
    assert torch.equal(w.to(torch.bfloat16).double(), w) and torch.equal(b.to(torch.bfloat16).double(), b)
    conv = torch.nn.functional.conv2d
    v = conv(a, w, b, padding=1)
    S = conv(a.abs(), w.abs(), b.abs(), padding=1)
    inv = float(np.float32(1.0) / np.float32(W.IMG_RANGE))
    mean = torch.tensor([float(np.float32(t)) for t in ((0.4488, 0.4371, 0.4040) if c == 3 else (0.0,))], dtype=torch.float64).view(1, c, 1, 1)
    shuffle = lambda t: torch.nn.functional.pixel_shuffle(t, s)[:, :, :H0 * s, :W0 * s]
    ref = shuffle(v) * inv + mean
    S = shuffle(S) * inv + mean.abs()
    return ref, Tol.f32(ref, Tol.delta(9 * 64, S))


def _run(s, c, hw):
    """-> (model, y of the guarded direct call, y of model.forward)"""
    m = W.model(s, c)
    x = W.image(c, hw).cuda()
    with torch.no_grad():
        y_mod = m(x)          # binds the engine, packs, sizes the workspace
        out = Guarded("f32", W.BATCH * c * hw[0] * s, hw[1] * s, hw[1] * s)
        _forward_into(m, x, out.ptr)
        torch.cuda.synchronize()
    out.assert_guards(f"head s={s} c={c} {hw}")
    return m, out.data().view(W.BATCH, c, hw[0] * s, hw[1] * s), y_mod.cpu()


@pytest.mark.parametrize("hw", W.SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("s,c", W.WIDE + W.CONTROLS)
def test_head_per_element_against_fp64(s, c, hw):
    m, y, y_mod = _run(s, c, hw)
    assert m._engine.plan.cfg.upsampler == 2 and y.shape == (W.BATCH, c, hw[0] * s, hw[1] * s)
    assert torch.equal(y, y_mod), "two runs of one forward differ in their bits"
    ref, tol = _head_reference(m, s, c, W.BATCH, *hw)
    err = (y.double() - ref).abs()
    ratio = float((err / tol).max())
    print(f"head s={s} c={c} N={s * s * c} {hw}: max err {float(err.max()):.3e}, max(err / tol) {ratio:.3f}, min tol {float(tol.min()):.3e}")
    assert ratio <= 1.0, f"{int((err > tol).sum())} of {err.numel()} elements off by more than the derived bound, first at {[int(v) for v in (err > tol).nonzero()[0]]}"
    # the bound is sharp enough to see a dropped, doubled or misplaced channel: the pixel-shuffled planes differ by far more than it
    moved = ref.roll(1, dims=3)
    assert float(((moved - ref).abs() / tol).median()) > 100.0


@pytest.mark.parametrize("s,c", W.CONTROLS)
def test_controls_give_the_bits_recorded_before_the_head_was_widened(s, c):
    """tests/golden/g20_head_controls.npz: sha1 of these outputs from the parent commit's library (tools/record_head_controls.py)."""
    g = load_golden("g20_head_controls")
    for hw in W.SIZES:
        m = W.model(s, c)
        with torch.no_grad():
            y = m(W.image(c, hw).cuda())
        assert W.digest(y) == str(g[W.key(s, c, hw)]), f"s={s} c={c} {hw}: the output's bits changed"


def test_plan_refuses_more_than_64_head_channels():
    from tpu_superresolution_amd._lib import SrkUnsupported
    m = W.model(9, 1)          # x9 gray: 81 head channels, five n-blocks
    with pytest.raises(SrkUnsupported, match=r"'pixelshuffledirect' path supports upscale\^2 \* in_chans <= 64 \(got 81\)"):
        with torch.no_grad():
            m(W.image(1, (8, 8)).cuda())


def test_training_through_a_wide_head_is_refused():
    from tpu_superresolution_amd._lib import SrkUnsupported, check, lib
    from tpu_superresolution_amd.engine import _stream
    m = W.model(4, 3).train()
    x = W.image(3, (8, 8)).cuda()
    with pytest.raises(SrkUnsupported, match="inference-only"):
        m(x)
    with torch.no_grad():          # the same module still predicts, in train mode too
        y = m(x)
    assert y.shape == (W.BATCH, 3, 32, 32)
    eng = m._engine          # the C entry points refuse by themselves
    ws = eng._workspace(W.BATCH, 8, 8, True)
    out = torch.empty(W.BATCH, 3, 32, 32, device="cuda")
    with pytest.raises(SrkUnsupported, match=r"forward: a 'pixelshuffledirect' head with upscale\^2 \* in_chans = 48 > 16 is inference-only"):
        check(lib().srk_swinir_forward(eng.plan.handle, eng.flat.data_ptr(), eng.packed.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), W.BATCH, 8, 8,
                                       1, None, _stream(eng.device)))
    g = torch.zeros_like(eng.flat)
    with pytest.raises(SrkUnsupported, match="backward: a 'pixelshuffledirect' head"):
        check(lib().srk_swinir_backward(eng.plan.handle, eng.flat.data_ptr(), eng.packed.data_ptr(), g.data_ptr(), out.data_ptr(), ws.data_ptr(), W.BATCH, 8, 8,
                                        None, 0, 1, _stream(eng.device)))
    assert float(g.abs().max()) == 0.0
    # the narrow head trains as before
    n = W.model(2, 3).train()
    n(W.image(3, (8, 8)).cuda()).mean().backward()
    assert n.upsample[0].weight.grad is not None and float(n.upsample[0].weight.grad.abs().max()) > 0.0
