"""Training through a wide one-step head (17 .. 64 output channels) on the device.

Direct calls: srk_widehead_grad_prep / _wgrad / _dgrad (include/srk.h, csrc/headconv_wide.hip) through the C ABI against the fp64
restatement and the derived bound of tests/wide_head_ref.py (pinned on the CPU by tests/test_wide_head_train_ref.py), in the manner of
tests/test_gpu_wgrad.py: outputs in Guarded buffers, operands between NaN rows, the exact class with torch.equal, the random and
dyadic classes per element, the accumulate contract, +0 pad columns of dx.

Whole model: fixture G21 (the reference's train-mode loss and gradients at 27 / 48 / 64 head channels) through
SwinIR.enable_wide_head_training() at the tolerances tests/test_gpu_model.py uses for the narrow heads.

The head's two tensors alone: the light-width model of tests/wide_head_case.py; the head's input ('fb') and output gradient ('gyimg')
are read back from the workspace and the engine's upsample.0 gradients are held to the direct-call bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_scales as GS
import test_gpu_wgrad as TW
import wgrad_ref as R
import wide_head_case as W
import wide_head_ref as WH
from guarded import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib


# ---- direct calls -----------------------------------------------------------------------------------------------------------------
def call(L, c, dev, bufs):
    h = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    B, H, Wd = c.geo
    if c.kind == "imgprep":
        Hc, Wc = c.img_hw
        inv = R.EXACT_INV_RANGE if c.cls == "exact" else R.IMG_INV_RANGE
        return h.srk_widehead_grad_prep(dev["d_pred"].ptr(), bufs["gy"].ptr, B, c.Cimg, Hc, Wc, H, Wd, c.r, c.CoP, inv, st)
    if c.kind == "smallw":
        return h.srk_widehead_wgrad(dev["x"].ptr(), dev["gy"].ptr(), bufs["dw"].ptr, bufs["db"].ptr, B, H, Wd, c.Cin, c.CinP, c.Co, c.CoP, st)
    return h.srk_widehead_dgrad(dev["gy"].ptr(), dev["weight"].ptr(), bufs["dx"].ptr, B, H, Wd, c.Cin, c.CinP, c.Co, c.CoP, st)


def run(L, c, inp, dev, repeat=1):
    bufs = TW.outputs(c, inp)
    for _ in range(repeat):
        rc = call(L, c, dev, bufs)
        assert rc == 0, (rc, L.lib().srk_last_error().decode())
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("c", WH.CASES, ids=lambda c: c.id)
def test_direct_calls_values_guards_and_contracts(L, c):
    inp = WH.make_inputs(c)
    exp = WH.expected(c, inp)
    dev = TW.upload(c, inp)
    bufs = run(L, c, inp, dev)
    for k, b in bufs.items():
        b.assert_guards(f"{c.id} {k}")
    got = TW.read(c, bufs, exp)
    ok, ratios = WH.accepts(c, got, exp)
    print(f"[widehead] {c.id} " + " ".join(f"{k}:{v:.3f}" for k, v in ratios.items()))
    assert ok, f"max(err / tol) {ratios}"
    if c.kind == "smalld":
        assert bool((TW.bits(bufs["dx"].data()[:, c.Cin:]) == 0).all()), "pad columns of dx are not +0"
    if c.kind == "imgprep":
        gy = bufs["gy"].data()
        assert bool((TW.bits(gy[:, c.Cimg * c.r * c.r:]) == 0).all())
    if c.kind in R.ACCUMULATING:                              # a second call adds the same increment again
        bufs = run(L, c, inp, dev, repeat=2)
        for k, b in bufs.items():
            b.assert_guards(f"{c.id} twice {k}")
        ok, ratios = WH.accepts(c, TW.read(c, bufs, exp), TW.twice(exp, inp))
        assert ok, f"second call: {ratios}"


# ---- whole model ------------------------------------------------------------------------------------------------------------------
def _train_model(cfg, sd, enable=True):
    import tpu_superresolution_amd as T
    m = T.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    m = m.cuda().train()
    return m.enable_wide_head_training() if enable else m


@pytest.mark.parametrize("hw", WH.G21_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("tag", WH.G21_TAGS)
def test_g21_gradients_vs_reference_golden(tag, hw):
    g, cfg, sd = WH.g21_checked_weights(tag)
    key = f"{tag}.{hw[0]}x{hw[1]}"
    m = _train_model(cfg, sd)
    x, t = torch.from_numpy(g[f"{key}.x"]).cuda(), torch.from_numpy(g[f"{key}.target"]).cuda()
    loss = torch.nn.functional.l1_loss(m(x), t)
    loss.backward()
    ref_loss = float(g[f"{key}.loss"])
    rels = {}
    for n, p in m.named_parameters():
        ref = torch.from_numpy(g[f"{key}.grad.{n}"])
        assert p.grad is not None and p.grad.shape == ref.shape, n
        rels[n] = float((p.grad.cpu() - ref).norm() / (ref.norm() + 1e-12))
    worst = max(rels, key=rels.get)
    print(f"[g21] {key}: loss {float(loss.detach()):.6f} (ref {ref_loss:.6f}), median rel L2 {np.median(list(rels.values())):.3e}, "
          f"worst {worst} {rels[worst]:.3e}, head weight {rels['upsample.0.weight']:.3e} bias {rels['upsample.0.bias']:.3e}")
    assert abs(float(loss.detach()) - ref_loss) <= 2e-3 * ref_loss
    for n, rel in rels.items():
        assert rel <= 0.1, f"{n}: relative L2 error {rel:.3e}"
    assert float(np.median(list(rels.values()))) <= 0.04
    g1 = {n: p.grad.clone() for n, p in m.named_parameters()}          # a second backward doubles the gradients
    torch.nn.functional.l1_loss(m(x), t).backward()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * g1[n], rtol=1e-3, atol=1e-6 * float(g1[n].abs().max())), n


# ---- the head's two tensors alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", W.SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("s,c", W.WIDE)
def test_head_gradients_against_fp64_of_the_workspace_operands(s, c, hw):
    m = W.model(s, c).train().enable_wide_head_training()
    x = W.image(c, hw).cuda()
    Co, CoP = s * s * c, (s * s * c + 15) // 16 * 16
    Hp, Wp = (hw[0] + 7) // 8 * 8, (hw[1] + 7) // 8 * 8
    d_y = torch.randn(W.BATCH, c, hw[0] * s, hw[1] * s, generator=torch.Generator().manual_seed(11 * s + c)).cuda()
    m(x).backward(d_y)
    torch.cuda.synchronize()
    eng = m._engine
    fb = eng.activation("fb", torch.bfloat16).view(W.BATCH, Hp, Wp, 64).cpu()
    gy = eng.activation("gyimg", torch.float32).view(W.BATCH * Hp * Wp, CoP).cpu()
    # gyimg is the prep of d_y: un-shuffled, times 1 / img_range, zero in the pad columns and outside the crop
    prep = R.prep_case(W.BATCH, Hp, Wp, s, c, CoP, crop=(Hp * s - hw[0] * s, Wp * s - hw[1] * s), cls="random")
    want = (d_y.cpu() * torch.tensor(1.0 / W.IMG_RANGE, dtype=torch.float32)).double()
    full = torch.zeros(W.BATCH, c, Hp * s, Wp * s, dtype=torch.float64)
    full[:, :, :hw[0] * s, :hw[1] * s] = want
    un = full.reshape(W.BATCH, c, Hp, s, Wp, s).permute(0, 2, 4, 1, 3, 5).reshape(prep.M, Co)
    assert torch.equal(gy[:, :Co].double(), un) and bool((TW.bits(gy[:, Co:]) == 0).all())
    case = R.head_case("smallw", "random", W.BATCH, Hp, Wp, 60, 64, Co, CoP)
    inp = {"x": fb, "gy": gy, "dw_0": torch.zeros(Co, 60, 3, 3), "db_0": torch.zeros(Co)}
    exp = WH.expected(case, inp)
    got = {"dw": m.upsample[0].weight.grad.cpu(), "db": m.upsample[0].bias.grad.cpu()}
    ok, ratios = WH.accepts(case, got, exp)
    print(f"[head grads] s={s} c={c} Co={Co} {hw}: max(err / tol) {ratios}")
    assert ok, ratios
    assert float(exp["dw"].ref.abs().max()) > 0 and float(exp["db"].ref.abs().max()) > 0


# ---- the opt-in -------------------------------------------------------------------------------------------------------------------
def test_enabled_model_predicts_the_same_bits():
    for s, c in ((4, 3), (3, 3)):
        x = W.image(c, (11, 13)).cuda()
        with torch.no_grad():
            plain = W.digest(W.model(s, c)(x))
            on = W.model(s, c).enable_wide_head_training()
            assert W.digest(on(x)) == plain                      # enabled before the plan exists
            late = W.model(s, c)
            assert W.digest(late(x)) == plain
            late.enable_wide_head_training()                     # enabled on a live plan: the workspace is dropped and re-made
            assert late._engine.workspace is None and W.digest(late(x)) == plain
            assert W.digest(late.train()(x)) == plain
        late(x).mean().backward()                                # and the late-enabled model trains
        assert float(late.upsample[0].weight.grad.abs().max()) > 0.0


def test_narrow_head_gives_the_same_gradient_bits_with_the_option_on():
    """A 12-channel head (x2 RGB) with the option 0 and 1.  What the option could touch is the head's own path, and every step of it is
    a fixed sequence of fp32 operations at this size: the training forward's output, the workspace layout, the prepared gradient
    'gyimg' and the head's weight gradient (one workgroup, one thread per element) -- these are compared BIT FOR BIT.  Other gradients
    of the engine (LayerNorm gains and biases, bias sums) are accumulated with fp32 atomics and differ in their last bits between
    two runs of the SAME option, so bit equality cannot be asked of them: each is held to eight times the difference of two runs
    with the option off plus 1e-5 of the tensor's largest value (atomic reordering moves a sum by a few u = 6e-8 of it)."""
    x = W.image(3, (11, 13)).cuda()
    d_y = torch.randn(W.BATCH, 3, 22, 26, generator=torch.Generator().manual_seed(5)).cuda()
    runs = []
    for opt in (0, 0, 1):
        m = W.model(2, 3).train()
        assert m.enable_wide_head_training() is m and not getattr(m, "plan_options", None)          # a no-op for 12 channels
        m.plan_options = {"wide_head_train": opt}
        y = m(x)
        y.backward(d_y)
        torch.cuda.synchronize()
        assert m._engine.plan.get_option("wide_head_train") == (opt, True)
        runs.append({"y": y.detach().clone(), "gyimg": m._engine.activation("gyimg", torch.float32).clone(),
                     "ws_bytes": m._engine.workspace.numel(), "grads": {n: p.grad.clone() for n, p in m.named_parameters()}})
    off, again, on = runs
    for k in ("y", "gyimg"):
        assert torch.equal(TW.bits(off[k]), TW.bits(on[k])) and torch.equal(TW.bits(off[k]), TW.bits(again[k])), k
    assert off["ws_bytes"] == on["ws_bytes"] and on["gyimg"].numel() == W.BATCH * 16 * 16 * 16
    worst = ("", 0.0)
    for n, g0 in off["grads"].items():
        g1, g2 = again["grads"][n], on["grads"][n]
        top = float(g0.abs().max())
        noise, diff = float((g1 - g0).abs().max()), float((g2 - g0).abs().max())
        worst = max(worst, (n, diff / (top + 1e-30)), key=lambda p: p[1])
        if n == "upsample.0.weight":
            assert torch.equal(TW.bits(g0), TW.bits(g1)) and torch.equal(TW.bits(g0), TW.bits(g2)), n
        assert diff <= 8.0 * noise + 1e-5 * top, f"{n}: option on differs by {diff:.3e}, two runs with it off by {noise:.3e} (max |g| {top:.3e})"
    print(f"[narrow] largest on / off difference: {worst[0]} {worst[1]:.2e} of the tensor's maximum")


def test_enable_refuses_what_it_does_not_cover():
    import tpu_superresolution_amd as T
    from tpu_superresolution_amd._lib import SrkUnsupported
    with pytest.raises(SrkUnsupported, match=r"upscale\^2 \* in_chans = 81 > 64"):
        W.model(9, 1).enable_wide_head_training()
    kw = W.config(4, 3).kwargs()
    with pytest.raises(SrkUnsupported, match=r"window_size = 7 .* stops at 16 head channels"):
        T.SwinIR(drop_path_rate=0.0, **{**kw, "window_size": 7, "img_size": 14}).enable_wide_head_training()
    with pytest.raises(SrkUnsupported, match="has no one-step head"):
        T.SwinIR(drop_path_rate=0.0, **{**kw, "upsampler": "pixelshuffle", "upscale": 4}).enable_wide_head_training()
    m = W.model(4, 3).train()                                    # without the call: the parent's refusal
    with pytest.raises(SrkUnsupported, match="inference-only"):
        m(W.image(3, (8, 8)).cuda())


def test_three_optimizer_steps_on_the_tiny_x4_model():
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import train_step
    _, cfg, sd = WH.g21_checked_weights("psd4")
    m = _train_model(cfg, sd)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
    x, t = WH.g21_input("psd4", (16, 16)).cuda(), WH.g21_target("psd4", (16, 16)).cuda()
    w0 = m.upsample[0].weight.detach().clone()
    losses = []
    for _ in range(3):
        loss, bad = train_step(m, opt, x, t)
        assert int(bad) == 0
        losses.append(float(loss))
    assert all(np.isfinite(losses)), losses
    assert float((m.upsample[0].weight.detach() - w0).abs().max()) > 0.0, "the head's weights did not move"
    print(f"[train] psd4 losses {losses}")
