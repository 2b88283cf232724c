"""Training at window sizes 2..7, the parts that need no GPU: G19 pins the CPU oracle's loss_and_grads to the reference's training
record (fixture from tools/make_golden_wsmall_train.py), option parsing, the optimizer's classification of models and the refusals of
SwinIR.enable_small_window_training."""
import pytest
import torch

from conftest import load_golden
from oracle import swinir_oracle as O
from test_oracle_golden_wsmall import WSMALL, wsmall_weights

# 10 x the worst max-over-tensors |d| / |ref| observed between the oracle's autograd and the reference's on the four tags (1.52e-6, tag
# 'ps'; 'ws4' 5.7e-7; 'car' and 'psd' agree bit for bit); capped at 1e-3
G19_GRAD_BOUND = 1.52e-5
assert G19_GRAD_BOUND <= 1e-3


@pytest.mark.parametrize("tag", sorted(WSMALL))
def test_g19_oracle_loss_and_grads_vs_reference(tag):
    """The oracle's L1 loss and every parameter gradient at window_size 7 / 4 against the reference's own autograd (drop_path 0, a
    2 x C x 16 x 19 batch with reflect padding).  Observed here, fp32 autograd on both sides: loss equal to the last digit on all four
    tags; worst relative L2 error over tensors 0 ('car'), 1.52e-6 ('ps'), 0 ('psd'), 5.7e-7 ('ws4')."""
    g = load_golden("g19_swinir_wsmall_train")
    _, cfg, sd = wsmall_weights(tag)
    assert str(g[f"{tag}.weight_sha1"]) == str(load_golden("g17_swinir_wsmall")[f"{tag}.weight_sha1"])
    h, w = (int(v) for v in g["hw"])
    x = torch.rand(2, cfg.in_chans, h, w, generator=torch.Generator().manual_seed(int(g["x_seed"])))
    t = torch.rand(2, cfg.in_chans, h * cfg.upscale, w * cfg.upscale, generator=torch.Generator().manual_seed(int(g["t_seed"])))
    loss, out, grads = O.loss_and_grads(sd, cfg, x, t)
    assert out.shape == t.shape
    assert abs(float(loss) - float(g[f"{tag}.loss"])) <= 2e-5 * float(g[f"{tag}.loss"])
    keys = O.param_keys(cfg)
    assert list(grads) == keys and len(g[f"{tag}.grad_norms"]) == len(keys)
    worst = 0.0
    for k, norm in zip(keys, g[f"{tag}.grad_norms"]):
        ref = torch.from_numpy(g[f"{tag}.grad.{k}"])
        assert ref.shape == grads[k].shape, k
        assert abs(float(ref.double().norm()) - float(norm)) <= 1e-6 * float(norm) + 1e-12, k
        worst = max(worst, float((grads[k] - ref).norm() / ref.norm()))
    print(f"{tag}: worst relative L2 gradient error {worst:.3e}")
    assert worst <= G19_GRAD_BOUND, (tag, worst)


def test_window_size_option_parses_and_builds_reference_state_dict():
    from tpu_superresolution_amd import evaluate, finetune_swinir
    a = finetune_swinir.parse_args(["--data_root", "D", "--scale", "X2", "--window_size", "7", "--graph"])
    assert a.window_size == 7 and a.graph and a.arch == "swinir"
    assert finetune_swinir.parse_args(["--data_root", "D", "--scale", "X2"]).window_size == 8
    for bad in (["--window_size", "9"], ["--window_size", "1"], ["--window_size", "7", "--arch", "hat"], ["--graph"]):
        with pytest.raises(SystemExit):
            finetune_swinir.parse_args(["--data_root", "D", "--scale", "X2", *bad])
    e = evaluate.parse_args(["--scale", "X4", "--ckpt", "F", "--arch", "swinir", "--window_size", "7"])
    assert e.window_size == 7
    assert evaluate.parse_args(["--scale", "X4", "--ckpt", "F"]).window_size == 8
    with pytest.raises(SystemExit):
        evaluate.parse_args(["--scale", "X4", "--ckpt", "F", "--window_size", "7"])          # default --arch ms_resunet
    m = finetune_swinir.build_model(2, window_size=7)
    assert m.window_size == 7
    cfg = O.SwinIRConfig(upscale=2, in_chans=3, img_size=63, window_size=7, img_range=1.0, depths=(6,) * 6, embed_dim=180,
                         num_heads=(6,) * 6, mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")
    assert list(m.state_dict().keys()) == [k for k, _, _ in O.state_dict_schema(cfg)]
    assert finetune_swinir.build_sr_model("swinir", 2, window_size=7).window_size == 7
    assert finetune_swinir.build_model(2).window_size == 8
    with pytest.raises(ValueError):
        finetune_swinir.build_sr_model("hat", 2, window_size=7)


TINY7 = dict(img_size=14, in_chans=3, embed_dim=24, depths=[2], num_heads=[2], window_size=7, mlp_ratio=2, upscale=2, img_range=1.0,
             upsampler="pixelshuffle", resi_connection="1conv")


def test_fused_adamw_classifies_enabled_small_window_models_as_list_models():
    import tpu_superresolution_amd as T
    from tpu_superresolution_amd.hat_arch import HAT
    from tpu_superresolution_amd.optim import FusedAdamW, trains_through_engine
    w8 = T.SwinIR(**{**TINY7, "window_size": 8, "img_size": 16})
    assert trains_through_engine(w8) and FusedAdamW(w8)._flat is True
    hat = HAT(img_size=32, embed_dim=24, depths=[1], num_heads=[2], window_size=16, upscale=2, upsampler="pixelshuffle")
    assert not trains_through_engine(hat) and FusedAdamW(hat)._flat is False
    w7 = T.SwinIR(**TINY7)
    late = FusedAdamW(w7)
    assert late._flat is True          # not enabled yet: classified as an engine model
    assert w7.enable_small_window_training() is w7          # touches no device
    assert not trains_through_engine(w7) and FusedAdamW(w7)._flat is False
    with pytest.raises(RuntimeError, match="enable_small_window_training"):
        late.step()


@pytest.mark.parametrize("bad", [dict(window_size=8, img_size=16), dict(window_size=16, img_size=32), dict(upsampler="nearest+conv"),
                                 dict(resi_connection="3conv"), dict(ape=True), dict(use_checkpoint=True), dict(img_size=7),
                                 dict(upsampler="", upscale=2)])
def test_enable_small_window_training_refuses_what_the_path_does_not_cover(bad):
    import tpu_superresolution_amd as T
    from tpu_superresolution_amd._lib import SrkUnsupported
    m = T.SwinIR(**{**TINY7, **bad})
    with pytest.raises(SrkUnsupported, match="enable_small_window_training"):
        m.enable_small_window_training()
    assert not getattr(m, "_small_window_training", False)
    assert m.draw_drop_path(2, "cpu") is None


def test_enable_small_window_training_accepts_the_three_heads():
    import tpu_superresolution_amd as T
    for head in (dict(upsampler="pixelshuffle"), dict(upsampler="pixelshuffledirect"), dict(upsampler="", upscale=1, in_chans=1)):
        for ws in (2, 4, 7):
            m = T.SwinIR(**{**TINY7, **head, "window_size": ws, "img_size": 4 * ws})
            assert m.enable_small_window_training() is m
    m.train()
    d = m.draw_drop_path(3, "cpu")
    assert d.shape == (2, 2, 3)
    assert T.SwinIR(**{**TINY7, "drop_path_rate": 0.0}).enable_small_window_training().train().draw_drop_path(3, "cpu") is None
