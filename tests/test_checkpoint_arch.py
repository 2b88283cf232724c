"""checkpoint_arch without a GPU: every published configuration of the three families is constructed on the CPU from its keywords, and
`infer_arch` has to give those keywords back from the state_dict alone; `build_from_state` has to load it strictly (or refuse with the
package's own reason).  Depth changes no shape, and the full-depth rows construct in well under a second each, so they stay at full depth."""
import pytest
import torch

from tpu_superresolution_amd import DAT, HAT, SwinIR
from tpu_superresolution_amd import checkpoint_arch as CA
from tpu_superresolution_amd._lib import SrkUnsupported
from tpu_superresolution_amd.evaluate import _load_state

CTOR = {"swinir": SwinIR, "hat": HAT, "dat": DAT}


def _swinir(upscale=2, upsampler="pixelshuffle", **kw):
    d = dict(img_size=64, in_chans=3, embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, window_size=8, mlp_ratio=2, ape=False, upscale=upscale,
             img_range=1.0, upsampler=upsampler, resi_connection="1conv")
    d.update(kw)
    return d


def _hat(upscale, **kw):
    d = dict(img_size=64, in_chans=3, embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, window_size=16, compress_ratio=3, squeeze_factor=30,
             conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=2, ape=False, upscale=upscale, img_range=1.0, upsampler="pixelshuffle", resi_connection="1conv")
    d.update(kw)
    return d


def _dat(upscale, **kw):
    d = dict(img_size=64, in_chans=3, embed_dim=180, split_size=[8, 32], depth=[6] * 6, num_heads=[6] * 6, expansion_factor=4, upscale=upscale,
             img_range=1.0, resi_connection="1conv", upsampler="pixelshuffle")
    d.update(kw)
    return d


LIGHT = dict(embed_dim=60, depths=[6] * 4, num_heads=[6] * 4)
ROWS = []          # (id, family, keywords, refused?)
for s in (2, 3, 4, 8):
    for size in (48, 64):
        ROWS.append((f"swinir-classical-{size}-x{s}", "swinir", _swinir(s, img_size=size), False))
for s in (2, 3, 4):
    ROWS.append((f"swinir-light-x{s}", "swinir", _swinir(s, "pixelshuffledirect", **LIGHT), False))
for s in (2, 4):
    ROWS.append((f"swinir-realsr-m-x{s}", "swinir", _swinir(s, "nearest+conv"), False))
ROWS.append(("swinir-realsr-l-x4", "swinir", _swinir(4, "nearest+conv", embed_dim=240, depths=[6] * 9, num_heads=[8] * 9, resi_connection="3conv"), False))
for c in (1, 3):
    ROWS.append((f"swinir-dn-{c}", "swinir", _swinir(1, "", in_chans=c, img_size=128), False))
    ROWS.append((f"swinir-jpeg-{c}", "swinir", _swinir(1, "", in_chans=c, img_size=126, window_size=7, img_range=255.0), False))
for s in (2, 3, 4):
    ROWS.append((f"hat-x{s}", "hat", _hat(s), False))
    ROWS.append((f"hat-l-x{s}", "hat", _hat(s, depths=[6] * 12, num_heads=[6] * 12), False))
    ROWS.append((f"hat-s-x{s}", "hat", _hat(s, embed_dim=144, compress_ratio=24, squeeze_factor=24), False))
    ROWS.append((f"dat-x{s}", "dat", _dat(s), False))
    ROWS.append((f"dat-s-x{s}", "dat", _dat(s, split_size=[8, 16], expansion_factor=2), False))
    ROWS.append((f"dat-2-x{s}", "dat", _dat(s, expansion_factor=2), False))
    ROWS.append((f"dat-light-x{s}", "dat", _dat(s, embed_dim=60, depth=[18], num_heads=[6], expansion_factor=2, resi_connection="3conv",
                                                upsampler="pixelshuffledirect"), True))


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


def _state(family, kw):
    return CTOR[family](drop_path_rate=0.0, **kw).state_dict()


@pytest.mark.parametrize("name,family,kw,refused", ROWS, ids=[r[0] for r in ROWS])
def test_published_configuration_round_trips(name, family, kw, refused):
    sd = _state(family, kw)
    spec = CA.infer_arch(sd)
    assert spec.arch == family
    assert spec.kwargs == kw, {k: (spec.kwargs.get(k), kw.get(k)) for k in set(kw) | set(spec.kwargs) if spec.kwargs.get(k) != kw.get(k)}
    rebuilt = CTOR[family](drop_path_rate=0.0, **spec.kwargs).state_dict()
    assert _shapes(rebuilt) == _shapes(sd)
    if refused:
        with pytest.raises(SrkUnsupported, match="resi_connection='3conv'"):
            CA.build_from_state(sd)
        return
    model, spec2 = CA.build_from_state(sd)          # strict load inside
    assert spec2.kwargs == kw and type(model) is CTOR[family]
    got = model.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)


# ---- small models for everything below ------------------------------------------------------------------------------------------------------
def tiny_swinir(**kw):
    d = _swinir(2, img_size=16, embed_dim=24, depths=[2, 2], num_heads=[2, 2])
    d.update(kw)
    return d


def tiny_hat(**kw):
    d = _hat(2, embed_dim=24, depths=[2], num_heads=[2], compress_ratio=3, squeeze_factor=6)
    d.update(kw)
    return d


def tiny_dat(**kw):
    d = _dat(2, img_size=32, embed_dim=32, depth=[2, 2], num_heads=[2, 2], split_size=[8, 16], expansion_factor=2)
    d.update(kw)
    return d


def test_module_prefix_is_stripped_only_when_uniform():
    sd = _state("swinir", tiny_swinir())
    pre = {"module." + k: v for k, v in sd.items()}
    assert CA.infer_arch(pre).kwargs == tiny_swinir()
    model, _ = CA.build_from_state(pre)
    assert _shapes(model.state_dict()) == _shapes(sd)
    mixed = dict(sd)
    mixed["module.conv_first.weight"] = mixed.pop("conv_first.weight")
    with pytest.raises(ValueError, match="conv_first.weight"):
        CA.infer_arch(mixed)


@pytest.mark.parametrize("envelope", ["params_ema", "params", "model", None])
def test_envelopes_through_load_state(tmp_path, envelope):
    sd = _state("hat", tiny_hat(upscale=3))
    path = tmp_path / "w.pt"
    torch.save(sd if envelope is None else {envelope: sd, "iter": 7}, path)
    state, msg = _load_state(str(path), "auto")
    assert ("raw" in msg) if envelope is None else (f"'{envelope}'" in msg)
    model, spec = CA.build_from_state(state)
    assert spec.arch == "hat" and spec.kwargs == tiny_hat(upscale=3) and isinstance(model, HAT)


def test_the_two_conventions_and_the_override():
    jpeg = _state("swinir", tiny_swinir(upscale=1, upsampler="", window_size=7, img_size=21, in_chans=1, img_range=255.0))
    spec = CA.infer_arch(jpeg)
    assert spec.kwargs["img_range"] == 255.0 and spec.kwargs["window_size"] == 7 and spec.kwargs["img_size"] == 21
    assert any(n.startswith("img_range=255") for n in spec.notes)
    dn = _state("swinir", tiny_swinir(upscale=1, upsampler="", in_chans=1))
    spec = CA.infer_arch(dn)
    assert spec.kwargs["img_range"] == 1.0 and any(n.startswith("img_range=1.0") for n in spec.notes)
    sr7 = CA.infer_arch(_state("swinir", tiny_swinir(window_size=7, img_size=21)))
    assert sr7.kwargs["img_range"] == 1.0          # window 7 alone is not the JPEG convention: the head must be the scale-1 one
    model, spec = CA.build_from_state(jpeg, img_range=1.0)
    assert model.img_range == 1.0 and spec.kwargs["img_range"] == 1.0
    assert [n for n in spec.notes if n.startswith("img_range=")] == ["img_range=1.0: given by the caller"]
    with pytest.raises(ValueError, match="img_range"):
        CA.build_from_state(jpeg, img_range=0.0)
    hat = CA.infer_arch(_state("hat", tiny_hat(conv_scale=0.5)))          # conv_scale leaves no trace in a file
    assert hat.kwargs["conv_scale"] == 0.01 and any(n.startswith("conv_scale=0.01") for n in hat.notes)
    assert any(n.startswith("img_size=64") for n in hat.notes) and hat.kwargs["img_size"] == 64


def test_img_size_default_without_a_mask_is_noted():
    spec = CA.infer_arch(_state("swinir", tiny_swinir(depths=[1, 1], img_size=24)))          # one block per group: no shifted block, no mask
    assert spec.kwargs["img_size"] == 64 and spec.kwargs["depths"] == [1, 1] and any(n.startswith("img_size=64") for n in spec.notes)
    ape = CA.infer_arch(_state("swinir", tiny_swinir(depths=[1, 1], img_size=24, ape=True)))
    assert ape.kwargs["img_size"] == 24 and ape.kwargs["ape"] is True


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_unknown_family_names_the_markers():
    with pytest.raises(ValueError) as e:
        CA.infer_arch({"body.0.weight": torch.zeros(4, 3, 3, 3)})
    for key in ("relative_position_index_SA", "before_RG.1.weight", "patch_embed.norm.weight", "layers.0.residual_group.blocks.0.attn.relative_position_index"):
        assert key in str(e.value)
    with pytest.raises(ValueError, match="none of SwinIR, HAT and DAT"):
        CA.infer_arch({})


@pytest.mark.parametrize("family,kw,marker", [("swinir", tiny_swinir(), "patch_embed.norm.weight"), ("hat", tiny_hat(), "relative_position_index_SA"),
                                              ("dat", tiny_dat(), "before_RG.1.weight")])
def test_deleted_marker_key(family, kw, marker):
    sd = _state(family, kw)
    del sd[marker]
    with pytest.raises(ValueError, match="none of SwinIR, HAT and DAT"):
        CA.infer_arch(sd)


def test_deleted_body_key_is_named():
    sd = _state("swinir", tiny_swinir())
    del sd["layers.1.residual_group.blocks.0.mlp.fc1.weight"]
    with pytest.raises(ValueError, match=r"layers\.1\.residual_group\.blocks\.0\.mlp\.fc1\.weight"):
        CA.infer_arch(sd)


def test_inconsistent_shapes_name_their_keys():
    base = _state("swinir", tiny_swinir())
    sd = dict(base)          # heads that do not divide embed_dim
    for k in list(sd):
        if k.startswith("layers.0.") and k.endswith("relative_position_bias_table"):
            sd[k] = torch.zeros(225, 5)
    with pytest.raises(ValueError, match=r"layers\.0\..*relative_position_bias_table.*5 heads do not divide embed_dim = 24"):
        CA.infer_arch(sd)
    sd = dict(base)          # a non-square index table
    sd["layers.0.residual_group.blocks.0.attn.relative_position_index"] = torch.zeros(64, 49, dtype=torch.long)
    with pytest.raises(ValueError, match=r"relative_position_index \(64, 49\).*square"):
        CA.infer_arch(sd)
    sd = dict(base)          # stages that disagree: one block's fc1 is wider
    sd["layers.1.residual_group.blocks.1.mlp.fc1.weight"] = torch.zeros(96, 24)
    with pytest.raises(ValueError, match=r"mlp\.fc1\.weight: the stages disagree"):
        CA.infer_arch(sd)
    sd = dict(base)          # blocks of one group with different head counts
    sd["layers.0.residual_group.blocks.1.attn.relative_position_bias_table"] = torch.zeros(225, 4)
    with pytest.raises(ValueError, match=r"layers\.0\..*the stages disagree"):
        CA.infer_arch(sd)
    sd = dict(base)          # the table's rows contradict the window
    sd["layers.0.residual_group.blocks.0.attn.relative_position_index"] = torch.zeros(49, 49, dtype=torch.long)
    with pytest.raises(ValueError, match=r"225 rows.*window 7"):
        CA.infer_arch(sd)
    sd = dict(base)          # a head that is none of the four
    del sd["conv_last.weight"], sd["conv_last.bias"]
    del sd["upsample.0.weight"], sd["upsample.0.bias"]
    with pytest.raises(ValueError, match="the head is none of"):
        CA.infer_arch(sd)
    dat = _state("dat", tiny_dat())
    dat["layers.0.blocks.0.attn.attns.0.rpe_biases"] = dat["layers.0.blocks.0.attn.attns.0.rpe_biases"][:-1]
    with pytest.raises(ValueError, match=r"rpe_biases.*rows"):
        CA.infer_arch(dat)
    hat = _state("hat", tiny_hat())
    hat["layers.0.residual_group.overlap_attn.relative_position_bias_table"] = torch.zeros(40 * 40 + 1, 2)
    with pytest.raises(ValueError, match=r"overlap_attn\.relative_position_bias_table.*not a square"):
        CA.infer_arch(hat)


def test_dat_light_is_inferred_then_refused_with_its_reason():
    kw = tiny_dat(embed_dim=32, depth=[4], num_heads=[2], resi_connection="3conv", upsampler="pixelshuffledirect", upscale=4)
    sd = _state("dat", kw)
    assert CA.infer_arch(sd).kwargs == kw
    with pytest.raises(SrkUnsupported, match=r"DAT\(.*resi_connection='3conv'.*does not cover resi_connection='3conv'"):
        CA.build_from_state(sd)
    # the one-step head alone (wide) keeps DAT's refusal: the host-run models stay at 16 output channels
    sd = _state("dat", dict(kw, resi_connection="1conv"))
    with pytest.raises(SrkUnsupported, match=r"pixelshuffledirect with upscale\^2 \* in_chans > 16"):
        CA.build_from_state(sd)


def test_host_run_swinir_keeps_its_wide_head_refusal_and_the_engine_its_cap():
    with pytest.raises(SrkUnsupported, match=r"pixelshuffledirect with upscale\^2 \* in_chans > 16"):
        CA.build_from_state(_state("swinir", tiny_swinir(window_size=4, upsampler="pixelshuffledirect", upscale=4)))
    with pytest.raises(SrkUnsupported, match=r"upscale\^2 \* in_chans > 64"):
        CA.build_from_state(_state("swinir", tiny_swinir(upsampler="pixelshuffledirect", upscale=9, in_chans=1)))
    model, spec = CA.build_from_state(_state("swinir", tiny_swinir(upsampler="pixelshuffledirect", upscale=8, in_chans=1)))          # the cap itself
    assert spec.kwargs["upscale"] == 8 and model.upsample[0].weight.shape[0] == 64


# ---- negative controls: each edit must change the inferred keywords ---------------------------------------------------------------------------
def test_swapped_split_size_changes_the_keywords():
    a = CA.infer_arch(_state("dat", tiny_dat(split_size=[8, 16])))
    b = CA.infer_arch(_state("dat", tiny_dat(split_size=[16, 8])))          # the same shapes everywhere: only the buffer's contents differ
    assert _shapes(_state("dat", tiny_dat(split_size=[8, 16])))["layers.0.blocks.0.attn.attns.0.rpe_biases"] == \
        _shapes(_state("dat", tiny_dat(split_size=[16, 8])))["layers.0.blocks.0.attn.attns.0.rpe_biases"]
    assert a.kwargs["split_size"] == [8, 16] and b.kwargs["split_size"] == [16, 8]


def test_dropped_conv_up2_changes_the_scale():
    sd = _state("swinir", tiny_swinir(upsampler="nearest+conv", upscale=4))
    assert CA.infer_arch(sd).kwargs["upscale"] == 4
    del sd["conv_up2.weight"], sd["conv_up2.bias"]
    spec = CA.infer_arch(sd)
    assert spec.kwargs["upscale"] == 2 and spec.kwargs["upsampler"] == "nearest+conv"
    CA.build_from_state(sd)          # and it is a complete x2 file


def test_widened_fc1_changes_the_ratio():
    for family, kw, key, name in (("swinir", tiny_swinir(), "mlp_ratio", "mlp"), ("hat", tiny_hat(), "mlp_ratio", "mlp"), ("dat", tiny_dat(), "expansion_factor", "ffn")):
        sd = _state(family, kw)
        for k in list(sd):
            if k.endswith(f"{name}.fc1.weight"):
                sd[k] = torch.zeros(sd[k].shape[0] * 2, sd[k].shape[1])
        assert CA.infer_arch(sd).kwargs[key] == 2 * kw[key]


def test_3conv_keys_change_resi_connection():
    a = CA.infer_arch(_state("swinir", tiny_swinir()))
    b = CA.infer_arch(_state("swinir", tiny_swinir(resi_connection="3conv")))
    assert a.kwargs["resi_connection"] == "1conv" and b.kwargs["resi_connection"] == "3conv"
    assert {k: v for k, v in a.kwargs.items() if k != "resi_connection"} == {k: v for k, v in b.kwargs.items() if k != "resi_connection"}


def test_hat_ratios_follow_the_shapes():
    spec = CA.infer_arch(_state("hat", tiny_hat(compress_ratio=4, squeeze_factor=12, overlap_ratio=0.25)))
    assert (spec.kwargs["compress_ratio"], spec.kwargs["squeeze_factor"], spec.kwargs["overlap_ratio"]) == (4, 12, 0.25)


def test_format_call_is_the_constructor_call():
    spec = CA.infer_arch(_state("swinir", tiny_swinir()))
    line = CA.format_call(spec)
    assert line.startswith("SwinIR(img_size=16, in_chans=3, embed_dim=24, depths=[2, 2], num_heads=[2, 2], window_size=8, mlp_ratio=2")
    assert eval(line, {"SwinIR": lambda **kw: kw}) == spec.kwargs
