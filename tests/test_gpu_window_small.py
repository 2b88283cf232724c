"""SwinIR with window sizes 2..7 on the HIP path (inference): the small-window attention kernel (csrc/attn_small.hip) against an fp32
torch restatement, whole models against the reference's G17 vectors and the CPU oracle, and the refusals that go with the path."""
import numpy as np
import pytest
import torch

from oracle import swinir_oracle as O
from test_oracle_golden_wsmall import SIZES, WSMALL, wsmall_weights

pytestmark = pytest.mark.gpu


def build(cfg, sd):
    import tpu_superresolution_amd as T
    m = T.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m.cuda().eval()


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def attention_reference(qkv, table, B, H, W, ws, shift, nH, dh, scale):
    """fp32 restatement of WindowAttention.forward + roll / partition / reverse (network_swinir.py:114-145, :240-279) on the raster
    qkv layout of the kernel, built from the oracle's index map, dense bias and shift mask."""
    CA = qkv.shape[1] // 3
    idx = torch.from_numpy(O.window_token_index(H, W, ws, shift))                       # [nW, N]
    nW, N = idx.shape
    rows = (torch.arange(B)[:, None, None] * H * W + idx[None]).reshape(-1)             # window-order row -> raster token

    def head(which):
        t = qkv[:, which * CA:(which + 1) * CA].reshape(-1, nH, 32)[:, :, :dh]
        return t[rows].reshape(B * nW, N, nH, dh).permute(0, 2, 1, 3)                  # [B_, nH, N, dh]
    q, k, v = head(0), head(1), head(2)
    s = (q * scale) @ k.transpose(-1, -2) + O.dense_rel_pos_bias(table, ws)[None]
    if shift > 0:
        mask = torch.from_numpy(O.shift_attn_mask(H, W, ws, shift))
        s = (s.reshape(B, nW, nH, N, N) + mask[None, :, None]).reshape(B * nW, nH, N, N)
    o = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3)                               # [B_, N, nH, dh]
    out = torch.zeros(B * H * W, nH, 32)
    out[rows] = torch.nn.functional.pad(o, (0, 32 - dh)).reshape(-1, nH, 32)
    return out.reshape(B * H * W, nH * 32)


@pytest.mark.parametrize("ws", [2, 3, 4, 5, 6, 7])
def test_small_window_attention_kernel_vs_fp32_restatement(ws):
    from tpu_superresolution_amd import ops
    B, H, W = 2, 3 * ws, 5 * ws
    for nH, dh in ((1, 24), (2, 16), (6, 30)) + (((9, 20),) if ws == 7 else ()):      # 9 heads: more heads than waves per workgroup
        CA = nH * 32
        for shift in (0, ws // 2):
            gen = torch.Generator().manual_seed(100 * ws + 10 * nH + shift)
            qkv = torch.randn(B * H * W, 3, nH, 32, generator=gen)
            qkv[..., dh:] = 0.0                                                          # head_dim zero-padded to 32
            qkv = qkv.reshape(B * H * W, 3 * CA).to(torch.bfloat16)
            table = torch.randn((2 * ws - 1) ** 2, nH, generator=gen) * 2.0
            scale = dh ** -0.5
            out = ops.window_attention_small_fwd(qkv.cuda(), table.cuda(), B, H, W, ws, shift, nH, scale).float().cpu()
            ref = attention_reference(qkv.float(), table, B, H, W, ws, shift, nH, dh, scale)
            assert not torch.isnan(out).any(), (ws, nH, shift)
            err = float((out - ref).abs().max())
            assert err <= 1e-2 * max(1.0, float(ref.abs().max())), (ws, nH, shift, err)
            assert float(out.reshape(-1, nH, 32)[..., dh:].abs().max()) == 0.0


def test_small_window_attention_refuses_other_windows_and_shapes():
    from tpu_superresolution_amd import _lib
    L = _lib.lib()
    nH, CA = 2, 64
    qkv = torch.zeros(2 * 14 * 14, 3 * CA, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(2 * 14 * 14, CA, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(13 * 13, nH, device="cuda")

    def call(ws, H, W, shift=0):
        return L.srk_win_small_attention_fwd(qkv.data_ptr(), 3 * CA, CA, table.data_ptr(), out.data_ptr(), CA, 2, H, W, ws, shift, nH,
                                             0.25, torch.cuda.current_stream().cuda_stream)
    assert call(8, 16, 8) == -3 and b"2..7" in L.srk_last_error()                        # SRK_E_UNSUPPORTED
    assert call(1, 14, 14) == -3
    assert call(7, 14, 13) == -1 and b"multiple" in L.srk_last_error()                    # SRK_E_SHAPE
    assert call(4, 14, 12) == -1
    assert call(7, 14, 14, shift=7) == -1
    torch.cuda.synchronize()


# ---- whole models ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(WSMALL))
def test_small_window_inference_vs_reference_golden(tag):
    """G17: SwinIR(window_size=7 / 4) -- the JPEG-artifact head '' (in_chans 1, img_range 255) and both pixel-shuffle heads at
    img_size, at a larger size (masks for the actual map) and at a size that needs reflect padding; T is not a multiple of 64."""
    g, cfg, sd = wsmall_weights(tag)
    m = build(cfg, sd)
    for hw in SIZES:
        x = torch.from_numpy(g[f"{tag}.x_{hw[0]}x{hw[1]}"]).cuda()
        with torch.no_grad():
            y = m(x).cpu()
        ref = torch.from_numpy(g[f"{tag}.y_{hw[0]}x{hw[1]}"])
        assert y.shape == ref.shape
        err = float((y - ref).abs().max())
        print(f"ws{cfg.window_size} {tag} {hw}: max err {err:.3e} (|ref| max {float(ref.abs().max()):.3f})")
        assert err <= 2e-2 * max(1.0, float(ref.abs().max())), (tag, hw)
    # eval mode without no_grad runs too (inference)
    y2 = m(torch.from_numpy(g[f"{tag}.x_14x14"]).cuda()).detach().cpu()
    assert float((y2 - torch.from_numpy(g[f"{tag}.y_14x14"])).abs().max()) <= 2e-2 * max(1.0, float(np.abs(g[f"{tag}.y_14x14"]).max()))


@pytest.mark.parametrize("upsampler,in_chans,upscale,img_range,size", [("", 1, 1, 255.0, 63), ("pixelshuffledirect", 3, 2, 1.0, 70)])
def test_small_window_at_width_180(upsampler, in_chans, upscale, img_range, size):
    """embed 180 / 6 heads (the SwinIR-M width of the JPEG models) at window 7, batch 8: 8 * 63^2 and 8 * 70^2 tokens are not multiples
    of 64, so the token rows are padded to a multiple of 64 for the persistent GEMMs and the fused MLP."""
    cfg = O.SwinIRConfig(upscale=upscale, in_chans=in_chans, img_size=size, window_size=7, img_range=img_range, depths=(2,), embed_dim=180,
                         num_heads=(6,), mlp_ratio=2, upsampler=upsampler, resi_connection="1conv")
    sd = O.random_state_dict(cfg, seed=7, scale=1.0)
    m = build(cfg, sd)
    x = torch.rand(8, in_chans, size, size, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        y = m(x.cuda()).cpu()
        want = O.swinir_forward(sd, cfg, x[:2])
    assert y.shape == (8, in_chans, size * upscale, size * upscale)
    assert not torch.isnan(y).any()
    err = float((y[:2] - want).abs().max())
    print(f"width 180 {upsampler!r} {size}: max err {err:.3e}")
    assert err <= 2e-2 * max(1.0, float(want.abs().max()))


def test_small_window_refusals():
    import tpu_superresolution_amd as T
    from tpu_superresolution_amd._lib import SrkUnsupported
    base = dict(img_size=14, in_chans=3, embed_dim=24, depths=[2], num_heads=[2], window_size=7, mlp_ratio=2, upscale=2, img_range=1.0,
                upsampler="pixelshuffle", resi_connection="1conv")
    x = torch.rand(1, 3, 14, 14, device="cuda")
    m = T.SwinIR(**base).cuda().train()
    with pytest.raises(SrkUnsupported, match="inference-only"):
        m(x)
    with torch.no_grad():
        assert m(x).shape == (1, 3, 28, 28)          # train mode under no_grad is inference
    for bad in (dict(upsampler="nearest+conv"), dict(resi_connection="3conv"), dict(img_size=7), dict(upsampler="", upscale=2)):
        mm = T.SwinIR(**{**base, **bad}).cuda().eval()
        with pytest.raises(SrkUnsupported):
            with torch.no_grad():
                mm(x)


def test_small_window_pack_follows_parameter_updates():
    """The bf16 pack is reused across calls only while no parameter has been written since it was made."""
    _, cfg, sd = wsmall_weights("ps")
    m = build(cfg, sd)
    x = torch.rand(2, 3, 14, 14, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        y1 = m(x).cpu()
        assert torch.equal(m(x).cpu(), y1)
        m.layers[0].residual_group.blocks[0].mlp.fc1.bias.add_(0.5)      # a packed (bf16) parameter
        y2 = m(x).cpu()
    key = "layers.0.residual_group.blocks.0.mlp.fc1.bias"
    sd2 = dict(sd, **{key: sd[key] + 0.5})
    want = O.swinir_forward(sd2, cfg, x.cpu())
    assert not torch.equal(y1, y2)
    assert float((y2 - want).abs().max()) <= 2e-2 * max(1.0, float(want.abs().max()))
