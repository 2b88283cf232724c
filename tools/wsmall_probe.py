"""Timing probe of SwinIR with small windows (HIP events, MI355X): prints one JSON document.

    python tools/wsmall_probe.py [--out FILE]
    python tools/wsmall_probe.py --train [--out profiles/r05_wsmall_train_probe.json]

(a) the small-window attention kernel (srk_win_small_attention_fwd, ws 7, raster qkv) against the 8 x 8 window kernel
    (srk_window_attention_fwd, window-order qkv) at equal token count and heads (embed 180, 6 heads, a 56 x 56 map, batch 32; shift 0 and
    ws // 2), reported per token;
(b) whole-model eval forwards: classical x4 (embed 180, depths 6 x 6, heads 6, mlp 2, pixelshuffle) at ws 7 on 63 x 63 LR against ws 8 on
    64 x 64 LR, batch 32, reported per HR pixel, and the JPEG-artifact configuration (ws 7, '', in_chans 3, upscale 1, img_range 255) on
    126 x 126, batch 8.
With --train (training at window 7, SwinIR.enable_small_window_training):
(c) the small-window attention backward (srk_win_small_attention_bwd, ws 7) against the 64-token attn_bwd_kernel
    (srk_window_attention_bwd) at the same token count, shift 0 and ws // 2;
(d) the ws 7 train step (classical x4, batch 32, 63 x 63 LR; forward + L1 + backward + FusedAdamW) launched eagerly and replayed as a
    graph (training.GraphedTrainStep), against the ws 8 engine step on 64 x 64 LR, reported per HR pixel.
The kernel-source digest is computed as bench.py does, so a stored result names the library it was measured on.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tpu_superresolution_amd as T  # noqa: E402
from bench import kernels_digest  # noqa: E402
from oracle import swinir_oracle as O  # noqa: E402
from tpu_superresolution_amd import ops  # noqa: E402


def time_ms(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_leg(iters: int) -> dict:
    B, H, W, nH, dh = 32, 56, 56, 6, 30
    T_ = B * H * W
    CA = nH * 32
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv_raster = torch.randn(T_, 3 * CA, device="cuda", generator=g).to(torch.bfloat16)
    table7 = torch.randn(13 * 13, nH, device="cuda", generator=g)
    qkv_win = torch.randn(3, T_ // 64, nH, 64, 32, device="cuda", generator=g).to(torch.bfloat16)
    bias8 = torch.randn(nH, 64, 64, device="cuda", generator=g)
    out = {}
    for shift7, shift8 in ((0, 0), (3, 4)):
        t7 = time_ms(lambda: ops.window_attention_small_fwd(qkv_raster, table7, B, H, W, 7, shift7, nH, dh ** -0.5), 5, iters)
        t8 = time_ms(lambda: ops.window_attention_fwd(qkv_win, bias8, H, W, shift8), 5, iters)
        out[f"shift_{shift7}_{shift8}"] = dict(ws7_ms=round(t7, 4), ws8_ms=round(t8, 4), ws7_ns_per_token=round(t7 * 1e6 / T_, 4),
                                              ws8_ns_per_token=round(t8 * 1e6 / T_, 4), ratio=round(t7 / t8, 3))
    return dict(tokens=T_, heads=nH, map=[H, W], batch=B, **out)


def model_ms(cfg: O.SwinIRConfig, B: int, size: int, iters: int) -> float:
    torch.manual_seed(0)
    m = T.SwinIR(drop_path_rate=0.0, **cfg.kwargs()).cuda().eval()
    x = torch.rand(B, cfg.in_chans, size, size, device="cuda")
    with torch.no_grad():
        return time_ms(lambda: m(x), 2, iters)


def model_leg(iters: int) -> dict:
    classical = dict(in_chans=3, embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, mlp_ratio=2, upscale=4, img_range=1.0,
                     upsampler="pixelshuffle", resi_connection="1conv")
    t7 = model_ms(O.SwinIRConfig(img_size=63, window_size=7, **classical), 32, 63, iters)
    t8 = model_ms(O.SwinIRConfig(img_size=64, window_size=8, **classical), 32, 64, iters)
    px7, px8 = 32 * (63 * 4) ** 2, 32 * (64 * 4) ** 2
    jpeg = O.SwinIRConfig(img_size=126, in_chans=3, embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, window_size=7, mlp_ratio=2,
                          upscale=1, img_range=255.0, upsampler="", resi_connection="1conv")
    tj = model_ms(jpeg, 8, 126, iters)
    return dict(classical_x4=dict(ws7_63x63_bs32_ms=round(t7, 3), ws8_64x64_bs32_ms=round(t8, 3), ws7_ns_per_hr_pixel=round(t7 * 1e6 / px7, 4),
                                  ws8_ns_per_hr_pixel=round(t8 * 1e6 / px8, 4), ratio_per_hr_pixel=round((t7 / px7) / (t8 / px8), 3)),
                jpeg_ws7_126x126_bs8_ms=round(tj, 3))


def kernel_bwd_leg(iters: int) -> dict:
    B, H, W, nH, dh = 32, 56, 56, 6, 30
    T_ = B * H * W
    CA = nH * 32
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv_raster = torch.randn(T_, 3 * CA, device="cuda", generator=g).to(torch.bfloat16)
    dout_raster = torch.randn(T_, CA, device="cuda", generator=g).to(torch.bfloat16)
    table7 = torch.randn(13 * 13, nH, device="cuda", generator=g)
    qkv_win = torch.randn(3, T_ // 64, nH, 64, 32, device="cuda", generator=g).to(torch.bfloat16)
    dout_win = torch.randn(T_, CA, device="cuda", generator=g).to(torch.bfloat16)
    bias8 = torch.randn(nH, 64, 64, device="cuda", generator=g)
    out = {}
    for shift7, shift8 in ((0, 0), (3, 4)):
        t7 = time_ms(lambda: ops.window_attention_small_bwd(qkv_raster, table7, dout_raster, B, H, W, 7, shift7, nH, dh ** -0.5), 5, iters)
        t8 = time_ms(lambda: ops.window_attention_bwd(qkv_win, bias8, dout_win, dh ** -0.5, H, W, shift8), 5, iters)
        out[f"shift_{shift7}_{shift8}"] = dict(ws7_ms=round(t7, 4), ws8_ms=round(t8, 4), ws7_ns_per_token=round(t7 * 1e6 / T_, 4),
                                              ws8_ns_per_token=round(t8 * 1e6 / T_, 4), ratio=round(t7 / t8, 3))
    return dict(tokens=T_, heads=nH, map=[H, W], batch=B, note="both sides include the wrappers' allocations and the table reduction", **out)


def train_leg(iters: int) -> dict:
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import GraphedTrainStep, l1_loss_checked
    classical = dict(in_chans=3, embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, mlp_ratio=2, upscale=4, img_range=1.0,
                     upsampler="pixelshuffle", resi_connection="1conv")

    def setup(ws, size):
        torch.manual_seed(0)
        m = T.SwinIR(**O.SwinIRConfig(img_size=size, window_size=ws, **classical).kwargs()).cuda().train()
        if ws < 8:
            m.enable_small_window_training()
        opt = FusedAdamW(m, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0)
        x, t = torch.rand(32, 3, size, size, device="cuda"), torch.rand(32, 3, size * 4, size * 4, device="cuda")

        def step():
            opt.zero_grad(set_to_none=True)
            loss, bad = l1_loss_checked(m(x), t)
            loss.backward()
            opt.step(nonfinite=bad)
        return m, opt, x, t, step
    m7, o7, x7, t7, step7 = setup(7, 63)
    eager7 = time_ms(step7, 2, iters)
    gs = GraphedTrainStep(m7, o7, warmup=1)
    graph7 = time_ms(lambda: gs(x7, t7), 2, iters)
    gs.close()
    del m7, o7, gs
    torch.cuda.empty_cache()
    _, _, _, _, step8 = setup(8, 64)
    eager8 = time_ms(step8, 2, iters)
    px7, px8 = 32 * (63 * 4) ** 2, 32 * (64 * 4) ** 2
    return dict(classical_x4_bs32=dict(ws7_63x63_eager_ms=round(eager7, 3), ws7_63x63_graphed_ms=round(graph7, 3), ws8_64x64_engine_ms=round(eager8, 3),
                                       ratio_eager_per_hr_pixel=round((eager7 / px7) / (eager8 / px8), 3),
                                       ratio_graphed_per_hr_pixel=round((graph7 / px7) / (eager8 / px8), 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true", help="measure the training legs (c), (d) instead of the inference legs")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.train:
        res = dict(probe="wsmall_train", device=torch.cuda.get_device_name(0), kernels_digest=kernels_digest(),
                   kernel_bwd=kernel_bwd_leg(max(a.iters, 20)), train=train_leg(min(a.iters, 10)))
    else:
        res = dict(probe="wsmall", device=torch.cuda.get_device_name(0), kernels_digest=kernels_digest(),
                   kernel=kernel_leg(max(a.iters, 20)), model=model_leg(a.iters))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
