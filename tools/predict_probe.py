"""Developer probe: the two image I/O kernels (csrc/image_io.hip) alone, and their share of one `predict` pass.

Part 1, kernels alone, RGB at B = 1: `unpack` (8-bit interleaved samples -> planar fp32) at 512 x 512 and 2048 x 2048; `pack` (planar
fp32 -> 8- and 16-bit interleaved samples, counters on) at the same two sizes.  Beside each launch:
  (a) `copy_as_<k>`: a device-to-device `copy_` of the same byte count (what the launch reads plus writes, counted from the shapes);
  (b) `host_form_<k>`: the host form the launch replaces, timed on the same machine with a host clock -- for pack the fp32 download plus the
      numpy clamp / x max / rint / transpose to HWC; for unpack the numpy / max and transpose to CHW plus the fp32 upload -- beside the
      device form end to end (`device_form_<k>`: the launch plus the 8- / 16-bit copy over the bus).
Kernel launches are bracketed by HIP events behind a spin kernel (as tools/tile_probe.py), variants alternating, median / min / max of
`--launches`.  The comparison is against (a) and (b), never against an earlier run of these kernels.

Part 2: `predict.upscale` on one decoded RGB image in memory (no PNG codec) -- SwinIR-light x2 (bench.py's cfg2) on 256 x 256 and the
full-size SwinIR x4 (finetune_swinir.build_model) on 512 x 512 -- host-clocked around the pass, median of `--passes`; the same pass with
the model replaced by a stub that returns a ready tensor gives the I/O part (upload, unpack, pack, download, counter read), and their
ratio is the share of a pass that I/O takes.

    python tools/predict_probe.py --out profiles/predict_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from tpu_superresolution_amd import ops  # noqa: E402
from tpu_superresolution_amd import predict as P  # noqa: E402

from tile_probe import host_clocked, time_variants  # noqa: E402  (tools/tile_probe.py: the protocol is shared, not restated)


def _stats(v, nbytes=None):
    med = statistics.median(v)
    out = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    if nbytes is not None:
        out.update(bytes=nbytes, tb_per_s=round(nbytes / med / 1e6, 3))
    return out


def kernels_alone(side, launches, warmup, host_passes):
    g = torch.Generator().manual_seed(side)
    a = torch.randint(0, 256, (1, side, side, 3), dtype=torch.uint8, generator=g)
    y = torch.rand(1, 3, side, side, generator=g) * 1.2 - 0.1
    a_dev, y_dev = a.cuda(), y.cuda()
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    px = side * side * 3
    moved = {"unpack_8": px * (1 + 4), "pack_8": px * (4 + 1), "pack_16": px * (4 + 2)}
    variants = {"unpack_8": lambda: ops.image_unpack(a_dev, 3), "pack_8": lambda: ops.image_pack(y_dev, bits=8, counters=cnt),
                "pack_16": lambda: ops.image_pack(y_dev, bits=16, counters=cnt)}
    for name, nbytes in list(moved.items()):
        src = torch.randint(0, 256, (nbytes // 2,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        variants[f"copy_as_{name}"] = (lambda src=src, dst=dst: dst.copy_(src))
    times = time_variants(variants, launches, warmup)
    res = {"side": side, "channels": 3, "variants": {}, "host_clocked_ms": {}}
    for name, v in times.items():
        res["variants"][name] = _stats(v, moved[name.replace("copy_as_", "")])
        print(f"{side} x {side} x 3  {name:18s} {res['variants'][name]}", flush=True)
    for k in ("unpack_8", "pack_8", "pack_16"):
        res["variants"][k]["over_its_copy"] = round(res["variants"][k]["median_us"] / res["variants"][f"copy_as_{k}"]["median_us"], 2)

    # (b) the host forms, end to end, beside the device forms end to end
    def host_pack(mx, dtype):
        v = y_dev.cpu().numpy()                                             # the fp32 download
        q = np.rint(np.clip(v, 0.0, 1.0) * np.float32(mx)).astype(dtype)
        return np.ascontiguousarray(q[0].transpose(1, 2, 0))

    def host_unpack():
        v = (a.numpy()[0].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
        return torch.from_numpy(np.ascontiguousarray(v))[None].cuda()     # the fp32 upload

    forms = {"host_form_pack_8": lambda: host_pack(255, np.uint8), "device_form_pack_8": lambda: ops.image_pack(y_dev, bits=8, counters=cnt).cpu(),
             "host_form_pack_16": lambda: host_pack(65535, np.uint16), "device_form_pack_16": lambda: ops.image_pack(y_dev, bits=16, counters=cnt).cpu(),
             "host_form_unpack_8": host_unpack, "device_form_unpack_8": lambda: ops.image_unpack(a.cuda(), 3)}
    for name, fn in forms.items():
        res["host_clocked_ms"][name] = host_clocked(fn, host_passes, 2)
        print(f"{side} x {side} x 3  {name:22s} {res['host_clocked_ms'][name]}", flush=True)
    return res


def predict_pass(name, model, scale, side, passes):
    g = np.random.default_rng(side)
    a = g.integers(0, 256, size=(side, side, 3), dtype=np.uint8)
    ready = torch.rand(1, 3, side * scale, side * scale, device="cuda")
    quiet = lambda s: None
    res = {"model": name, "side": side, "scale": scale, "passes": passes}
    with torch.no_grad():
        x = ops.image_unpack(torch.from_numpy(a[None]).cuda(), 3)[0]
        res["model_alone"] = host_clocked(lambda: model(x), passes, 2)
        res["upscale"] = host_clocked(lambda: P.upscale(model, [a], scale=scale, device="cuda", log=quiet), passes, 2)
        res["upscale_with_a_stub_model"] = host_clocked(lambda: P.upscale(lambda t: ready, [a], scale=scale, device="cuda", log=quiet), passes, 2)
    res["io_share_of_a_pass"] = round(res["upscale_with_a_stub_model"]["median_ms"] / res["upscale"]["median_ms"], 4)
    print(f"{name}: {res}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--host_passes", type=int, default=5)
    ap.add_argument("--skip_full_size", action="store_true", help="leave out the full-size SwinIR x4 pass")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup,
           "note": "kernels_alone.variants: us per launch between two HIP events, median / min / max, variants alternating; bytes = what the "
                   "launch reads plus writes, counted from the shapes; tb_per_s = bytes / median; copy_as_<k> is a device-to-device copy_ of the "
                   "same byte count; over_its_copy = launch median / copy median.  Buffers below 256 MiB stay in the Infinity Cache between "
                   "launches, for the copy as for the kernel: compare a kernel with its copy, not with HBM.  host_clocked_ms: ms per call, host "
                   "clock around a device synchronise; host_form_* = the numpy form with its fp32 transfer, device_form_* = the launch with its "
                   "8- / 16-bit transfer (pageable host memory both ways).  predict: ms per pass of predict.upscale on one decoded image; "
                   "io_share_of_a_pass = the pass with a stub model / the pass with the model",
           "kernels_alone": [], "predict": []}
    for side in (512, 2048):
        res["kernels_alone"].append(kernels_alone(side, args.launches, args.warmup, args.host_passes))
    import tpu_superresolution_amd as pkg
    from tpu_superresolution_amd.finetune_swinir import build_model
    torch.manual_seed(42)
    light = pkg.SwinIR(upscale=2, in_chans=3, img_size=64, window_size=8, img_range=1.0, depths=[6] * 4, embed_dim=60, num_heads=[6] * 4,
                       mlp_ratio=2, upsampler="pixelshuffledirect").cuda().eval()
    res["predict"].append(predict_pass("SwinIR-light x2 (bench.py cfg2)", light, 2, 256, args.passes))
    if not args.skip_full_size:
        full = build_model(4, drop_path_rate=0.0).cuda().eval()
        res["predict"].append(predict_pass("SwinIR x4 (finetune_swinir.build_model)", full, 4, 512, max(3, args.passes // 2)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
