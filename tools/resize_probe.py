"""Developer probe: the antialiased bicubic resampler (csrc/resize.hip) where it is used.

1. The training batch: `DeviceHRPool.sample` (HR pool; one srk_crop_degrade_u8 launch crops the HR patches and filters their LR
   patches) beside `DevicePairPool.sample` (HR + LR pool made with PIL on the host; srk_paired_crop_u8, two copy launches) on the same
   24 gray 500 x 500 images (the DeepRockSR-2D image size), B 32, P 64, x2 and x4, augment none.
   - `sample_us`: host clock around `--calls` consecutive `sample` calls that ends in a device synchronise, per call: what a training
     loop pays per batch (descriptor upload, allocation, launch, kernel).  Blocks of the two pools alternate; median over `--repeats`.
   - `kernel_us`: the C entry alone on fixed descriptors between two HIP events, each bracket queued behind a ~100 us spin kernel so
     that it holds device time and not the host's enqueue gap; variants alternate launch by launch; median / min / max.
2. `ops.resize_aa` beside torch's `F.interpolate(mode='bicubic', antialias=True)` on the device, fp32 8 x 3 x 512 x 512 -> /2 and /4,
   bracketed the same way, plus the largest absolute difference of the two results.

Everything is warmed up first.  The tensors are small enough to stay in the 256 MiB Infinity Cache between launches: these are not HBM
rates.  There is no pass / fail threshold; a train step is hundreds of times longer than any figure here.

    python tools/resize_probe.py --out profiles/resize_probe.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd import ops  # noqa: E402
from tpu_superresolution_amd._lib import check, lib  # noqa: E402
from tpu_superresolution_amd.sr_datasets import DeviceHRPool, DevicePairPool  # noqa: E402


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def _bracketed(variants, launches, warmup, spin):
    """us per launch between two HIP events, variants alternating launch by launch."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in variants}
    for _ in range(launches):
        pairs = []
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(spin)
            e0.record()
            fn()
            e1.record()
            pairs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in pairs:
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: _stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200, help="sample calls per timed block")
    ap.add_argument("--repeats", type=int, default=7, help="timed blocks per pool")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    torch.cuda.set_device(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    e0.record()
    torch.cuda._sleep(1_000_000)
    e1.record()
    torch.cuda.synchronize()
    spin = max(1, int(1_000_000 * 0.1 / e0.elapsed_time(e1)))
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "calls_per_block": args.calls,
           "blocks": args.repeats, "spin_cycles_before_each_bracket": spin,
           "note": "sample_us: host clock around calls_per_block sample() calls ending in a synchronise, per call, median / min / max "
                   "over blocks, the two pools alternating; kernel_us and resize: us between two HIP events per launch, median / min / "
                   "max over launches, variants alternating; cache-resident tensors, not HBM rates",
           "pool": {}, "resize": {}}

    rng = np.random.RandomState(0)
    hrs = [(rng.rand(500, 500) * 255).astype(np.uint8) for _ in range(24)]
    B, P = 32, 64
    st = torch.cuda.current_stream().cuda_stream
    for s in (2, 4):
        pairs = [(np.asarray(Image.fromarray(a, "L").resize((500 // s, 500 // s), Image.BICUBIC)), a) for a in hrs]
        pools = {"hr_pool": DeviceHRPool(hrs, P, s), "pair_pool": DevicePairPool(pairs, P, s)}
        idx = [i % len(hrs) for i in range(B)]
        random.seed(0)
        for p in pools.values():
            for _ in range(args.warmup):
                p.sample(idx)
        torch.cuda.synchronize()
        blocks = {k: [] for k in pools}
        for _ in range(args.repeats):
            for k, p in pools.items():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    p.sample(idx)
                torch.cuda.synchronize()
                blocks[k].append((time.perf_counter() - t0) / args.calls * 1e6)
        # the C entries alone, on one fixed set of descriptors
        random.seed(1)
        hd, _ = pools["hr_pool"].draw(idx)
        hdesc = torch.tensor(hd, dtype=torch.int64).cuda()
        pm = pools["pair_pool"].meta
        pdesc = torch.tensor([pm[i][1] + (d[4] // s, d[5] // s) for i, d in zip(idx, hd)] + [pm[i][2] + (d[4], d[5]) for i, d in zip(idx, hd)],
                             dtype=torch.int64).cuda()
        lr, hr = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
        hp, pp = pools["hr_pool"].pool, pools["pair_pool"].pool
        kern = _bracketed({
            "crop_degrade_u8_q8": lambda: check(lib().srk_crop_degrade_u8(hp.data_ptr(), hdesc.data_ptr(), lr.data_ptr(), hr.data_ptr(), B, P, s, 8, st)),
            "crop_degrade_u8_q0": lambda: check(lib().srk_crop_degrade_u8(hp.data_ptr(), hdesc.data_ptr(), lr.data_ptr(), hr.data_ptr(), B, P, s, 0, st)),
            "paired_crop_u8": lambda: check(lib().srk_paired_crop_u8(pp.data_ptr(), pdesc[:B].data_ptr(), pdesc[B:].data_ptr(), lr.data_ptr(),
                                                                      hr.data_ptr(), B, P, s, st))}, args.launches, args.warmup, spin)
        res["pool"][f"x{s}"] = {"B": B, "lr_patch": P, "images": len(hrs), "image_size": [500, 500],
                                "pool_bytes": {k: int(p.pool.numel()) for k, p in pools.items()},
                                "sample_us": {k: _stats(v) for k, v in blocks.items()}, "kernel_us": kern}
        print(f"x{s}", json.dumps(res["pool"][f"x{s}"]), flush=True)

    x = torch.rand(8, 3, 512, 512, device="cuda")
    for s in (2, 4):
        size = (512 // s, 512 // s)
        out = torch.empty(8, 3, *size, device="cuda")
        r = _bracketed({"resize_aa": lambda: ops.resize_aa(x, size, out=out),
                        "torch_interpolate_aa": lambda: F.interpolate(x, size=size, mode="bicubic", antialias=True, align_corners=False)},
                       args.launches, args.warmup, spin)
        r["max_abs_diff"] = float((ops.resize_aa(x, size) - F.interpolate(x, size=size, mode="bicubic", antialias=True, align_corners=False)).abs().max())
        r["shape"] = [8, 3, 512, 512, *size]
        res["resize"][f"/{s}"] = r
        print(f"/{s}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
