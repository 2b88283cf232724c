"""Developer probe: the JPEG round trip (csrc/jpeg.hip) where training uses it.

The training batch of tools/degrade_probe.py: 24 gray 500 x 500 images, B 32, P 64, x2 and x4, augment none.
   - `kernel_us`: srk_jpeg_roundtrip_f32 alone on one fixed LR batch [32, C, 64, 64] between two HIP events, each bracket queued behind a
     ~100 us spin kernel so that it holds device time and not the host's enqueue gap; gray (C 1) and colour (C 3) at 4:4:4 and 4:2:0,
     quality 75 in every sample, plus the pass-through (quality 0); variants alternate launch by launch; median / min / max.
   - `sample_us`: host clock around ONE `DeviceHRPool.sample` call that ends in a device synchronise, with and without a JpegSpec
     (default range, p = 1), the two pools alternating call by call; median / min / max over `--calls`.
   - `--only_plain`: the pool without `jpeg=` alone, in blocks like tools/degrade_probe.py.  It needs nothing this stage added, so
     the same file runs inside a checkout of an earlier commit: alternate the two processes to see that the unchanged path kept its time.

Everything is warmed up first.  The tensors stay in the 256 MiB Infinity Cache between launches: these are not HBM rates.  There is no
pass / fail threshold; a train step is hundreds of times longer than any figure here.

    python tools/jpeg_probe.py --out profiles/jpeg_probe.json
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd._lib import check, lib  # noqa: E402
from tpu_superresolution_amd.sr_datasets import DeviceHRPool  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=300, help="timed sample calls per pool")
    ap.add_argument("--repeats", type=int, default=5, help="--only_plain: timed blocks of --calls calls")
    ap.add_argument("--label", default="in-tree", help="what the result file calls the measured tree")
    ap.add_argument("--only_plain", action="store_true", help="measure the pool without jpeg= only (runs in a checkout without the stage)")
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
    res = {"device": torch.cuda.get_device_name(0), "tree": args.label, "launches": args.launches,
           "warmup": args.warmup, "calls": args.calls, "spin_cycles_before_each_bracket": spin,
           "note": "kernel_us: us between two HIP events per launch, median / min / max over launches, variants alternating; sample_us: host "
                   "clock around one sample() call ending in a synchronise, pools alternating call by call (--only_plain: per call over "
                   "blocks of calls); cache-resident tensors, not HBM rates",
           "pool": {}}

    rng = np.random.RandomState(0)
    hrs = [(rng.rand(500, 500) * 255).astype(np.uint8) for _ in range(24)]
    B, P = 32, 64
    idx = [i % len(hrs) for i in range(B)]
    for s in (2, 4):
        pools = {"plain": DeviceHRPool(hrs, P, s)}
        if not args.only_plain:
            from tpu_superresolution_amd.sr_datasets import JpegSpec
            pools["jpeg_444"] = DeviceHRPool(hrs, P, s, jpeg=JpegSpec())
            pools["jpeg_420"] = DeviceHRPool(hrs, P, s, jpeg=JpegSpec(subsample=True))
        random.seed(0)
        for p in pools.values():
            for _ in range(args.warmup):
                p.sample(idx)
        torch.cuda.synchronize()
        calls = {k: [] for k in pools}
        if args.only_plain:
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    pools["plain"].sample(idx)
                torch.cuda.synchronize()
                calls["plain"].append((time.perf_counter() - t0) / args.calls * 1e6)
        else:
            for _ in range(args.calls):
                for k, p in pools.items():
                    t0 = time.perf_counter()
                    p.sample(idx)
                    torch.cuda.synchronize()
                    calls[k].append((time.perf_counter() - t0) * 1e6)
        res["pool"][f"x{s}"] = {"B": B, "lr_patch": P, "images": len(hrs), "image_size": [500, 500], "sample_us": {k: _stats(v) for k, v in calls.items()}}
        print(f"x{s}", json.dumps(res["pool"][f"x{s}"]), flush=True)

    if not args.only_plain:
        st = torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(0)
        variants = {}
        keep = []
        for name, C, sub, q in (("gray", 1, 0, 75), ("colour_444", 3, 0, 75), ("colour_420", 3, 1, 75), ("colour_pass_through", 3, 0, 0)):
            x = (torch.randint(0, 256, (B, C, P, P), generator=g).float() / 255.0).cuda()
            out, qd = torch.empty_like(x), torch.full((B,), q, dtype=torch.int32).cuda()
            keep.append((x, out, qd))
            variants[name] = (lambda x=x, out=out, qd=qd, C=C, sub=sub:
                              check(lib().srk_jpeg_roundtrip_f32(x.data_ptr(), out.data_ptr(), qd.data_ptr(), B, C, P, P, sub, None, st)))
        res["kernel_us"] = {"batch": [B, "C", P, P], **_bracketed(variants, args.launches, args.warmup, spin)}
        print("kernel_us", json.dumps(res["kernel_us"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
