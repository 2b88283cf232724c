"""Developer probe: the blind degradation (csrc/degrade.hip) beside the clean one (csrc/resize.hip), where training uses them.

The training batch of tools/resize_probe.py: 24 gray 500 x 500 images (the DeepRockSR-2D image size), B 32, P 64, x2 and x4, augment none.
   - `kernel_us`: the C entries alone on one fixed set of descriptors between two HIP events, each bracket queued behind a ~100 us spin
     kernel so that it holds device time and not the host's enqueue gap; variants alternate launch by launch; median / min / max.
     `crop_degrade_blind_u8_worst`: sigma = 2.5 on both axes (R = 8, the widest composed tables) plus noise (sigma_n 10 / 255, gain
     0.01); `crop_degrade_blind_u8_off`: the same entry with both sigmas and the noise at 0 (the bits of srk_crop_degrade_u8);
     `crop_degrade_u8`: the clean entry.  All with the 8-bit rounding.
   - `sample_us`: host clock around `--calls` consecutive `DeviceHRPool.sample` calls that end in a device synchronise, per call, with
     and without a DegradeSpec (default ranges); blocks of the two pools alternate; median / min / max over `--repeats`.

`SRK_LIB_PATH` selects the library, so the same probe measures a library built from another commit (tools/ab.sh alternates whole
benchmark runs the same way); `--only_clean` restricts it to the entries such a library has.  Everything is warmed up first.  The tensors
stay in the 256 MiB Infinity Cache between launches: these are not HBM rates.  There is no pass / fail threshold; a train step is
hundreds of times longer than any figure here.

    python tools/degrade_probe.py --out profiles/degrade_probe.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200, help="sample calls per timed block")
    ap.add_argument("--repeats", type=int, default=7, help="timed blocks per pool")
    ap.add_argument("--only_clean", action="store_true", help="measure srk_crop_degrade_u8 and the plain pool only (a library without the blind entries)")
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
    res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SRK_LIB_PATH", "in-tree"), "launches": args.launches,
           "warmup": args.warmup, "calls_per_block": args.calls, "blocks": args.repeats, "spin_cycles_before_each_bracket": spin,
           "note": "kernel_us: us between two HIP events per launch, median / min / max over launches, variants alternating; sample_us: "
                   "host clock around calls_per_block sample() calls ending in a synchronise, per call, median / min / max over blocks, "
                   "the pools alternating; cache-resident tensors, not HBM rates",
           "pool": {}}

    rng = np.random.RandomState(0)
    hrs = [(rng.rand(500, 500) * 255).astype(np.uint8) for _ in range(24)]
    B, P = 32, 64
    st = torch.cuda.current_stream().cuda_stream
    for s in (2, 4):
        pools = {"plain": DeviceHRPool(hrs, P, s)}
        if not args.only_clean:
            from tpu_superresolution_amd.ops import pack_degrade_params
            from tpu_superresolution_amd.sr_datasets import DegradeSpec
            pools["blind"] = DeviceHRPool(hrs, P, s, degrade=DegradeSpec())
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
        random.seed(1)
        hd, _ = pools["plain"].draw(idx)
        hdesc = torch.tensor(hd, dtype=torch.int64).cuda()
        lr, hr = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
        hp = pools["plain"].pool
        variants = {"crop_degrade_u8": lambda: check(lib().srk_crop_degrade_u8(hp.data_ptr(), hdesc.data_ptr(), lr.data_ptr(), hr.data_ptr(), B, P, s, 8, st))}
        if not args.only_clean:
            worst = torch.tensor([d + tuple(pack_degrade_params((2.5, 2.5), (10.0 / 255.0, 0.01), i, True)) for i, d in enumerate(hd)], dtype=torch.int64).cuda()
            off = torch.tensor([d + tuple(pack_degrade_params((0.0, 0.0), (0.0, 0.0), i, True)) for i, d in enumerate(hd)], dtype=torch.int64).cuda()
            variants["crop_degrade_blind_u8_worst"] = lambda: check(lib().srk_crop_degrade_blind_u8(hp.data_ptr(), worst.data_ptr(), lr.data_ptr(), hr.data_ptr(), B, P, s, 8, st))
            variants["crop_degrade_blind_u8_off"] = lambda: check(lib().srk_crop_degrade_blind_u8(hp.data_ptr(), off.data_ptr(), lr.data_ptr(), hr.data_ptr(), B, P, s, 8, st))
        kern = _bracketed(variants, args.launches, args.warmup, spin)
        res["pool"][f"x{s}"] = {"B": B, "lr_patch": P, "images": len(hrs), "image_size": [500, 500],
                                "sample_us": {k: _stats(v) for k, v in blocks.items()}, "kernel_us": kern}
        print(f"x{s}", json.dumps(res["pool"][f"x{s}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
