"""Developer probe: blur and sinc tables built on the device (csrc/tables.hip) where training uses them.

The training batch of tools/degrade2_probe.py: 24 gray 500 x 500 images, B 32, P 64, x4, augment none, margin 8.
   - `sample_us`: host clock around `--calls` consecutive `sample` calls that end in a device synchronise, per call, for
     DeviceHR2Pool(SecondOrderSpec(), DegradeSpec()) and for DeviceHRPool(degrade=DegradeSpec(), psf=PsfSpec("mixed")), each with
     tables="host" and tables="device" in ONE process: `--rounds` rounds of `--repeats` blocks per setting, the settings alternating
     block by block and their order reversed every round (the scheme of tools/ab.sh).  The host setting is the yardstick: it is what
     the pool did before the option existed.  A gain counts when the device setting's median lies outside the host setting's own
     round-to-round range.
   - `draw_us`: the host clock around the draws alone (`draw` + `draw_second_order` / `draw_psf` without the launches: descriptors or
     tables), the part of a `sample` call that the training thread spends before anything is queued.
   - `kernel_us`: srk_kernel_tables_f32 alone, 32 tables of 21 x 21 -- all sinc, all generalized, all delta -- between two HIP events,
     each bracket queued behind a ~100 us spin kernel; variants alternate launch by launch; median / min / max over `--launches`.
Everything is warmed up first.  There is no pass / fail threshold.

    python tools/tables_probe.py --out profiles/tables_probe.json
"""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG3_STEP_MS = 27.7          # the cfg3 train step of DESIGN.md (7n "Time")
CHAIN_DEVICE_MS = 2.5        # the chain's own device time (7p "Time")


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def _images():
    import numpy as np
    rng = np.random.RandomState(0)
    return [(rng.rand(500, 500) * 255).astype(np.uint8) for _ in range(24)]


def _rounds(pools, idx, calls, repeats, rounds, warmup, fn):
    """{setting: [one median per round]} and every block, the settings alternating, the order reversed every round."""
    import torch
    random.seed(0)
    for p in pools.values():
        for _ in range(warmup):
            fn(p, idx)
    torch.cuda.synchronize()
    per_round, blocks = {k: [] for k in pools}, {k: [] for k in pools}
    for rnd in range(rounds):
        order = list(pools) if rnd % 2 == 0 else list(pools)[::-1]
        mine = {k: [] for k in pools}
        for _ in range(repeats):
            for k in order:
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn(pools[k], idx)
                torch.cuda.synchronize()
                mine[k].append((time.perf_counter() - t0) / calls * 1e6)
        for k in pools:
            per_round[k].append(round(statistics.median(mine[k]), 2))
            blocks[k] += mine[k]
    return per_round, blocks


def _verdict(per_round):
    lo, hi = min(per_round["host"]), max(per_round["host"])
    md, mh = statistics.median(per_round["device"]), statistics.median(per_round["host"])
    return {"round_median_us": per_round, "median_of_round_medians_us": {"host": round(mh, 2), "device": round(md, 2)},
            "host_round_to_round_range_us": [lo, hi], "device_below_the_hosts_range": bool(md < lo), "gain_us": round(mh - md, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="sample calls per timed block")
    ap.add_argument("--repeats", type=int, default=3, help="timed blocks per setting and round")
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    sys.path.insert(0, ROOT)
    import torch
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd._lib import check, lib
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHR2Pool, DeviceHRPool, PsfSpec, SecondOrderSpec
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    e0.record()
    torch.cuda._sleep(1_000_000)
    e1.record()
    torch.cuda.synchronize()
    spin = max(1, int(1_000_000 * 0.1 / e0.elapsed_time(e1)))
    B, P, s, m = 32, 64, 4, 8
    hrs = _images()
    idx = [i % len(hrs) for i in range(B)]
    st = torch.cuda.current_stream().cuda_stream
    TD = bk.TableDesc

    # the launch alone
    sets = {"sinc": [TD.sinc(math.pi / 5 + 0.08 * b, 21) for b in range(B)],
            "generalized": [TD.generalized(21, 0.5 + 0.07 * b, 2.5 - 0.05 * b, 0.1 * b, 0.5 + 0.1 * b) for b in range(B)],
            "delta": [TD.delta(21)] * B}
    variants = {}
    for name, ds in sets.items():
        desc = torch.tensor([d.row() for d in ds], dtype=torch.float64).cuda()
        tab = torch.empty(B, 21, 21, device="cuda")
        variants[f"kernel_tables_32x21x21_{name}"] = lambda desc=desc, tab=tab: check(
            lib().srk_kernel_tables_f32(desc.data_ptr(), None, 0, 0, tab.data_ptr(), B, 21, st))
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.launches):
        pairs = []
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(spin)
            a.record()
            fn()
            b.record()
            pairs.append((k, a, b))
        torch.cuda.synchronize()
        for k, a, b in pairs:
            times[k].append(a.elapsed_time(b) * 1e3)
    # the same 32 sinc tables on the host, as the pool's host setting makes them
    host_sinc = []
    for _ in range(5):
        t0 = time.perf_counter()
        for d in sets["sinc"]:
            d.table()
        host_sinc.append((time.perf_counter() - t0) * 1e6)

    hr2 = {t: DeviceHR2Pool(hrs, P, s, SecondOrderSpec(), DegradeSpec(), margin=m, tables=t) for t in ("host", "device")}
    hr1 = {t: DeviceHRPool(hrs, P, s, degrade=DegradeSpec(), psf=PsfSpec("mixed"), tables=t) for t in ("host", "device")}
    sample = lambda p, i: p.sample(i)          # noqa: E731
    r2, b2 = _rounds(hr2, idx, args.calls, args.repeats, args.rounds, args.warmup, sample)
    r1, b1 = _rounds(hr1, idx, args.calls, args.repeats, args.rounds, args.warmup, sample)
    d2, _ = _rounds(hr2, idx, args.calls, args.repeats, args.rounds, 1, lambda p, i: p.draw_second_order(p.draw(i)[0]))
    d1, _ = _rounds(hr1, idx, args.calls, args.repeats, args.rounds, 1, lambda p, i: p.draw_psf(p.draw(i)[0]))
    v2, v1 = _verdict(r2), _verdict(r1)
    left = v2["median_of_round_medians_us"]["device"]
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "calls_per_block": args.calls,
           "blocks_per_setting_and_round": args.repeats, "rounds": args.rounds, "spin_cycles_before_each_bracket": spin, "B": B, "lr_patch": P,
           "scale": s, "margin": m,
           "note": "sample_us / draw_us: host clock around calls_per_block calls ending in a synchronise, per call; one process, the host "
                   "and device settings alternating block by block, the order reversed every round; round_median_us = the median of a "
                   "round's blocks.  draw_us of DeviceHRPool's device setting includes its kernel_tables launch (draw_psf makes the "
                   "tables).  kernel_us: us between two HIP events per launch, median / min / max over launches, variants alternating",
           "kernel_us": {k: _stats(v) for k, v in times.items()}, "host_32_sinc_tables_21_us": _stats(host_sinc),
           "sample_us": {"DeviceHR2Pool": {**v2, "blocks": {k: _stats(v) for k, v in b2.items()}},
                         "DeviceHRPool_mixed": {**v1, "blocks": {k: _stats(v) for k, v in b1.items()}}},
           "draw_us": {"DeviceHR2Pool": _verdict(d2), "DeviceHRPool_mixed": _verdict(d1)},
           "cfg3_train_step_ms": CFG3_STEP_MS, "chain_device_ms": CHAIN_DEVICE_MS,
           "DeviceHR2Pool_device_sample_share_of_cfg3_step_percent": round(100.0 * left / (CFG3_STEP_MS * 1e3), 2),
           "DeviceHR2Pool_device_sample_below_cfg3_step": bool(left < CFG3_STEP_MS * 1e3)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
