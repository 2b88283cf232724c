"""Developer probe: the USM target and the resize rules (csrc/usm.hip, csrc/resize_modes.hip) where training uses them.

The training batch of tools/degrade2_probe.py: 24 gray 500 x 500 images, B 32, P 64, x4, augment none; margin 8, so the chain runs on
windows of E = 4 (64 + 16) = 320 HR pixels.
   - `kernel_us`: each C entry alone on one fixed set of operands between two HIP events, each bracket queued behind a ~100 us spin kernel
     so that it holds device time and not the host's enqueue gap; variants alternate launch by launch; median / min / max over
     `--launches` launches.  srk_usm_sharpen_f32 (two launches) at B 32, C 3, 320 x 320 and 256 x 256; srk_resize_ragged_mode_f32 with every
     sample at mode 0, 1, 2 beside srk_resize_aa_ragged_f32 on the three resizes of the 7p probe (the extents of 32 draws of the default
     SecondOrderSpec).
   - `sample_us`: host clock around `--calls` consecutive `sample` calls that end in a device synchronise, per call, for DeviceHR2Pool
     plain, with usm=UsmSpec(), and with usm and resize_mode_prob (0.3, 0.3, 0.4); blocks of the pools alternate.
   - `--ab_tree DIR` (after the above, or alone with `--ab_only`): `DeviceHR2Pool.sample` WITHOUT a new option in this tree and in the tree at
     DIR (a checkout of the parent commit with its library built), each in a fresh child process, four rounds, the order reversed every
     round: the scheme of tools/ab.sh.  `--ab_tables device` runs both trees with the tables built on the device.
Everything is warmed up first.  The tensors stay in the 256 MiB Infinity Cache between launches: these are not HBM rates.  There is no
pass / fail threshold.

    python tools/usm_probe.py --out profiles/usm_probe.json [--ab_tree ../parent --ab_out profiles/usm_probe_ab.json]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG3_STEP_MS = 27.7          # the cfg3 train step of DESIGN.md (7n "Time")


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def _images():
    import numpy as np
    rng = np.random.RandomState(0)
    return [(rng.rand(500, 500) * 255).astype(np.uint8) for _ in range(24)]


def _sample_blocks(pools, idx, calls, repeats, warmup):
    import torch
    random.seed(0)
    for p in pools.values():
        for _ in range(warmup):
            p.sample(idx)
    torch.cuda.synchronize()
    blocks = {k: [] for k in pools}
    for _ in range(repeats):
        for k, p in pools.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                p.sample(idx)
            torch.cuda.synchronize()
            blocks[k].append((time.perf_counter() - t0) / calls * 1e6)
    return blocks


def sample_only(tree, calls, repeats, warmup, tables):
    """One child run of the A/B: `sample` of the second-order pool of the package under `tree` at x4, no new option -> one JSON line."""
    sys.path.insert(0, tree)
    import torch
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHR2Pool, SecondOrderSpec
    torch.cuda.set_device(0)
    pool = DeviceHR2Pool(_images(), 64, 4, SecondOrderSpec(), DegradeSpec(), margin=8, tables=tables)
    blocks = _sample_blocks({"second_order": pool}, [i % 24 for i in range(32)], calls, repeats, warmup)
    print("AB " + json.dumps(blocks["second_order"]), flush=True)


def ab(args):
    trees = {"branch": ROOT, "parent": os.path.abspath(args.ab_tree)}
    rounds = {k: [] for k in trees}
    for rnd in range(args.ab_rounds):
        for k in (list(trees) if rnd % 2 == 0 else list(trees)[::-1]):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sample_only", trees[k], "--calls", str(args.calls), "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup), "--ab_tables", args.ab_tables], capture_output=True, text=True, timeout=300, cwd=trees[k])
            if r.returncode != 0:
                raise SystemExit(f"the {k} run failed (exit {r.returncode}):\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1]
            rounds[k].append(round(statistics.median(json.loads(line[3:])), 2))
            print(f"round {rnd} {k}", line, flush=True)
    lo, hi = min(rounds["parent"]), max(rounds["parent"])
    mb = statistics.median(rounds["branch"])
    res = {"what": f"DeviceHR2Pool(SecondOrderSpec(), DegradeSpec(), margin=8, tables='{args.ab_tables}').sample with no new option, B 32, P 64, x4, 24 gray 500 x 500 "
                   "images: us per call, host clock around calls_per_block calls ending in a synchronise; each run a fresh process, branch "
                   "and parent alternating, the order reversed every round; round_median_us = the median of a run's blocks",
           "calls_per_block": args.calls, "blocks_per_run": args.repeats, "rounds": args.ab_rounds, "round_median_us": rounds,
           "median_of_round_medians_us": {k: round(statistics.median(v), 2) for k, v in rounds.items()},
           "parent_round_to_round_range_us": [lo, hi],
           "branch_inside_the_parents_range": bool(lo <= mb <= hi), "branch_inside_or_below_the_parents_range": bool(mb <= hi)}
    with open(args.ab_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("round_median_us", "median_of_round_medians_us", "branch_inside_the_parents_range")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usm_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50, help="sample calls per timed block")
    ap.add_argument("--repeats", type=int, default=7, help="timed blocks per pool")
    ap.add_argument("--ab_tree", default=None, help="a checkout of the parent commit with its library built: A/B of DeviceHR2Pool.sample")
    ap.add_argument("--ab_out", default=os.path.join(ROOT, "profiles", "usm_probe_ab.json"))
    ap.add_argument("--ab_rounds", type=int, default=4)
    ap.add_argument("--ab_tables", choices=["host", "device"], default="host",
                    help="the pool's table setting in the A/B: 'host' is the default path (28 of its 30 ms are numpy on the host), 'device' "
                         "leaves the chain's launches as the bulk of a call")
    ap.add_argument("--ab_only", action="store_true")
    ap.add_argument("--sample_only", default=None, metavar="TREE", help="(a child run of --ab_tree)")
    args = ap.parse_args()
    if args.sample_only:
        return sample_only(args.sample_only, args.calls, args.repeats, args.warmup, args.ab_tables)
    if args.ab_only:
        if not args.ab_tree:
            raise SystemExit("--ab_only needs --ab_tree DIR")
        return ab(args)
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    sys.path.insert(0, ROOT)
    import torch
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd._lib import check, lib
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHR2Pool, SecondOrderSpec, UsmSpec, stage1_table
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
    E = s * (P + 2 * m)
    hrs = _images()
    idx = [i % len(hrs) for i in range(B)]
    st = torch.cuda.current_stream().cuda_stream
    spec = SecondOrderSpec()
    g = spec.rng(0)
    ps = [spec.draw(g, stage1_table((1.0, 1.5)), (0.02, 0.0), i, False, True, E, s) for i in range(B)]
    sizes = [ops.second_order_sizes(E, E, s, p) for p in ps]
    e1x, e2x = ops.RaggedExt([z[0] for z in sizes], "cuda"), ops.RaggedExt([z[1] for z in sizes], "cuda")
    Hp1, Hp2, Lo = int(E * 1.5 + 0.5), int(E / s * 1.2 + 0.5), E // s
    x = torch.rand(B, 3, E, E, device="cuda")
    a1, b1 = torch.rand(B, 3, Hp1, Hp1, device="cuda"), torch.empty(B, 3, Hp1, Hp1, device="cuda")
    a2 = torch.rand(B, 3, Hp2, Hp2, device="cuda")
    lr1 = torch.empty(B, 3, Lo, Lo, device="cuda")
    variants = {}
    taps = ops.usm_taps(51, 8.0, x.device)
    for n in (E, 256):
        xi = torch.rand(B, 3, n, n, device="cuda")
        yo, wk = torch.empty_like(xi), torch.empty_like(xi)
        variants[f"usm_sharpen_{n}_ks51"] = lambda xi=xi, yo=yo, wk=wk, n=n: check(lib().srk_usm_sharpen_f32(
            xi.data_ptr(), taps.data_ptr(), yo.data_ptr(), wk.data_ptr(), B, 3, n, n, 51, 0.5, 10.0, st))
    stages = {f"{E}_to_pad{Hp1}": (x, None, b1, e1x.dev, E, Hp1), f"pad{Hp1}_to_pad{Hp2}": (a1, e1x.dev, a2.clone(), e2x.dev, Hp1, Hp2),
              f"pad{Hp2}_to_{Lo}": (a2, e2x.dev, lr1, None, Hp2, Lo)}
    for name, (src, ei, dst, eo, hi, ho) in stages.items():
        pi, po = (None if ei is None else ei.data_ptr()), (None if eo is None else eo.data_ptr())
        variants[f"resize_aa_ragged_{name}"] = lambda src=src, dst=dst, pi=pi, po=po, hi=hi, ho=ho: check(lib().srk_resize_aa_ragged_f32(
            src.data_ptr(), pi, dst.data_ptr(), po, B, 3, hi, hi, ho, ho, 0, st))
        for mode in (0, 1, 2):
            md = torch.full((B,), mode, dtype=torch.int32, device="cuda")
            variants[f"resize_ragged_mode{mode}_{name}"] = lambda src=src, dst=dst, pi=pi, po=po, hi=hi, ho=ho, md=md: check(
                lib().srk_resize_ragged_mode_f32(src.data_ptr(), pi, dst.data_ptr(), po, md.data_ptr(), B, 3, hi, hi, ho, ho, 0, st))
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
    pools = {"second_order": DeviceHR2Pool(hrs, P, s, spec, DegradeSpec(), margin=m),
             "second_order_usm": DeviceHR2Pool(hrs, P, s, spec, DegradeSpec(), margin=m, usm=UsmSpec()),
             "second_order_usm_modes": DeviceHR2Pool(hrs, P, s, SecondOrderSpec(resize_mode_prob=(0.3, 0.3, 0.4)), DegradeSpec(), margin=m, usm=UsmSpec())}
    blocks = _sample_blocks(pools, idx, args.calls, args.repeats, args.warmup)
    sample = {k: _stats(v) for k, v in blocks.items()}
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "calls_per_block": args.calls,
           "blocks": args.repeats, "spin_cycles_before_each_bracket": spin, "B": B, "lr_patch": P, "scale": s, "margin": m, "window": E,
           "stage1_extents": sorted(h for h, _ in e1x.host), "stage2_extents": sorted(h for h, _ in e2x.host),
           "note": "kernel_us: us between two HIP events per call of the C entry (srk_usm_sharpen_f32 is two launches), median / min / max over "
                   "launches, variants alternating; sample_us: host clock around calls_per_block sample() calls ending in a synchronise, per "
                   "call, median / min / max over blocks, the pools alternating; cache-resident tensors, not HBM rates",
           "kernel_us": {k: _stats(v) for k, v in times.items()}, "sample_us": sample, "cfg3_train_step_ms": CFG3_STEP_MS,
           "share_of_cfg3_step_percent": {k: round(100.0 * v["median_us"] / (CFG3_STEP_MS * 1e3), 3) for k, v in sample.items()}}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if args.ab_tree:
        ab(args)


if __name__ == "__main__":
    main()
