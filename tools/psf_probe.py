"""Developer probe: the 2-D blur degradation (csrc/blur2d.hip) beside the separable one (csrc/degrade.hip), where training uses them.

The training batch of tools/degrade_probe.py: 24 gray 500 x 500 images (the DeepRockSR-2D image size), B 32, P 64, x2 and x4, augment none.
   - `kernel_us`: the C entries alone on one fixed set of descriptors between two HIP events, each bracket queued behind a ~100 us spin
     kernel so that it holds device time and not the host's enqueue gap; variants alternate launch by launch; median / min / max.
     `crop_degrade_blind_u8`: sigma = 2.5 on both axes (the widest composed tables); `crop_degrade_psf_u8_ks7 / 17 / 21`: the new entry
     with a rotated Gaussian of that size per sample (17 is the support of sigma 2.5).  All with noise (sigma_n 10 / 255, gain 0.01) and
     the 8-bit rounding.
   - `sample_us`: host clock around `--calls` consecutive `DeviceHRPool.sample` calls that end in a device synchronise, per call, for the
     blind pool and the same pool with PsfSpec('rotated') and PsfSpec('mixed'); blocks of the pools alternate; median / min / max.
   - `--ab_tree DIR` (after the above, or alone with `--ab_only`): `sample` of the blind pool WITHOUT psf= in this tree and in the tree at
     DIR (a checkout of the parent commit with its library built), each in a fresh child process, the trees alternating run by run -- the
     scheme of tools/ab.sh -- to show that the path without the new options costs what it did.
Everything is warmed up first.  The tensors stay in the 256 MiB Infinity Cache between launches: these are not HBM rates.  There is no
pass / fail threshold; a train step is hundreds of times longer than any figure here.

    python tools/psf_probe.py --out profiles/psf_probe.json [--ab_tree ../parent --ab_out profiles/psf_probe_ab.json]
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


def sample_only(tree, calls, repeats, warmup):
    """One child run of the A/B: `sample` of the blind pool of the package under `tree`, x2 and x4 -> one JSON line."""
    sys.path.insert(0, tree)
    import torch
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool
    torch.cuda.set_device(0)
    hrs, out = _images(), {}
    for s in (2, 4):
        blocks = _sample_blocks({"blind": DeviceHRPool(hrs, 64, s, degrade=DegradeSpec())}, [i % len(hrs) for i in range(32)], calls, repeats, warmup)
        out[f"x{s}"] = blocks["blind"]
    print("AB " + json.dumps(out), flush=True)


def ab(args):
    trees = {"branch": ROOT, "parent": os.path.abspath(args.ab_tree)}
    runs = {k: {"x2": [], "x4": []} for k in trees}
    for rnd in range(args.ab_rounds):
        for k in (list(trees) if rnd % 2 == 0 else list(trees)[::-1]):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sample_only", trees[k], "--calls", str(args.calls), "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=300, cwd=trees[k])
            if r.returncode != 0:
                raise SystemExit(f"the {k} run failed (exit {r.returncode}):\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1]
            for s, v in json.loads(line[3:]).items():
                runs[k][s] += v
            print(f"round {rnd} {k}", line, flush=True)
    res = {"what": "DeviceHRPool(degrade=DegradeSpec()).sample without psf=, B 32, P 64, 24 gray 500 x 500 images: us per call, host clock around "
                   "calls_per_block calls ending in a synchronise; each run a fresh process, branch and parent alternating",
           "calls_per_block": args.calls, "blocks_per_run": args.repeats, "rounds": args.ab_rounds,
           "sample_us": {k: {s: _stats(v) for s, v in d.items()} for k, d in runs.items()}}
    with open(args.ab_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["sample_us"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psf_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200, help="sample calls per timed block")
    ap.add_argument("--repeats", type=int, default=7, help="timed blocks per pool")
    ap.add_argument("--ab_tree", default=None, help="a checkout of the parent commit with its library built: A/B of `sample` without psf=")
    ap.add_argument("--ab_out", default=os.path.join(ROOT, "profiles", "psf_probe_ab.json"))
    ap.add_argument("--ab_rounds", type=int, default=4)
    ap.add_argument("--ab_only", action="store_true")
    ap.add_argument("--sample_only", default=None, metavar="TREE", help="(a child run of --ab_tree)")
    args = ap.parse_args()
    if args.sample_only:
        return sample_only(args.sample_only, args.calls, args.repeats, args.warmup)
    if args.ab_only:
        if not args.ab_tree:
            raise SystemExit("--ab_only needs --ab_tree DIR")
        return ab(args)
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd._lib import check, lib
    from tpu_superresolution_amd.ops import pack_degrade_params
    from tpu_superresolution_amd.sr_datasets import DegradeSpec, DeviceHRPool, PsfSpec
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
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "calls_per_block": args.calls,
           "blocks": args.repeats, "spin_cycles_before_each_bracket": spin,
           "note": "kernel_us: us between two HIP events per launch, median / min / max over launches, variants alternating; sample_us: "
                   "host clock around calls_per_block sample() calls ending in a synchronise, per call, median / min / max over blocks, "
                   "the pools alternating; cache-resident tensors, not HBM rates",
           "pool": {}}
    hrs = _images()
    B, P = 32, 64
    st = torch.cuda.current_stream().cuda_stream
    idx = [i % len(hrs) for i in range(B)]
    for s in (2, 4):
        pools = {"blind": DeviceHRPool(hrs, P, s, degrade=DegradeSpec()),
                 "psf_rotated": DeviceHRPool(hrs, P, s, degrade=DegradeSpec(), psf=PsfSpec("rotated")),
                 "psf_mixed": DeviceHRPool(hrs, P, s, degrade=DegradeSpec(), psf=PsfSpec("mixed"))}
        blocks = _sample_blocks(pools, idx, args.calls, args.repeats, args.warmup)
        random.seed(1)
        hd, _ = pools["blind"].draw(idx)
        desc = torch.tensor([d + tuple(pack_degrade_params((2.5, 2.5), (10.0 / 255.0, 0.01), i, True)) for i, d in enumerate(hd)], dtype=torch.int64).cuda()
        lr, hr = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P * s, P * s, device="cuda")
        hp = pools["blind"].pool
        variants = {"crop_degrade_blind_u8": lambda: check(lib().srk_crop_degrade_blind_u8(hp.data_ptr(), desc.data_ptr(), lr.data_ptr(), hr.data_ptr(), B, P, s, 8, st))}
        rng = np.random.RandomState(2)
        for ks in (7, 17, 21):
            sig = (ks - 1) / 6.0
            tabs = torch.from_numpy(np.stack([bk.gaussian(ks, sig, 0.5 * sig, rng.uniform(-np.pi / 2, np.pi / 2)) for _ in range(B)])).cuda()
            variants[f"crop_degrade_psf_u8_ks{ks}"] = lambda tabs=tabs, ks=ks: check(lib().srk_crop_degrade_psf_u8(
                hp.data_ptr(), desc.data_ptr(), tabs.data_ptr(), ks, lr.data_ptr(), hr.data_ptr(), B, P, s, 8, st))
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
        res["pool"][f"x{s}"] = {"B": B, "lr_patch": P, "images": len(hrs), "image_size": [500, 500],
                                "sample_us": {k: _stats(v) for k, v in blocks.items()}, "kernel_us": {k: _stats(v) for k, v in times.items()}}
        print(f"x{s}", json.dumps(res["pool"][f"x{s}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if args.ab_tree:
        ab(args)


if __name__ == "__main__":
    main()
