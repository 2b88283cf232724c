"""Developer probe: the scale-1 restoration pairs (csrc/restore.hip) where training uses them.

   - `kernel_us`: srk_crop_restore_u8 alone on fixed descriptors between two HIP events, each bracket queued behind a ~100 us spin
     kernel so that it holds device time and not the host's enqueue gap; B 32 at P 64 and B 8 at P 126, gray (out_chans 1) and colour
     (out_chans 3) from RGB 500 x 500 images, quality 0 (noise alone) and 75, 4:4:4 and 4:2:0; variants alternate launch by launch;
     median / min / max.
   - `sample_us`: host clock around ONE `DeviceRestorePool.sample` call that ends in a device synchronise, beside the THREE-LAUNCH
     composition of the same pair from patch-anchored pieces (srk_paired_crop_u8 at scale 1, ops.noise, ops.jpeg_roundtrip), the two
     alternating call by call; median / min / max over `--calls`.
   - `--only_jpeg`: srk_jpeg_roundtrip_f32 on [32, 3, 64, 64] at quality 75 alone, bracketed as above.  It needs nothing this stage
     added, so it runs on the library of an earlier commit (SRK_LIB_PATH).  `--ab PARENT_LIB` alternates fresh processes of it on the
     in-tree library and on PARENT_LIB, order reversed every round, and writes the rounds side by side: did the unchanged entry keep
     its time after its device routines moved to jpeg.h?

Everything is warmed up first.  The tensors stay in the 256 MiB Infinity Cache between launches: these are not HBM rates.  There is no
pass / fail threshold; a train step is hundreds of times longer than any figure here.

    python tools/restore_probe.py --out profiles/restore_probe.json
    python tools/restore_probe.py --ab /path/to/parent/libsrk.so --out profiles/restore_probe_ab.json
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
sys.path.insert(0, ROOT)


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def _spin_cycles(torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    e0.record()
    torch.cuda._sleep(1_000_000)
    e1.record()
    torch.cuda.synchronize()
    return max(1, int(1_000_000 * 0.1 / e0.elapsed_time(e1)))


def _bracketed(torch, variants, launches, warmup, spin):
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


def only_jpeg(args):
    import ctypes as C

    import torch

    from tpu_superresolution_amd._lib import LIB_PATH
    # the one entry, bound by hand: the package's own table names entries that an earlier library does not have
    entry = C.CDLL(LIB_PATH).srk_jpeg_roundtrip_f32
    entry.restype, entry.argtypes = C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p] * 2
    torch.cuda.set_device(0)
    spin = _spin_cycles(torch)
    B, Cc, P = 32, 3, 64
    g = torch.Generator().manual_seed(0)
    x = (torch.randint(0, 256, (B, Cc, P, P), generator=g).float() / 255.0).cuda()
    out, qd = torch.empty_like(x), torch.full((B,), 75, dtype=torch.int32).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def fn():
        if entry(x.data_ptr(), out.data_ptr(), qd.data_ptr(), B, Cc, P, P, 0, None, st) != 0:
            raise SystemExit("srk_jpeg_roundtrip_f32 refused the probe's batch")

    res = {"library": os.path.relpath(LIB_PATH, ROOT), "launches": args.launches, **_bracketed(torch, {"jpeg_roundtrip_444_q75": fn}, args.launches, args.warmup, spin)}
    print(json.dumps(res), flush=True)


def ab(args):
    """Fresh processes of --only_jpeg, alternating the in-tree library and the parent's; this process never opens the GPU."""
    libs = {"branch": os.path.join(ROOT, "tpu_superresolution_amd", "libsrk.so"), "parent": os.path.abspath(args.ab)}
    rounds = []
    for rnd in range(1, args.rounds + 1):
        for tree in (("parent", "branch") if rnd % 2 else ("branch", "parent")):
            env = dict(os.environ, SRK_LIB_PATH=libs[tree])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only_jpeg", "--launches", str(args.launches), "--warmup", str(args.warmup)],
                               env=env, capture_output=True, text=True, timeout=120)
            if r.returncode != 0:
                raise SystemExit(f"--only_jpeg on the {tree} library ended with status {r.returncode}:\n{r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            rounds.append({"round": rnd, "tree": tree, **line["jpeg_roundtrip_444_q75"]})
            print(json.dumps(rounds[-1]), flush=True)
    summary = {}
    for tree in libs:
        med = [r["median_us"] for r in rounds if r["tree"] == tree]
        summary[tree] = {"median_of_round_medians_us": round(statistics.median(med), 2), "round_medians_min_us": min(med), "round_medians_max_us": max(med),
                         "min_us": min(r["min_us"] for r in rounds if r["tree"] == tree), "max_us": max(r["max_us"] for r in rounds if r["tree"] == tree)}
    p, b = summary["parent"], summary["branch"]
    summary["branch_median_inside_parent_round_range"] = p["round_medians_min_us"] <= b["median_of_round_medians_us"] <= p["round_medians_max_us"]
    res = {"note": "srk_jpeg_roundtrip_f32 on [32, 3, 64, 64] at quality 75, 4:4:4 (tools/restore_probe.py --only_jpeg): us between two HIP events "
                   "behind a spin kernel, per round the median / min / max over the launches; one fresh process per library and round, order "
                   "reversed every round; 'parent' is the library of the parent commit",
           "launches": args.launches, "rounds": rounds, "summary": summary}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=300, help="timed sample calls per variant")
    ap.add_argument("--only_jpeg", action="store_true", help="measure srk_jpeg_roundtrip_f32 alone (runs on an earlier library through SRK_LIB_PATH)")
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB", help="alternate --only_jpeg processes on the in-tree library and on PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=4, help="--ab: rounds of one process per library")
    args = ap.parse_args()
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    if args.ab is not None:
        return ab(args)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    if args.only_jpeg:
        return only_jpeg(args)
    from tpu_superresolution_amd import ops
    from tpu_superresolution_amd._lib import check, lib
    from tpu_superresolution_amd.sr_datasets import DeviceRestorePool, RestoreSpec
    torch.cuda.set_device(0)
    spin = _spin_cycles(torch)
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "calls": args.calls,
           "spin_cycles_before_each_bracket": spin,
           "note": "kernel_us: us between two HIP events per launch of srk_crop_restore_u8, median / min / max over launches, variants "
                   "alternating; sample_us: host clock around one call ending in a synchronise, variants alternating call by call; "
                   "cache-resident tensors, not HBM rates",
           "kernel_us": {}, "sample_us": {}}
    rng = np.random.RandomState(0)
    imgs = [(rng.rand(500, 500, 3) * 255).astype(np.uint8) for _ in range(24)]
    st = torch.cuda.current_stream().cuda_stream

    for B, P in ((32, 64), (8, 126)):
        idx = [i % len(imgs) for i in range(B)]
        variants, keep = {}, []
        for name, oc, q, sub in (("gray_noise_only", 1, 0, 0), ("gray_q75", 1, 75, 0), ("colour_noise_only", 3, 0, 0), ("colour_q75_444", 3, 75, 0),
                                 ("colour_q75_420", 3, 75, 1)):
            pool = DeviceRestorePool(imgs, P, oc, RestoreSpec(sigma=(25 / 255, 25 / 255), jpeg_quality=(q, q) if q else None, subsample=bool(sub)))
            random.seed(0)
            hd, _ = pool.draw(idx)
            desc = torch.tensor(pool.draw_restore(hd), dtype=torch.int64).cuda()
            clean, degr = torch.empty(B, oc, P, P, device="cuda"), torch.empty(B, oc, P, P, device="cuda")
            keep.append((pool, desc, clean, degr))
            variants[name] = (lambda pool=pool, desc=desc, clean=clean, degr=degr, oc=oc, sub=sub:
                              check(lib().srk_crop_restore_u8(pool.pool.data_ptr(), desc.data_ptr(), clean.data_ptr(), degr.data_ptr(), B, P, oc, sub, 0, st)))
        res["kernel_us"][f"B{B}_P{P}"] = _bracketed(torch, variants, args.launches, args.warmup, spin)
        print(f"kernel_us B{B}_P{P}", json.dumps(res["kernel_us"][f"B{B}_P{P}"]), flush=True)

        # one sample() call against the three-launch composition of a patch-anchored pair
        for name, oc, q, sub in (("colour_q75_444", 3, 75, False), ("colour_q75_420", 3, 75, True), ("colour_noise_only", 3, 0, False)):
            pool = DeviceRestorePool(imgs, P, oc, RestoreSpec(sigma=(25 / 255, 25 / 255), jpeg_quality=(q, q) if q else None, subsample=sub))

            def three(pool=pool, q=q, sub=sub):
                hd, _ = pool.draw(idx)
                desc = torch.tensor(hd + hd, dtype=torch.int64).cuda()
                a, b = torch.empty(B, 3, P, P, device="cuda"), torch.empty(B, 3, P, P, device="cuda")
                check(lib().srk_paired_crop_u8(pool.pool.data_ptr(), desc[:B].data_ptr(), desc[B:].data_ptr(), a.data_ptr(), b.data_ptr(), B, P, 1, st))
                y = ops.noise(a, (25 / 255, 0.0), range(B), False, 0)
                return (ops.jpeg_roundtrip(y, q, sub) if q else y), b

            fns = {"one_launch": lambda pool=pool: pool.sample(idx), "three_launches": three}
            random.seed(0)
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            calls = {k: [] for k in fns}
            for _ in range(args.calls):
                for k, fn in fns.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    calls[k].append((time.perf_counter() - t0) * 1e6)
            res["sample_us"][f"B{B}_P{P}_{name}"] = {k: _stats(v) for k, v in calls.items()}
            print(f"sample_us B{B}_P{P}_{name}", json.dumps(res["sample_us"][f"B{B}_P{P}_{name}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
