"""Developer probe: the six launches of metrics.niqe_moments (csrc/niqe.hip) on preallocated buffers -> profiles/niqe_probe.json.

    python tools/niqe_probe.py [--out profiles/niqe_probe.json] [--launches 50]

Shapes: B 1 at 1024 x 1024 (one predicted photograph) and B 8 at 256 x 256 (a batch of training-size outputs), RGB, border 0, bs 96.  Each C
entry runs alone between two HIP events, each bracket queued behind a ~100 us spin kernel (the bracket holds device time, not the launch
path); median / min / max over `launches` brackets, the six entries alternating, and the share each takes of their sum.  `all_six` brackets
the six launches together.  The end-to-end deviations |device score - fp64 reference score| of tests/test_gpu_niqe.py's seven images are
measured here too (the figures of DESIGN 7x).  No gate.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd import metrics  # noqa: E402
from tpu_superresolution_amd._lib import _p, _stream, check, lib  # noqa: E402
from tpu_superresolution_amd.niqe import niqe_window  # noqa: E402


def probe(shape, launches, warmup, spin, bs=96):
    B, C, H, W = shape
    Hk, Wk = H // bs * bs, W // bs * bs
    nb = (Hk // bs) * (Wk // bs)
    f32 = dict(dtype=torch.float32, device="cuda")
    x = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(0)).cuda()
    win = torch.from_numpy(niqe_window().astype(np.float32).reshape(49)).cuda()
    plane, half = torch.empty(B, Hk, Wk, **f32), torch.empty(B, Hk // 2, Wk // 2, **f32)
    m1, sg, m2 = torch.empty_like(plane), torch.empty_like(plane), torch.empty_like(half)
    mom1, mom2, sharp = torch.empty(B, nb, 25, **f32), torch.empty(B, nb, 25, **f32), torch.empty(B, nb, **f32)
    L, s = lib(), _stream()
    stages = {
        "plane": lambda: check(L.srk_niqe_plane_f32(_p(x), _p(plane), B, C, H, W, 0, bs, s)),
        "half": lambda: check(L.srk_niqe_half_f32(_p(plane), _p(half), B, Hk, Wk, s)),
        "mscn_scale1": lambda: check(L.srk_niqe_mscn_f32(_p(plane), _p(win), _p(m1), _p(sg), B, Hk, Wk, s)),
        "mscn_scale2": lambda: check(L.srk_niqe_mscn_f32(_p(half), _p(win), _p(m2), None, B, Hk // 2, Wk // 2, s)),
        "moments_scale1": lambda: check(L.srk_niqe_moments_f32(_p(m1), _p(sg), _p(mom1), _p(sharp), B, Hk, Wk, bs, s)),
        "moments_scale2": lambda: check(L.srk_niqe_moments_f32(_p(m2), None, _p(mom2), None, B, Hk // 2, Wk // 2, bs // 2, s)),
    }

    def all_six():
        for fn in stages.values():
            fn()

    variants = dict(stages, all_six=all_six)
    for _ in range(warmup):
        all_six()
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
    out = {}
    total = sum(statistics.median(times[k]) for k in stages)
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        if k in stages:
            out[k]["share_of_the_six_percent"] = round(100.0 * med / total, 1)
        print(f"{'x'.join(map(str, shape)):>16s} {k:16s} {med:9.2f} us  [{min(v):.2f} - {max(v):.2f}]", flush=True)
    out["sum_of_the_six_us"] = round(total, 2)
    out["blocks_per_image"] = nb
    return out


def end_to_end():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import niqe_ref as R
    S = R.suite()
    names = list(S["images"])
    x = torch.from_numpy(np.concatenate([S["images"][k] for k in names])).cuda()
    got = metrics.niqe(x, (S["mu"], S["cov"], R.window())).numpy()
    return {k: {"reference_fp64": round(S["scores"][k], 6), "abs_deviation_of_the_device_score": float(f"{abs(got[i] - S['scores'][k]):.3e}")}
            for i, k in enumerate(names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "niqe_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
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
    res = {"probe": "niqe", "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup,
           "spin_cycles_before_each_bracket": spin,
           "note": "us per C entry between two HIP events behind a spin kernel: median / min / max over `launches` brackets, entries "
                   "alternating; share = median over the sum of the six medians; no gate", "shapes": {}}
    for shape in ((1, 3, 1024, 1024), (8, 3, 256, 256)):
        res["shapes"]["x".join(map(str, shape))] = probe(shape, args.launches, args.warmup, spin)
    res["end_to_end_288x288_bs96"] = end_to_end()
    res["end_to_end_largest_abs_deviation"] = max(v["abs_deviation_of_the_device_score"] for v in res["end_to_end_288x288_bs96"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
