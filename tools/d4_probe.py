"""Developer probe: the D4 transform kernel (csrc/dihedral.hip, augment.dihedral) for each of the eight ops on one fp32 batch
(default 32 x 3 x 256 x 256: a training batch of HR patches), beside a device-to-device `copy_` of the same tensor -- the least any
out-of-place pass over it can cost -- and beside the stock torch operators that do the same permutation (torch.flip / transpose +
contiguous).  Also: one launch with per-sample codes (each of 0..7, four times over the batch) and the accumulating form the
self-ensemble uses (out += alpha * T(in): one more read of out).

Every launch is bracketed by its own pair of HIP events; the variants alternate launch by launch after a warm-up of every variant, and
the figure is the median over `--launches` launches (min and max kept as the spread).  A launch takes about as long as the host needs
to enqueue it, so each bracket is preceded by a spin kernel (torch.cuda._sleep, about 100 us, no memory traffic): the events and the
launch are all queued behind it and the bracket holds device time only, not the host's enqueue gap.  The tensor (25 MB, 50 MB of
traffic per launch) stays inside the 256 MiB Infinity Cache between launches, for the copy as for the kernel: the ratio to the copy is
the result, the GB/s are not HBM rates.

    python tools/d4_probe.py --out profiles/d4_probe.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd import augment as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "d4_probe.json"))
    ap.add_argument("--shape", type=int, nargs=4, default=[32, 3, 256, 256], metavar=("B", "C", "H", "W"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    torch.cuda.set_device(0)
    B, C, H, W = args.shape
    x = torch.rand(B, C, H, W, device="cuda")
    out = torch.empty_like(x)
    out_t = torch.empty(B, C, W, H, device="cuda")
    codes = torch.tensor([b % 8 for b in range(B)], dtype=torch.int32).cuda()

    variants = {"copy_": lambda: out.copy_(x)}
    for k in range(8):
        variants[f"op{k}"] = (lambda k=k: A.dihedral(x, k, out=out_t if k & 4 else out))
        variants[f"torch_op{k}"] = (lambda k=k: A.apply_op_host(x, k).contiguous() if k else x.clone())
    if H == W:
        variants["per_sample_codes"] = lambda: A.dihedral(x, codes, out=out)
    variants["op5_accumulate"] = lambda: A.dihedral(x, 5, out=out_t, alpha=0.125, accumulate=True)

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    # spin length for ~100 us, from a timed spin of a million cycles
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    e0.record()
    torch.cuda._sleep(1_000_000)
    e1.record()
    torch.cuda.synchronize()
    spin = max(1, int(1_000_000 * 0.1 / e0.elapsed_time(e1)))
    times = {k: [] for k in variants}
    for _ in range(args.launches):
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

    nbytes = x.numel() * 4
    copy_us = statistics.median(times["copy_"])
    res = {"device": torch.cuda.get_device_name(0), "shape": [B, C, H, W], "bytes_read_plus_written": 2 * nbytes,
           "launches": args.launches, "warmup": args.warmup, "spin_cycles_before_each_bracket": spin,
           "note": "us per launch between two HIP events: median / min / max over `launches` launches, variants alternating; "
                   "ratio_to_copy = median / median of copy_; gb_per_s = bytes moved / median (cache-resident tensor, not an HBM rate); "
                   "torch_op<k> = torch.flip / transpose + contiguous for the same permutation (op 0: clone)",
           "variants": {}}
    for k, v in times.items():
        med = statistics.median(v)
        moved = 3 * nbytes if k.endswith("accumulate") else 2 * nbytes
        res["variants"][k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                              "ratio_to_copy": round(med / copy_us, 3), "gb_per_s": round(moved / med / 1e3, 1)}
        print(f"{k:18s} {med:8.2f} us  [{min(v):.2f} - {max(v):.2f}]  x{med / copy_us:.2f} of copy_", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
