"""Developer probe: srk_psnrb and srk_msssim (csrc/fullref.hip) on preallocated buffers -> profiles/fullref_probe.json.

    python tools/fullref_probe.py [--out profiles/fullref_probe.json] [--launches 50]

Shapes: B 1 at 1024 x 1024 (one predicted photograph) and B 8 at 256 x 256 (a batch of training-size outputs), one luma plane each (mode y)
and three colour planes (mode rgb), integer planes 0..255.  Each C entry runs alone between two HIP events, each bracket queued behind a
~100 us spin kernel (the bracket holds device time, not the launch path); median / min / max over `launches` brackets, the entries
alternating.  srk_ssim and srk_bench_planes_f32 + srk_bench_psnr on the same planes / images are timed beside them for scale.  bytes_min is
what the entry must move at least (PSNR-B: both planes once; MS-SSIM: both images of every level once, the pooled planes written once) and
GB/s that figure over the median: a rate of the whole entry, its finishing launch included, not a kernel's share of peak.  No gate.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd._lib import _p, _stream, check, lib  # noqa: E402


def probe(shape, launches, warmup, spin):
    B, C, H, W = shape
    f32 = dict(dtype=torch.float32, device="cuda")
    g = torch.Generator().manual_seed(0)
    t = torch.randint(0, 256, shape, generator=g).float()
    p = (t + (6.0 * torch.randn(shape, generator=g)).round()).clamp(0, 255)
    x01, y01 = (p / 255.0).cuda(), (t / 255.0).cuda()
    p, t = p.cuda(), t.cuda()
    L, s = lib(), _stream()
    levels = 5
    ws_pb = torch.empty(int(L.srk_psnrb_workspace(B, C, H, W)), dtype=torch.uint8, device="cuda")
    ws_ms = torch.empty(int(L.srk_msssim_workspace(B, C, H, W, levels)), dtype=torch.uint8, device="cuda")
    ws_ss = torch.empty(int(L.srk_ssim_workspace(B, C, H, W)), dtype=torch.uint8, device="cuda")
    ws_bp = torch.empty(int(L.srk_bench_workspace(B, C, H, W)), dtype=torch.uint8, device="cuda")
    sums, out, means = torch.empty(B, C, 5, **f32), torch.empty(B, **f32), torch.empty(levels, B, C, 2, **f32)
    per, pp, pt, sq = torch.empty(B, **f32), torch.empty(shape, **f32), torch.empty(shape, **f32), torch.empty(B, **f32)

    def bench_planes_psnr():
        check(L.srk_bench_planes_f32(_p(x01), _p(y01), _p(pp), _p(pt), _p(ws_bp), B, C, H, W, 0, 1, s))
        check(L.srk_bench_psnr(_p(ws_bp), B, C, H, W, _p(sq), _p(per), None, s))

    entries = {
        "psnrb": lambda: check(L.srk_psnrb(_p(p), _p(t), _p(ws_pb), B, C, H, W, _p(sums), _p(out), s)),
        "msssim_5_levels": lambda: check(L.srk_msssim(_p(p), _p(t), _p(ws_ms), B, C, H, W, levels, 255.0, _p(means), s)),
        "ssim": lambda: check(L.srk_ssim(_p(p), _p(t), _p(ws_ss), B, C, H, W, 255.0, _p(per), None, s)),
        "bench_planes_rgb_and_psnr": bench_planes_psnr,
    }
    for _ in range(warmup):
        for fn in entries.values():
            fn()
    times = {k: [] for k in entries}
    for _ in range(launches):
        pairs = []
        for k, fn in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(spin)
            e0.record()
            fn()
            e1.record()
            pairs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in pairs:
            times[k].append(e0.elapsed_time(e1) * 1e3)
    plane_bytes = 4 * B * C * H * W
    pyramid = [plane_bytes]
    h, w = H, W
    for _ in range(levels - 1):
        h, w = (h + h % 2) // 2, (w + w % 2) // 2
        pyramid.append(4 * B * C * h * w)
    bytes_min = {"psnrb": 2 * plane_bytes, "msssim_5_levels": 2 * (sum(pyramid) + sum(pyramid[1:])), "ssim": 2 * plane_bytes,
                 "bench_planes_rgb_and_psnr": 4 * plane_bytes}
    res = {}
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "bytes_min": bytes_min[k],
                  "GB_per_s_of_bytes_min": round(bytes_min[k] / med / 1e3, 1)}
        print(f"{'x'.join(map(str, shape)):>16s} {k:28s} {med:9.2f} us  [{min(v):.2f} - {max(v):.2f}]", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullref_probe.json"))
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
    res = {"probe": "fullref", "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup,
           "spin_cycles_before_each_bracket": spin,
           "note": "us per C entry between two HIP events behind a spin kernel: median / min / max over `launches` brackets, entries "
                   "alternating; GB/s = bytes_min over the median, a rate of the whole entry; no gate", "shapes": {}}
    for shape in ((1, 1, 1024, 1024), (1, 3, 1024, 1024), (8, 1, 256, 256), (8, 3, 256, 256)):
        res["shapes"]["x".join(map(str, shape))] = probe(shape, args.launches, args.warmup, spin)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
