"""Developer probe: the benchmark-protocol metric kernels of csrc/metrics.hip on one full-size validation image, for a run under
rocprofv3 (kernel times come from the trace, not from this script):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/bench_metric_probe.py --variant y_psnr

Variants (one per process, so that the per-kernel statistics of a trace belong to one configuration):
    batch_psnr   the existing srk_batch_psnr pass (ops.batch_psnr) on the same two tensors: what validation runs beside the new kernels;
                 `--pkg-root TREE` imports the package of another checkout (the parent commit with its own library)
    y_psnr       srk_bench_planes_f32 without planes + srk_bench_psnr, mode y           (PSNR-Y alone)
    y_planes     the same with both planes written, then srk_ssim on them               (PSNR-Y + SSIM-Y)
    rgb_planes   mode rgb with planes, then srk_ssim                                    (PSNR-RGB + SSIM-RGB)

The image is [1, 3, 1356, 2040] (a 2K validation image at x4: border 4); bytes per launch are counted from the shapes and printed.
"""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--variant", choices=["batch_psnr", "y_psnr", "y_planes", "rgb_planes"], required=True)
ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--shape", type=int, nargs=4, default=[1, 3, 1356, 2040])
ap.add_argument("--border", type=int, default=4)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg_root))
from tpu_superresolution_amd import ops  # noqa: E402

B, C, H, W = args.shape
g = torch.Generator().manual_seed(0)
t = torch.rand(B, C, H, W, generator=g).cuda()
p = (t + 0.05 * torch.randn(B, C, H, W, generator=g).cuda()).contiguous()
acc = torch.zeros(1, device="cuda")
mode = "rgb" if args.variant.startswith("rgb") else "y"


def run():
    if args.variant == "batch_psnr":
        ops.batch_psnr(p, t, 1.0, psnr_sum=acc)
        return
    planes = args.variant.endswith("planes")
    pp, pt, ws = ops.bench_planes(p, t, args.border, mode, planes=planes)
    ops.bench_psnr(ws, ops.bench_plane_shape(p.shape, args.border, mode), psnr_sum=acc)
    if planes:
        ops.ssim(pp, pt, 255.0)


for _ in range(args.warmup):
    run()
torch.cuda.synchronize()
for _ in range(args.launches):
    run()
torch.cuda.synchronize()
Hc, Wc = H - 2 * args.border, W - 2 * args.border
Cm = C if mode == "rgb" else 1
read = 2 * 4 * B * C * (H * W if args.variant == "batch_psnr" else Hc * Wc)
written = 2 * 4 * B * Cm * Hc * Wc if args.variant.endswith("planes") else 0
print(json.dumps({"variant": args.variant, "shape": args.shape, "border": args.border, "launches": args.launches, "pkg_root": args.pkg_root,
                  "bytes_read_by_the_pass": read, "bytes_written_by_the_pass": written, "psnr_sum": float(acc)}))
