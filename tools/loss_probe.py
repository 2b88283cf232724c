"""Developer probe: the training objectives of csrc/loss.hip at cfg3's output shape (32 x 3 x 256 x 256) and at 16 x 3 x 128 x 128.

Timed, each between its own pair of HIP events behind a ~100 us spin kernel (the bracket holds device time, not the host's enqueue gap),
variants alternating launch by launch after a warm-up of every variant, median over `--launches` launches:

    l1                    the existing srk_l1_loss_fwd_bwd call (ops.l1_loss_fwd_bwd: two fills + the kernel)
    pixel_l1 / _mse / _charbonnier
                          srk_pixel_loss_fwd_bwd (ops.pixel_loss_fwd_bwd: the same fills + kernel + finishing workgroup)
    ssim_term             srk_ssim_loss_fwd_bwd, value and gradient accumulated onto an existing d_pred (what make_loss runs)
    ssim_value            the same kernel without d_x
    ssim_metric           the existing srk_ssim (ops.ssim), value only
    torch_ssim_fwd_bwd    what a user has without the kernel: metrics.ssim_torch on the same device tensors, forward + backward through
                          torch autograd (1 - S).backward()

The kernel-source digest is computed as bench.py does, so a stored result names the library it was measured on.

    python tools/loss_probe.py --out profiles/loss_probe.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import kernels_digest  # noqa: E402
from tpu_superresolution_amd import metrics, ops  # noqa: E402


def probe(shape, launches, warmup, spin):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(0)
    t = torch.rand(B, C, H, W, generator=g).cuda()
    p = (t + 0.05 * torch.randn(B, C, H, W, generator=g).cuda()).contiguous()
    d = torch.zeros_like(p)
    loss = torch.zeros(1, device="cuda")
    leaf = p.clone().requires_grad_(True)

    def torch_ssim():
        leaf.grad = None
        (1.0 - metrics.ssim_torch(leaf, t, data_range=1.0)).backward()

    variants = {"l1": lambda: ops.l1_loss_fwd_bwd(p, t)}
    for kind in ("l1", "mse", "charbonnier"):
        variants[f"pixel_{kind}"] = (lambda kind=kind: ops.pixel_loss_fwd_bwd(p, t, kind, 1e-3))
    variants["ssim_term"] = lambda: ops.ssim_loss_fwd_bwd(p, t, 1.0, alpha=0.2, d_x=d, accumulate=True, loss=loss)
    variants["ssim_value"] = lambda: ops.ssim_loss_fwd_bwd(p, t, 1.0, want_grad=False)
    variants["ssim_metric"] = lambda: ops.ssim(p, t, 1.0)
    variants["torch_ssim_fwd_bwd"] = torch_ssim
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
    out = {}
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        print(f"{'x'.join(map(str, shape)):>16s} {k:20s} {med:9.2f} us  [{min(v):.2f} - {max(v):.2f}]", flush=True)
    out["ssim_term_speedup_over_torch"] = round(out["torch_ssim_fwd_bwd"]["median_us"] / out["ssim_term"]["median_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_probe.json"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step_ms", type=float, default=None, help="cfg3 step time of one bench.py run on the same machine: recorded, and "
                                                                 "every time is also given as a share of it")
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
    res = {"probe": "loss", "device": torch.cuda.get_device_name(0), "kernels_digest": kernels_digest(), "launches": args.launches,
           "warmup": args.warmup, "spin_cycles_before_each_bracket": spin,
           "note": "us per call between two HIP events (allocations and fills of the Python wrapper included): median / min / max over "
                   "`launches` calls, variants alternating; torch_ssim_fwd_bwd = metrics.ssim_torch forward + autograd backward on the "
                   "same device tensors", "shapes": {}}
    for shape in ((32, 3, 256, 256), (16, 3, 128, 128)):
        res["shapes"]["x".join(map(str, shape))] = probe(shape, args.launches, args.warmup, spin)
    if args.step_ms:
        res["cfg3_step_ms"] = args.step_ms
        big = res["shapes"]["32x3x256x256"]
        res["share_of_cfg3_step_percent"] = {k: round(100.0 * v["median_us"] / (args.step_ms * 1e3), 3) for k, v in big.items()
                                             if isinstance(v, dict)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
