"""Developer probe: the frequency loss of csrc/fft_loss.hip at cfg3's output shape (32 x 3 x 256 x 256) and at 16 x 3 x 128 x 128.

Protocol of tools/loss_probe.py: each call between its own pair of HIP events behind a ~100 us spin kernel (the bracket holds device
time, not the host's enqueue gap), variants alternating launch by launch after a warm-up of every variant, median over `--launches`:

    fft_term              srk_fft_loss_fwd_bwd, value and gradient accumulated onto an existing d_pred (what make_loss runs)
    fft_value             the same entry without d_x (transpose, stages 1 and 2, finish)
    ssim_term             srk_ssim_loss_fwd_bwd, value and gradient accumulated: the other structural term, for scale
    torch_fft_fwd_bwd     what a user has without the kernel: F.l1_loss of the stacked torch.fft.rfft2 parts on the same device tensors,
                          forward + backward through torch autograd; left out (with the reason) when torch's FFT backend does not run

Counted FLOPs of the term: 2 H W Wh * 2 (stage 1) + 2 H H Wh * 4 (stage 2) per plane forward, the same backward; reported as a fraction
of the 155 TF fp32 matrix peak.  The fused-strip variant (a column strip resident in LDS across stages 1 and 2) was not built: no A/B.

    python tools/fft_loss_probe.py --out profiles/fft_loss_probe.json [--step_ms MS]
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
from tpu_superresolution_amd import ops  # noqa: E402

PEAK_TF = 155.0


def flops(shape, with_grad=True):
    B, C, H, W = shape
    Wh = W // 2 + 1
    fwd = B * C * (4.0 * H * W * Wh + 8.0 * H * H * Wh)
    return fwd * (2 if with_grad else 1)


def probe(shape, launches, warmup, spin):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(0)
    t = torch.rand(B, C, H, W, generator=g).cuda()
    p = (t + 0.05 * torch.randn(B, C, H, W, generator=g).cuda()).contiguous()
    d = torch.zeros_like(p)
    loss = torch.zeros(1, device="cuda")
    leaf = p.clone().requires_grad_(True)

    def torch_fft():
        leaf.grad = None
        fp, ft = torch.fft.rfft2(leaf), torch.fft.rfft2(t)
        torch.nn.functional.l1_loss(torch.stack([fp.real, fp.imag], -1), torch.stack([ft.real, ft.imag], -1)).backward()

    variants = {"fft_term": lambda: ops.fft_loss_fwd_bwd(p, t, alpha=0.05, d_x=d, accumulate=True, loss=loss),
                "fft_value": lambda: ops.fft_loss_fwd_bwd(p, t, want_grad=False),
                "ssim_term": lambda: ops.ssim_loss_fwd_bwd(p, t, 1.0, alpha=0.2, d_x=d, accumulate=True, loss=loss)}
    skipped = None
    try:
        torch_fft()
        torch.cuda.synchronize()
        variants["torch_fft_fwd_bwd"] = torch_fft
    except Exception as e:          # no usable FFT backend in this torch build: the row is left out
        skipped = f"{type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}"
        print(f"torch_fft_fwd_bwd left out: {skipped}", flush=True)
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
    for k, grad in (("fft_term", True), ("fft_value", False)):
        out[k]["gflop"] = round(flops(shape, grad) / 1e9, 3)
        out[k]["fraction_of_fp32_matrix_peak"] = round(flops(shape, grad) / (out[k]["median_us"] * 1e-6) / (PEAK_TF * 1e12), 4)
    out["fft_term_over_ssim_term"] = round(out["fft_term"]["median_us"] / out["ssim_term"]["median_us"], 2)
    if skipped is None:
        out["fft_term_speedup_over_torch"] = round(out["torch_fft_fwd_bwd"]["median_us"] / out["fft_term"]["median_us"], 2)
    else:
        out["torch_fft_fwd_bwd_left_out"] = skipped
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft_loss_probe.json"))
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
    res = {"probe": "fft_loss", "device": torch.cuda.get_device_name(0), "kernels_digest": kernels_digest(), "launches": args.launches,
           "warmup": args.warmup, "spin_cycles_before_each_bracket": spin, "fp32_matrix_peak_tf": PEAK_TF,
           "note": "us per call between two HIP events (allocations and fills of the Python wrapper included): median / min / max over "
                   "`launches` calls, variants alternating; torch_fft_fwd_bwd = l1_loss of the stacked torch.fft.rfft2 parts, forward + "
                   "autograd backward on the same device tensors; the fused-strip variant was not built (no A/B)", "shapes": {}}
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
