"""Developer probe: the optimizer part of a HAT (cfg4) / DAT (cfg5) train step at the bench's shapes (bs 16, 64 x 64 LR, x4), alone and
inside the whole graphed step, for
  (a) torch:  clip_grad_norm_ + torch.optim.AdamW(capturable=True)      -- what bench.py builds for cfg4 / cfg5
  (b) fused:  optim.FusedAdamW (multi-tensor kernels, csrc/optim_multi.hip)
  (c) fused_ema:  (b) with ema_decay = 0.999: the EMA of the weights advanced inside the step kernel
  (d) fused_then_foreach:  (b) followed by torch._foreach_mul_ + torch._foreach_add_(.., alpha=) on clones of the weights: the unfused
      way to the same average
eager and replayed from a hipGraph.  One process; every number is a median over `--repeats` windows of `--reps` steps taken after a
warm-up, the variants alternating window by window; min and max of the windows are kept beside it as the run-to-run spread.  Device time
= hip events around a window; host time = wall clock around the same window including the final synchronise.  Launch counts come from
torch.profiler (kernel + memcpy/memset records of one step) and are null when the profiler is unavailable.

    python tools/optim_probe.py --out profiles/r06_optim_ema_probe.json [--archs hat dat] [--no-profile]

(profiles/r05_optim_probe.json is the record of (a) and (b) from before the EMA variants existed.)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd.finetune_swinir import build_sr_model  # noqa: E402
from tpu_superresolution_amd.optim import FusedAdamW  # noqa: E402
from tpu_superresolution_amd.training import GraphedTrainStep, l1_loss_checked  # noqa: E402


EMA_DECAY = 0.999


def batch(bs, device, seed=1000):
    g = torch.Generator().manual_seed(seed)
    lr = torch.rand(bs, 3, 64, 64, generator=g)
    hr = torch.nn.functional.interpolate(lr, scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 1)
    return lr.to(device), hr.to(device)


def window(fn, reps):
    """-> (device ms / step, host ms / step) of `reps` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) * 1e3 / reps


def compare(fns: dict, reps, repeats, warm=10):
    """Alternating windows over the entries of fns -> {name: {device_ms: {median, min, max}, host_ms: {...}}}"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    got = {k: ([], []) for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            d, h = window(fn, reps)
            got[k][0].append(d)
            got[k][1].append(h)

    def summary(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return {k: {"device_ms": summary(d), "host_ms": summary(h)} for k, (d, h) in got.items()}


def count_launches(fn):
    """Device activities of one call: kernels and memcpy / memset records."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [e for e in ev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return {"kernels": len(kernels), "copies_and_fills": len(ev) - len(kernels), "distinct_kernels": len({e.name for e in kernels})}
    except Exception as exc:          # the probe's timings stand without the counts
        return {"error": f"{type(exc).__name__}: {exc}"[:200]}


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def probe(arch, args, out, flush):
    dev = torch.device("cuda", 0)
    lr_img, hr_img = batch(args.batch, dev)
    res = out.setdefault(arch, {})

    # ---- the optimizer part alone, on gradients that are already there ---------------------------------------------------------------
    torch.manual_seed(42)
    model = build_sr_model(arch, 4, 0.1).to(dev).train()
    loss, _ = l1_loss_checked(model(lr_img), hr_img)
    loss.backward()
    params = [p for p in model.parameters() if p.grad is not None]
    res["tensors"] = len(params)
    res["elements"] = sum(p.numel() for p in params)
    # the least traffic a step needs: read p, g, m, v and write p, m, v (fp32) + one more read of g for the norm
    res["min_bytes_per_step"] = 8 * 4 * res["elements"]
    t_opt = torch.optim.AdamW(params, lr=2e-5, weight_decay=0.0, capturable=True)
    f_opt = FusedAdamW(model, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0)

    def torch_part():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        t_opt.step()

    def fused_part():
        f_opt.step()
    e_opt = FusedAdamW(model, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0, ema_decay=EMA_DECAY)
    u_opt = FusedAdamW(model, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0)
    weights = [p.detach() for p in params]
    avg = [w.clone() for w in weights]

    def fused_ema_part():
        e_opt.step()

    def fused_then_foreach_part():
        u_opt.step()
        torch._foreach_mul_(avg, EMA_DECAY)
        torch._foreach_add_(avg, weights, alpha=1.0 - EMA_DECAY)
    res["fused_launches_expected"] = 1 + math.ceil(len(params) / 160) + math.ceil(len(params) / 80)
    res["fused_ema_launches_expected"] = 1 + math.ceil(len(params) / 160) + math.ceil(len(params) / 72)
    # the average costs one more read and one more write of an fp32 array
    res["ema_extra_bytes_per_step"] = 2 * 4 * res["elements"]
    parts = {"torch": torch_part, "fused": fused_part, "fused_ema": fused_ema_part, "fused_then_foreach": fused_then_foreach_part}
    res["eager"] = compare(parts, args.reps, args.repeats)
    flush()
    graphs = {k: capture(fn) for k, fn in parts.items()}

    def replay_of(opt, g):
        def run():
            opt.begin_replay()
            g.replay()
            opt.end_replay()
        return run
    res["graphed"] = compare({"torch": graphs["torch"].replay, "fused": replay_of(f_opt, graphs["fused"]),
                              "fused_ema": replay_of(e_opt, graphs["fused_ema"]),
                              "fused_then_foreach": replay_of(u_opt, graphs["fused_then_foreach"])}, args.reps, args.repeats)
    flush()
    if not args.no_profile:
        res["launches"] = {k: count_launches(fn) for k, fn in parts.items()}
        flush()
    del graphs, t_opt, f_opt, e_opt, u_opt, avg, weights, model, params
    torch.cuda.empty_cache()

    # ---- the whole graphed train step with either optimizer ----------------------------------------------------------------------------
    steps = {}
    for name in ("torch", "fused", "fused_ema"):
        torch.manual_seed(42)
        m = build_sr_model(arch, 4, 0.1).to(dev).train()
        opt = (torch.optim.AdamW(m.parameters(), lr=2e-5, weight_decay=0.0, capturable=True) if name == "torch"
               else FusedAdamW(m, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0, ema_decay=EMA_DECAY if name == "fused_ema" else None))
        gs = GraphedTrainStep(m, opt, max_grad_norm=1.0, warmup=2)
        gs(lr_img, hr_img)
        steps[name] = (lambda gs=gs: gs(lr_img, hr_img))
    res["graphed_train_step"] = compare(steps, max(args.reps // 5, 5), args.repeats, warm=3)
    flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_optim_ema_probe.json"))
    ap.add_argument("--archs", nargs="+", default=["hat", "dat"], choices=["hat", "dat"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "lr_patch": 64, "scale": 4, "reps": args.reps, "repeats": args.repeats,
           "ema_decay": EMA_DECAY,
           "note": "ms per step: median / min / max over `repeats` alternating windows of `reps` steps; cfg4 = hat, cfg5 = dat"}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for arch in args.archs:
        probe(arch, args, out, flush)
        r = out[arch]
        for mode in ("eager", "graphed", "graphed_train_step"):
            print(f"[{arch}] {mode:18s} " + "  ".join(f"{k} {v['device_ms']['median']:.3f} [{v['device_ms']['min']:.3f}-{v['device_ms']['max']:.3f}]"
                                                      f" (host {v['host_ms']['median']:.3f})" for k, v in r[mode].items()) + "  ms, device median [min-max]",
                  flush=True)
        print(f"[{arch}] launches {r.get('launches')}", flush=True)


if __name__ == "__main__":
    main()
