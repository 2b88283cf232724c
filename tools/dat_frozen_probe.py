"""Timing probe of the DAT x4 train step with batch statistics against frozen BatchNorm statistics (HIP events, MI355X): prints one JSON
document.

    python tools/dat_frozen_probe.py [--steps 24] [--out profiles/r07_dat_frozen_bn_probe.json] [--kernel-stats batch.csv frozen.csv]
    rocprofv3 --kernel-trace --stats -d DIR -o batch  -- python tools/dat_frozen_probe.py --trace-leg batch
    rocprofv3 --kernel-trace --stats -d DIR -o frozen -- python tools/dat_frozen_probe.py --trace-leg frozen

BASELINE cfg5 as a train step (DAT x4: dim 180, 6 x 6 blocks, split 8 x 32; 64 x 64 LR, batch 16, drop_path 0.1; fwd + L1 + bwd + fused
clip + AdamW), eager launches and one hipGraph replay per step (training.GraphedTrainStep).  Two models with the same weights live in the
one process -- one with every BatchNorm in training mode, one after training.freeze_batchnorm -- and their steps ALTERNATE, so that both
see the same clocks and the same neighbours; every step is bracketed by its own pair of events and the median is reported.  The
yardstick of the frozen step is the batch-statistics step of the same run.

--trace-leg runs a few eager steps of one mode and nothing else: the workload of a `rocprofv3 --kernel-trace --stats` run of its own
(tracing is never combined with the event timing above).  --kernel-stats takes the two kernel-stats CSVs of such runs and adds the
per-kernel split to the document: the kernels that differ between the modes, and the fused conv pass against the three passes it
replaces.  The kernel-source digest is computed as bench.py does, so a stored result names the library it was measured on.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import kernels_digest, synthetic_batch  # noqa: E402
from tpu_superresolution_amd.finetune_swinir import build_sr_model  # noqa: E402
from tpu_superresolution_amd.optim import FusedAdamW  # noqa: E402
from tpu_superresolution_amd.training import GraphedTrainStep, freeze_batchnorm, train_step  # noqa: E402

BATCH = 16


def make(frozen: bool, state):
    m = build_sr_model("dat", 4, 0.1).cuda()
    m.load_state_dict(state)
    m.train()
    if frozen:
        freeze_batchnorm(m)
    return m, FusedAdamW(m, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def alternate(steps: int, warmup: int, legs: dict) -> dict:
    """legs: name -> callable running one step; -> name -> sorted per-step milliseconds, the legs taking turns"""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    marks = {k: [] for k in legs}
    for _ in range(steps):
        for k, fn in legs.items():
            marks[k].append(timed(fn))
    torch.cuda.synchronize()
    return {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in marks.items()}


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(ms[0], 3), max_ms=round(ms[-1], 3), steps=len(ms))


def kernel_split(batch_csv: str, frozen_csv: str, steps: int) -> dict:
    def read(path):
        with open(path) as f:
            rows = list(csv.DictReader(f))
        return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3) for r in rows}

    def short(name):
        return name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    b, f = read(batch_csv), read(frozen_csv)
    out = {}
    for name in sorted(set(b) | set(f)):
        cb, tb = b.get(name, (0, 0.0))
        cf, tf = f.get(name, (0, 0.0))
        if cb != cf:          # the kernels whose launch count differs between the modes
            out[short(name)] = dict(batch_calls_per_step=cb / steps, batch_us_per_step=round(tb / steps, 1), frozen_calls_per_step=cf / steps,
                                    frozen_us_per_step=round(tf / steps, 1))
    tot_b, tot_f = sum(t for _, t in b.values()) / steps, sum(t for _, t in f.values()) / steps
    return dict(kernels_that_differ=out, batch_kernel_us_per_step=round(tot_b, 1), frozen_kernel_us_per_step=round(tot_f, 1), traced_steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-leg", choices=["batch", "frozen"], default=None)
    ap.add_argument("--trace-steps", type=int, default=3)
    ap.add_argument("--kernel-stats", nargs=2, metavar=("BATCH_CSV", "FROZEN_CSV"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(1234)
    state = {k: v.clone() for k, v in build_sr_model("dat", 4, 0.1).state_dict().items()}
    x, t = synthetic_batch(BATCH, torch.device("cuda", 0), seed=1000)
    if a.trace_leg:
        m, opt = make(a.trace_leg == "frozen", state)
        for _ in range(a.trace_steps):
            train_step(m, opt, x, t)
        torch.cuda.synchronize()
        print(f"traced {a.trace_steps} eager {a.trace_leg} steps")
        return
    assert a.steps >= 20, "the medians are over at least 20 steps"
    (mb, ob), (mf, of) = make(False, state), make(True, state)
    res = dict(probe="dat_frozen_bn", device=torch.cuda.get_device_name(0), kernels_digest=kernels_digest(),
               workload="DAT x4 train step (cfg5): 64x64 LR, batch 16, drop_path 0.1, fwd + L1 + bwd + fused clip + AdamW; batch-statistics and "
                        "frozen steps alternate in one process, one event pair per step")
    eager = alternate(a.steps, a.warmup, dict(batch=lambda: train_step(mb, ob, x, t), frozen=lambda: train_step(mf, of, x, t)))
    res["eager"] = {k: summary(v) for k, v in eager.items()}
    res["eager"]["frozen_over_batch"] = round(statistics.median(eager["frozen"]) / statistics.median(eager["batch"]), 4)
    gb, gf = GraphedTrainStep(mb, ob, warmup=1), GraphedTrainStep(mf, of, warmup=1)
    graphed = alternate(a.steps, a.warmup, dict(batch=lambda: gb(x, t), frozen=lambda: gf(x, t)))
    res["graphed"] = {k: summary(v) for k, v in graphed.items()}
    res["graphed"]["frozen_over_batch"] = round(statistics.median(graphed["frozen"]) / statistics.median(graphed["batch"]), 4)
    moved = sum(1 for k, v in mf.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked")) and not torch.equal(v.cpu(), state[k]))
    res["frozen_buffers_moved"] = moved
    if a.kernel_stats:
        res["kernel_split"] = kernel_split(a.kernel_stats[0], a.kernel_stats[1], a.trace_steps)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
