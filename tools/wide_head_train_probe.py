"""Developer probe: the three launches of the wide one-step head's backward (csrc/headconv_wide.hip) on preallocated buffers
-> profiles/wide_head_train_probe.json.

    python tools/wide_head_train_probe.py [--out profiles/wide_head_train_probe.json] [--launches 50]

Shapes: the light family's own training shape, B 32 of 64 x 64 LR patches, 60 -> 48 channels (x4 RGB), and 180 -> 48 at the same
geometry.  Each C entry runs alone between two HIP events, each bracket queued behind a ~100 us spin kernel (the bracket holds device
time, not the launch path); median / min / max over `launches` brackets, the entries alternating.

The yardstick, timed beside them, is what the library could already do at that geometry with a bf16 gradient: srk_conv3x3_wgrad_bf16
and the LD_CONV3 dgrad of srk_gemm_ex on a bf16 copy of gy padded to 64 channels.  That path rounds the gradient to bf16 and is no
substitute; `pair_over_yardstick` = (widehead_wgrad + widehead_dgrad) / (yardstick_wgrad + yardstick_dgrad), expected <= 1.5.
flop = 2 * pixels * Cin * Co * 9 per launch; TF/s of the fp32-input MFMA against its 157 TF/s peak.  No gate.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd import _lib as LIB  # noqa: E402
from tpu_superresolution_amd._lib import _p, _stream, check, lib  # noqa: E402


def probe(shape, launches, warmup, spin):
    B, H, W, Cin, CinP, Co, CoP, r, Cimg = shape
    M = B * H * W
    g = torch.Generator().manual_seed(0)
    dev = dict(device="cuda")
    x = torch.randn(M, CinP, generator=g).to(torch.bfloat16).cuda()
    d_pred = torch.randn(B, Cimg, H * r, W * r, generator=g).cuda()
    gy = torch.empty(M, CoP, dtype=torch.float32, **dev)
    w = (0.1 * torch.randn(Co, Cin, 3, 3, generator=g)).cuda()
    dw, db = torch.zeros(Co, Cin, 3, 3, **dev), torch.zeros(Co, **dev)
    dx = torch.empty(M, CinP, dtype=torch.bfloat16, **dev)
    # the yardstick's operands: gy as bf16 padded to 64 channels, packed bf16 weights [CinP][9 * 64], dW fp32 [64][9 * CinP]
    gy16 = torch.zeros(M, 64, dtype=torch.bfloat16, **dev)
    wt16 = (0.1 * torch.randn(CinP, 9 * 64, generator=g)).to(torch.bfloat16).cuda()
    dw_y, db_y = torch.zeros(64, 9 * CinP, **dev), torch.zeros(64, **dev)
    dx_y = torch.empty(M, CinP, dtype=torch.bfloat16, **dev)
    L, s = lib(), _stream()
    ws = torch.empty(int(L.srk_wgrad_workspace_bytes()), dtype=torch.uint8, **dev)      # the yardstick's split partials (its fast path)
    check(L.srk_set_wgrad_workspace(_p(ws), ws.numel()))
    check(L.srk_widehead_grad_prep(_p(d_pred), _p(gy), B, Cimg, H * r, W * r, H, W, r, CoP, 1.0, s))
    gy16[:, :CoP] = gy.to(torch.bfloat16)
    a = LIB.GemmArgs()
    a.loader, a.epilogue = LIB.LD_CONV3, LIB.EP_BF16
    a.A, a.W, a.M, a.N, a.K = _p(gy16), _p(wt16), M, CinP, 9 * 64
    a.B, a.H, a.Wd, a.CinP = B, H, W, 64
    a.outb, a.ldo = _p(dx_y), CinP

    entries = {
        "widehead_grad_prep": lambda: check(L.srk_widehead_grad_prep(_p(d_pred), _p(gy), B, Cimg, H * r, W * r, H, W, r, CoP, 1.0, s)),
        "widehead_wgrad": lambda: check(L.srk_widehead_wgrad(_p(x), _p(gy), _p(dw), _p(db), B, H, W, Cin, CinP, Co, CoP, s)),
        "widehead_dgrad": lambda: check(L.srk_widehead_dgrad(_p(gy), _p(w), _p(dx), B, H, W, Cin, CinP, Co, CoP, s)),
        "yardstick_wgrad_bf16": lambda: check(L.srk_conv3x3_wgrad_bf16(_p(gy16), _p(x), _p(dw_y), _p(db_y), B, H, W, CinP, 64, s)),
        "yardstick_dgrad_bf16": lambda: check(L.srk_gemm_ex(C.byref(a), s)),
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
    check(L.srk_set_wgrad_workspace(None, 0))
    flop = 2.0 * M * Cin * Co * 9
    res = {}
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        if k in ("widehead_wgrad", "widehead_dgrad"):
            res[k]["TF_per_s"] = round(flop / med / 1e6, 1)
        print(f"{B}x{H}x{W} {Cin}->{Co} {k:24s} {med:9.2f} us  [{min(v):.2f} - {max(v):.2f}]", flush=True)
    pair = res["widehead_wgrad"]["median_us"] + res["widehead_dgrad"]["median_us"]
    yard = res["yardstick_wgrad_bf16"]["median_us"] + res["yardstick_dgrad_bf16"]["median_us"]
    res["pair_us"], res["yardstick_pair_us"], res["pair_over_yardstick"] = round(pair, 2), round(yard, 2), round(pair / yard, 3)
    res["flop_per_launch"] = flop
    print(f"{B}x{H}x{W} {Cin}->{Co} pair {pair:.2f} us, yardstick {yard:.2f} us, ratio {pair / yard:.3f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_head_train_probe.json"))
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
    res = {"probe": "wide_head_train", "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup,
           "spin_cycles_before_each_bracket": spin,
           "note": "us per C entry between two HIP events behind a spin kernel: median / min / max over `launches` brackets, entries "
                   "alternating; the yardstick is the bf16-gradient path (srk_conv3x3_wgrad_bf16 + LD_CONV3 dgrad of srk_gemm_ex at 64 "
                   "padded channels), which loses the fp32 gradient; expectation pair_over_yardstick <= 1.5; no gate", "shapes": {}}
    for shape in ((32, 64, 64, 60, 64, 48, 48, 4, 3), (32, 64, 64, 180, 192, 48, 48, 4, 3)):
        res["shapes"][f"{shape[0]}x{shape[1]}x{shape[2]}_{shape[3]}to{shape[5]}"] = probe(shape, args.launches, args.warmup, spin)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
