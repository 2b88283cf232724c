"""Developer probe: the launch time of the engine's one-step upsample head ('pixelshuffledirect') by its width, and its share of a
SwinIR-light x4 forward.

The head is the last conv-GEMM launch of srk_swinir_forward and has no entry point of its own, so it is timed with the library's launch
probe (srk_probe_begin / srk_probe_end: HIP events around the launches of one kernel family).  A light-width model with ONE RSTB launches
three conv GEMMs per forward (the RSTB conv, conv_after_body, the head); behind one forward_features call (one conv GEMM: the RSTB conv)
the head is launch 3, so with probe_stride 3 the probe brackets launches 0 and 3: that RSTB conv and the head.  The same conv alone is
probed in a pass of its own and subtracted.  Every probed pass starts behind a spin kernel (the host is ahead of the device, as in
tools/predict_probe.py); the widths alternate; median / min / max of `--launches`.

B = 1, 256 x 256, embed 60: M = 65 536 rows for every width; N = upscale^2 * in_chans = 12, 16 (one n-block: the path that was there
before), 25, 27, 48, 64 (2, 2, 3, 4 n-blocks of 16 columns).  With SRK_LIB_PATH naming a library of the commit before the head was widened,
`--heads 12,16` gives that library's launch at the same M.

    python tools/wide_head_probe.py --out profiles/wide_head_probe.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import tpu_superresolution_amd as pkg  # noqa: E402
from tpu_superresolution_amd._lib import check, lib  # noqa: E402

from tile_probe import time_variants  # noqa: E402  (tools/tile_probe.py: the protocol is shared, not restated)

HEADS = {12: (2, 3), 16: (4, 1), 25: (5, 1), 27: (3, 3), 48: (4, 3), 64: (8, 1)}          # N: (upscale, in_chans)
FAM_GEMM_CONV = 2


def light(s, c, depths):
    torch.manual_seed(42)
    return pkg.SwinIR(upscale=s, in_chans=c, img_size=64, window_size=8, img_range=1.0, depths=depths, embed_dim=60, num_heads=[6] * len(depths),
                      mlp_ratio=2, upsampler="pixelshuffledirect", drop_path_rate=0.0).cuda().eval()


def probed(fn):
    """-> (ms summed over the bracketed launches, their count)"""
    check(lib().srk_probe_begin(FAM_GEMM_CONV, 8))
    fn()
    ms, n = C.c_double(), C.c_int()
    check(lib().srk_probe_end(C.byref(ms), None, None, C.byref(n)))
    return ms.value, n.value


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_head_probe.json"))
    ap.add_argument("--heads", default="16,27,48,64,12,25", help="comma-separated head widths N out of " + str(sorted(HEADS)))
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip_forward", action="store_true", help="leave out the SwinIR-light x4 forward (the head's share of it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    torch.cuda.set_device(0)
    heads = [int(v) for v in args.heads.split(",")]
    side = args.side
    models, xs, feats = {}, {}, torch.rand(1, 60, side, side, device="cuda")
    with torch.no_grad():
        for N in heads:
            s, c = HEADS[N]
            models[N] = light(s, c, [2])
            xs[N] = torch.rand(1, c, side, side, device="cuda")
            for _ in range(args.warmup):
                models[N].forward_features(feats)
                models[N](xs[N])
        # the launch pattern the subtraction relies on: one conv GEMM per forward_features, three per forward
        check(lib().srk_set_option(b"probe_stride", 1))
        for N in heads:
            assert probed(lambda: models[N].forward_features(feats))[1] == 1 and probed(lambda: models[N](xs[N]))[1] == 3, "launch pattern changed"
        check(lib().srk_set_option(b"probe_stride", 3))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)
        e0.record()
        torch.cuda._sleep(1_000_000)
        e1.record()
        torch.cuda.synchronize()
        spin = max(1, int(1_000_000 * 0.1 / e0.elapsed_time(e1)))          # about 100 us
        both, conv = {N: [] for N in heads}, {N: [] for N in heads}
        for _ in range(args.launches):
            for N in heads:
                m, x = models[N], xs[N]
                torch.cuda._sleep(spin)
                ms, n = probed(lambda: (m.forward_features(feats), m(x)))
                assert n == 2
                both[N].append(ms * 1e3)
                torch.cuda._sleep(spin)
                ms, n = probed(lambda: m.forward_features(feats))
                assert n == 1
                conv[N].append(ms * 1e3)
        check(lib().srk_set_option(b"probe_stride", 1))
        res = {"device": torch.cuda.get_device_name(0), "library": "SRK_LIB_PATH" if os.environ.get("SRK_LIB_PATH") else "in-tree", "side": side,
               "M": side * side, "K": 9 * 64, "launches": args.launches,
               "note": "head_us = (RSTB conv + head, two bracketed launches of one probed pass) - median(the RSTB conv alone, its own probed pass); us "
                       "between HIP events behind a spin kernel, widths alternating.  n_blocks = N / 16 rounded up: 16-column blocks of the narrow "
                       "image-head kernel, each reading the 128-row A tile of its M-tile again (from the XCD's L2: the blocks of one M-tile are "
                       "neighbours in the tile order)", "heads": {}}
        for N in heads:
            c_med = statistics.median(conv[N])
            head = [b - c_med for b in both[N]]
            s, c = HEADS[N]
            res["heads"][str(N)] = {"upscale": s, "in_chans": c, "n_blocks": (N + 15) // 16, "head_us": _stats(head), "rstb_conv_us": _stats(conv[N]),
                                    "out_bytes": side * side * N * 4}
            print(f"N={N:3d} (x{s}, {c} ch, {(N + 15) // 16} n-blocks): head {res['heads'][str(N)]['head_us']}  rstb conv {res['heads'][str(N)]['rstb_conv_us']}", flush=True)
        if not args.skip_forward and 48 in heads:
            full = light(4, 3, [6] * 4)
            x = torch.rand(1, 3, side, side, device="cuda")
            t = time_variants({"light_x4_forward": lambda: full(x)}, args.launches, args.warmup)["light_x4_forward"]
            res["light_x4_forward_us"] = _stats(t)
            res["head_share_of_light_x4_forward"] = round(res["heads"]["48"]["head_us"]["median_us"] / res["light_x4_forward_us"]["median_us"], 4)
            print("SwinIR-light x4 forward:", res["light_x4_forward_us"], "head share", res["head_share_of_light_x4_forward"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
