"""Developer probe: the two tiling kernels (csrc/tile.hip) alone, and tiling.tiled_forward beside the whole-image call.

Part 1, kernels alone, on a 512 x 512 LR image at B = 1, C = 3: tile 64 / overlap 32 (15 x 15 tiles) and tile 256 / overlap 32 (3 x 3),
output scale s in {2, 4}.  `gather` crops every tile of the LR image in one launch; `merge_mean` / `merge_center` merge every output
tile (tile s x tile s pixels each) into the s-times larger image in one launch.  Beside each: a device-to-device `copy_` moving the
same number of bytes, and the copy ceilings of profiles/r01_hbm_ceilings.txt.  Bytes per launch are counted from the shapes: gather
reads and writes N B C th tw floats; merge 'mean' reads N B C th tw floats and writes B C Ho Wo; merge 'center' reads and writes
B C Ho Wo (every output pixel has one owner).

Part 2: the SwinIR-light x2 of bench.py's cfg2 on one 256 x 256 LR image, whole, and through tiled_forward at tile 64 / overlap 32
with 1 and 16 tiles per model call; the same chunked gather / merge launches are then timed without the model, which gives the
share of a tiled pass the two kernels take.

Kernel launches are bracketed by HIP events behind a spin kernel (as tools/d4_probe.py), variants alternating, median / min / max of
`--launches`; the model passes are host-clocked around a device synchronise, median of `--passes`.

    python tools/tile_probe.py --out profiles/tile_probe.json
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tpu_superresolution_amd import tiling as T  # noqa: E402
from tpu_superresolution_amd._lib import check, lib  # noqa: E402


def _stream():
    return torch.cuda.current_stream().cuda_stream


def gather(x, tiles, t0, n, th, tw, sy, sx):
    B, C, H, W = x.shape
    check(lib().srk_tile_gather_f32(x.data_ptr(), tiles.data_ptr(), t0, n, B, C, H, W, th, tw, sy, sx, _stream()))


def merge(tiles, out, t0, n, th, tw, sy, sx, mode):
    B, C, H, W = out.shape
    check(lib().srk_tile_merge_f32(tiles.data_ptr(), out.data_ptr(), t0, n, B, C, H, W, th, tw, sy, sx, mode, _stream()))


def copy_ceilings():
    """The 'copy (1R:1W)' lines of profiles/r01_hbm_ceilings.txt: {MB: TB/s}."""
    out = {}
    path = os.path.join(ROOT, "profiles", "r01_hbm_ceilings.txt")
    for line in open(path):
        m = re.match(r"\s*(\d+) MB copy\s+\(1R:1W\):\s+[\d.]+ us\s+([\d.]+) TB/s", line)
        if m:
            out[f"{m.group(1)} MB"] = float(m.group(2))
    return out


def time_variants(variants, launches, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    e0.record()
    torch.cuda._sleep(1_000_000)
    e1.record()
    torch.cuda.synchronize()
    spin = max(1, int(1_000_000 * 0.1 / e0.elapsed_time(e1)))          # about 100 us
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
    return times


def kernels_alone(lr, C, tile, overlap, s, launches, warmup):
    x = torch.rand(1, C, lr, lr, device="cuda")
    st = tile - overlap
    k = len(T.tile_origins(lr, tile, overlap))
    N = k * k
    tiles = torch.empty(N, C, tile, tile, device="cuda")
    y = torch.rand(N, C, tile * s, tile * s, device="cuda")
    out = torch.empty(1, C, lr * s, lr * s, device="cuda")
    moved = {"gather": 2 * tiles.numel() * 4, "merge_mean": (y.numel() + out.numel()) * 4, "merge_center": 2 * out.numel() * 4}
    variants = {"gather": lambda: gather(x, tiles, 0, N, tile, tile, st, st),
                "merge_mean": lambda: merge(y, out, 0, N, tile * s, tile * s, st * s, st * s, 0),
                "merge_center": lambda: merge(y, out, 0, N, tile * s, tile * s, st * s, st * s, 1)}
    for name, nbytes in list(moved.items()):                             # a copy_ moving the same bytes
        src = torch.rand(nbytes // 8, device="cuda")
        dst = torch.empty_like(src)
        variants[f"copy_as_{name}"] = (lambda src=src, dst=dst: dst.copy_(src))
    times = time_variants(variants, launches, warmup)
    res = {"lr": lr, "C": C, "tile": tile, "overlap": overlap, "scale": s, "tiles": N, "variants": {}}
    for name, v in times.items():
        med = statistics.median(v)
        nbytes = moved[name.replace("copy_as_", "")]
        res["variants"][name] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "bytes": nbytes,
                                 "tb_per_s": round(nbytes / med / 1e6, 3)}
        print(f"lr {lr} tile {tile} overlap {overlap} x{s}  {name:22s} {med:9.2f} us  [{min(v):.2f} - {max(v):.2f}]  "
              f"{nbytes / 2**20:8.1f} MiB  {nbytes / med / 1e6:.2f} TB/s", flush=True)
    return res


def host_clocked(fn, passes, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def model_passes(lr, tile, overlap, passes, warmup):
    import tpu_superresolution_amd as P
    torch.manual_seed(42)
    m = P.SwinIR(upscale=2, in_chans=3, img_size=64, window_size=8, img_range=1.0, depths=[6] * 4, embed_dim=60, num_heads=[6] * 4,
                 mlp_ratio=2, upsampler="pixelshuffledirect").cuda().eval()
    x = torch.rand(1, 3, lr, lr, device="cuda")
    s, st = 2, tile - overlap
    k = len(T.tile_origins(lr, tile, overlap))
    N = k * k
    res = {"model": "SwinIR-light x2 (bench.py cfg2)", "lr": lr, "tile": tile, "overlap": overlap, "tiles": N, "passes": passes}
    with torch.no_grad():
        res["whole_image"] = host_clocked(lambda: m(x), passes, warmup)
        print(f"whole image {lr} x {lr}: {res['whole_image']}", flush=True)
        for tb in (1, 16):
            tiles = torch.empty(tb, 3, tile, tile, device="cuda")
            y = torch.rand(tb, 3, tile * s, tile * s, device="cuda")
            out = torch.empty(1, 3, lr * s, lr * s, device="cuda")

            def kernels_only():
                for t0 in range(0, N, tb):
                    n = min(tb, N - t0)
                    gather(x, tiles, t0, n, tile, tile, st, st)
                    merge(y, out, t0, n, tile * s, tile * s, st * s, st * s, 0)
            tiled = host_clocked(lambda: T.tiled_forward(m, x, tile, overlap, tile_batch=tb), passes, warmup)
            alone = host_clocked(kernels_only, passes, warmup)
            res[f"tile_batch_{tb}"] = {"model_calls": -(-N // tb), "tiled_forward": tiled, "gather_and_merge_launches_alone": alone,
                                       "kernels_share_of_tiled_pass": round(alone["median_ms"] / tiled["median_ms"], 4),
                                       "tiled_over_whole": round(tiled["median_ms"] / res["whole_image"]["median_ms"], 3)}
            print(f"tile_batch {tb}: {res[f'tile_batch_{tb}']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_probe.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--passes", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the probe measures on the GPU (no CPU fallback)")
    if args.launches < 20:
        raise SystemExit("--launches: at least 20 (the figure is a median)")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup,
           "copy_ceilings_tb_per_s_from_profiles_r01_hbm_ceilings": copy_ceilings(),
           "note": "kernels_alone: us per launch between two HIP events, median / min / max, variants alternating; bytes = what the launch "
                   "reads plus writes, counted from the shapes; tb_per_s = bytes / median.  copy_as_<k> is a device-to-device copy_ of "
                   "the same byte count.  Buffers below 256 MiB stay in the Infinity Cache between launches, for the copy as for the "
                   "kernel: compare a kernel with its copy, not with HBM.  model: host clock around a device synchronise, ms per pass; "
                   "gather_and_merge_launches_alone = the chunked launches of one tiled pass without the model calls",
           "kernels_alone": [], "model": None}
    for tile in (64, 256):
        for s in (2, 4):
            res["kernels_alone"].append(kernels_alone(512, 3, tile, 32, s, args.launches, args.warmup))
    res["model"] = model_passes(256, 64, 32, args.passes, 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
