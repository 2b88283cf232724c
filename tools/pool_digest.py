"""Developer tool: sha256 digests of what the on-device data path returns, for comparing two trees bit for bit (no timing in it).

`pool_configs()` names the pools of tests/test_gpu_image_ops_launches.py: three 40 x 48 uint8 images, one of them gray, P 8, x2, B 3,
augment d4.  For each, `random` is seeded and four batches are drawn; every returned tensor's raw bytes go into one sha256.  `op_digests()`
adds `degrade_blind`, `degrade_psf`, `restore_degrade` and `degrade_second_order` on one fixed 2 x 3 x 24 x 24 input.  One JSON object
is printed (and written with --out).  Run it in a fresh process per tree; `--compare A.json B.json` joins two outputs key for key.

    python tools/pool_digest.py --out profiles/digest.json
    python tools/pool_digest.py --compare parent.json branch.json --out profiles/image_ops_refactor_digests.json
"""
import argparse
import hashlib
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, S, B, MARGIN = 8, 2, 3, 2
INDICES = [0, 1, 2]


def images():
    import numpy as np
    rng = np.random.RandomState(7)
    return [rng.randint(0, 256, (40, 48, 3), dtype=np.uint8), rng.randint(0, 256, (40, 48), dtype=np.uint8),
            rng.randint(0, 256, (40, 48, 3), dtype=np.uint8)]


def pool_configs():
    """name -> a function building that pool (the package is imported by the caller's `sys.path`)."""
    from tpu_superresolution_amd import sr_datasets as D
    im = images()
    hr = dict(lr_patch=P, scale=S, augment="d4")
    return {
        "pair": lambda: D.DevicePairPool([(a[::S, ::S].copy(), a) for a in im], P, S, augment="d4"),
        "hr": lambda: D.DeviceHRPool(im, **hr),
        "hr_degrade": lambda: D.DeviceHRPool(im, degrade=D.DegradeSpec(), **hr),
        "hr_psf_host": lambda: D.DeviceHRPool(im, degrade=D.DegradeSpec(), psf=D.PsfSpec(mode="mixed"), tables="host", **hr),
        "hr_psf_device": lambda: D.DeviceHRPool(im, degrade=D.DegradeSpec(), psf=D.PsfSpec(mode="mixed"), tables="device", **hr),
        "hr_jpeg": lambda: D.DeviceHRPool(im, jpeg=D.JpegSpec(), **hr),
        "hr2": lambda: D.DeviceHR2Pool(im, P, S, D.SecondOrderSpec(ksize=(3, 7)), margin=MARGIN, augment="d4"),
        "hr2_usm": lambda: D.DeviceHR2Pool(im, P, S, D.SecondOrderSpec(ksize=(3, 7)), margin=MARGIN, augment="d4", usm=D.UsmSpec(radius=3)),
        "restore": lambda: D.DeviceRestorePool(im, P, spec=D.RestoreSpec(sigma=(0.0, 0.2), jpeg_quality=(30, 95)), augment="d4"),
    }


def _sha(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def pool_digests():
    out = {}
    for name, make in pool_configs().items():
        pool = make()
        random.seed(1)
        out["pool:" + name] = _sha([t for _ in range(4) for t in pool.sample(INDICES)])
    return out


def op_digests():
    import torch
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd import ops
    x = torch.rand(2, 3, 24, 24, generator=torch.Generator().manual_seed(3)).cuda()
    x = (x * 255).round() / 255
    psf = [bk.gaussian(5, 1.2, 0.7, 0.4), bk.plateau(7, 2.0, 1.0, 0.4, 1.2)]
    chain = [ops.SecondOrder(bk.gaussian(7, 1.5, 0.8, 0.3), 1.3, (0.03, 0.0), False, 60, bk.sinc(2.0, 7), 0.7, (0.02, 0.01), True, 45, False,
                             bk.sinc(2.5, 5), 11),
             ops.SecondOrder(bk.sinc(1.8, 9), 0.6, (0.05, 0.02), True, 35, bk.delta(), 1.1, (0.04, 0.0), False, 80, True, bk.delta(), 12,
                             (1, 2, 0))]
    return {
        "op:degrade_blind": _sha(ops.degrade_blind(x, 2, [(1.0, 0.5), (0.3, 2.0)], (0.02, 0.01), [5, 6], [False, True])),
        "op:degrade_psf": _sha(ops.degrade_psf(x, 2, psf, (0.02, 0.0), [5, 6], False)),
        "op:restore_degrade": _sha([ops.restore_degrade(x, (0.05, 0.0), [1, 2], False, [0, 40], True, 8)]),
        "op:restore_degrade_no_jpeg": _sha([ops.restore_degrade(x, [(0.05, 0.0), (0.0, 0.1)], [1, 2], [True, False])]),
        "op:degrade_second_order": _sha([ops.degrade_second_order(x, 2, chain)]),
    }


def compare(a_path, b_path):
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    keys = sorted(set(a) | set(b))
    return {"what": "tools/pool_digest.py in a checkout of the parent commit and in this tree, each in a fresh process: sha256 of the raw "
                    "bytes of every tensor of four seeded `sample` calls per pool, and of four ops on one fixed input",
            "parent": a, "branch": b, "equal": {k: a.get(k) == b.get(k) and k in a for k in keys},
            "all_equal": all(a.get(k) == b.get(k) and k in a for k in keys)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is imported")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_JSON", "BRANCH_JSON"), default=None)
    args = ap.parse_args()
    if args.compare:
        res = compare(*args.compare)
    else:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("the digests are of device results (no CPU fallback)")
        torch.cuda.set_device(0)
        res = {**pool_digests(), **op_digests()}
        torch.cuda.synchronize()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.compare and not res["all_equal"]:
        raise SystemExit("the digests differ")


if __name__ == "__main__":
    main()
