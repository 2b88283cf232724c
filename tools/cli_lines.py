"""What the two scripts print and save, once per branch of their main(): the record that a change of the command-line layer compares.

    python tools/cli_lines.py --out lines.json                       (needs the GPU)
    python tools/cli_lines.py --compare parent.json branch.json --out profiles/cli_refactor_lines.json

It builds the tiny data set of the script tests (four 96 x 96 RGB PNGs per split, LR directories for the paired runs), runs
finetune_swinir.main for one epoch and evaluate.main on the checkpoint for each of RUNS, and keeps of every run the printed lines that
hold no timing, loss or PSNR (those that start with one of KEEP), the key set of each checkpoint and its 'args' dict.  The working
directory reads '@W' in what is kept.  --compare writes both records and whether they are equal (exit status 1 if not)."""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZE = 96
KEEP = ("[task", "[synth_lr]", "[degrade]", "[gpu_data]", "[weights]", "[params]", "[freeze", "[val_tile]", "[data]", "[save]", "[tile]", "[ckpt]",
        "[self_ensemble]")
SYNTH = ["--gpu_data", "--synth_lr"]
# name, scale, training flags, evaluation flags ('@W' = the working directory)
RUNS = (
    ("paired_host", "X2", [], []),
    ("gpu_data_paired", "X2", ["--gpu_data", "--weights", "@W/paired_host/best_swinir_finetune_X2.pt", "--freeze_regex", "conv_first", "--val_tile",
                               "32", "--val_tile_overlap", "8", "--ema_decay", "0.999"],
     ["--tile", "32", "--tile_overlap", "8", "--save_indices", "0,2", "--self_ensemble", "--param_key", "params_ema"]),
    ("synth_jpeg", "X2", SYNTH + ["--jpeg_quality", "30", "95"], ["--synth_lr", "--jpeg_quality", "60"]),
    ("blind_mixed_device", "X2", SYNTH + ["--degrade", "blind", "--blur_kernel", "mixed", "--degrade_tables", "device"],
     ["--synth_lr", "--degrade", "blind", "--blur_theta", "30"]),
    ("blind_psf", "X2", SYNTH + ["--degrade", "blind", "--blur_psf", "@W/psf.npy"], ["--synth_lr", "--degrade", "blind", "--blur_psf", "@W/psf.npy"]),
    ("second_order_usm", "X2", SYNTH + ["--degrade", "second_order", "--gt_usm", "--resize_mode_prob", "0.2", "0.3", "0.5"],
     ["--synth_lr", "--degrade", "second_order", "--gt_usm"]),
    ("dn_gray", "X1", ["--task", "dn", "--channels", "1", "--dn_sigma", "15", "50"], ["--task", "dn", "--channels", "1", "--dn_sigma", "25"]),
    ("car", "X1", ["--task", "car", "--jpeg_quality", "10", "40"], ["--task", "car", "--jpeg_quality", "10", "--bench_metric", "y"]),
)


def make_dataset(work: str) -> None:
    import numpy as np
    from PIL import Image

    from tpu_superresolution_amd import blur_kernels as bk
    rs = np.random.RandomState(0)
    for split in ("train", "valid", "test"):
        hr_dir = os.path.join(work, "shuffled2D", f"shuffled2D_{split}_HR")
        lr_dir = os.path.join(work, "shuffled2D", f"shuffled2D_{split}_LR_default_X2")
        os.makedirs(hr_dir)
        os.makedirs(lr_dir)
        for i in range(4):
            base = (rs.rand(SIZE // 4 + 1, SIZE // 4 + 1, 3) * 255).astype(np.uint8)
            hr = Image.fromarray(base).resize((SIZE, SIZE), Image.BICUBIC)
            hr.save(os.path.join(hr_dir, f"{i:04d}.png"))
            hr.resize((SIZE // 2, SIZE // 2), Image.BICUBIC).save(os.path.join(lr_dir, f"{i:04d}x2.png"))
    np.save(os.path.join(work, "psf.npy"), np.stack([bk.gaussian(5, 1.0, 2.0, 0.3), bk.gaussian(5, 0.7, 0.7)]))


def train_argv(work: str, scale: str, flags: list) -> list:
    return ["--data_root", work, "--scale", scale, "--epochs", "1", "--batch_size", "2", "--lr_patch", "16", "--workers", "0",
            *[a.replace("@W", work) for a in flags]]


def eval_argv(work: str, here: str, scale: str, flags: list) -> list:
    return ["--scale", scale, "--data_root", work, "--ckpt", os.path.join(here, f"bestpsnr_swinir_finetune_{scale}.pt"), "--batch_size", "2",
            "--arch", "swinir", "--device", "cuda", "--save_dir", os.path.join(here, "preds"), "--save_n", "2", *[a.replace("@W", work) for a in flags]]


def _plain(v, work):
    if isinstance(v, str):
        return v.replace(work, "@W")
    if isinstance(v, (list, tuple)):
        return [_plain(x, work) for x in v]
    return v


def _kept(text: str, work: str) -> list:
    return [_plain(ln, work) for ln in text.splitlines() if ln.startswith(KEEP)]


def record() -> dict:
    import torch

    from tpu_superresolution_amd import evaluate, finetune_swinir
    out = {}
    with tempfile.TemporaryDirectory() as work:
        make_dataset(work)
        for name, scale, train, ev in RUNS:
            here = os.path.join(work, name)
            os.makedirs(here)
            os.chdir(here)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                finetune_swinir.main(train_argv(work, scale, train))
            run = {"train_lines": _kept(buf.getvalue(), work), "checkpoints": {}}
            for f in sorted(os.listdir(here)):
                ck = torch.load(os.path.join(here, f), map_location="cpu", weights_only=False)
                run["checkpoints"][f] = {"keys": sorted(ck), "args": {k: _plain(v, work) for k, v in sorted(ck["args"].items())}}
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                evaluate.main(eval_argv(work, here, scale, ev))
            run["eval_lines"] = _kept(buf.getvalue(), work)
            out[name] = run
            print(f"[cli_lines] {name}: {len(run['train_lines'])} + {len(run['eval_lines'])} lines, {len(run['checkpoints'])} checkpoints", flush=True)
            os.chdir(work)
        os.chdir(ROOT)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "BRANCH"), default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    if args.compare:
        parent, branch = (json.load(open(p)) for p in args.compare)
        doc = {"equal": parent == branch, "runs": list(parent), "parent": parent, "branch": branch}
        diff = [n for n in sorted(set(parent) | set(branch)) if parent.get(n) != branch.get(n)]
        print(f"[cli_lines] equal: {doc['equal']}" + (f"; differing runs: {diff}" if diff else ""))
    else:
        doc = record()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0 if not args.compare or doc["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
