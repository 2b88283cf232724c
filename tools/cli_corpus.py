"""Characterization corpus of the two command lines (finetune_swinir.parse_args, evaluate.parse_args).

    python tools/cli_corpus.py --write [--out tests/cli_corpus.json]

--write records, in the checkout it runs in, what both parsers make of a list of command lines and the shape of the parsers themselves;
tests/test_cli_corpus.py compares a later checkout with that record.  The list is every command line that the host tests named in
HARVEST feed to either parse_args (collected by running them with both functions wrapped), plus EXTRA: lines with two faults each,
which pin the order of the checks, and --blur_psf lines against a small table.  A file a line names by absolute path is kept in
the record ("files", base64) and the path is written '@F/<name>'; whoever replays the line writes the files into a directory first.
Only names that every checkout has are used here (parse_args, the nine spec functions, saved_args), so that the record can be made at
any commit.  No GPU."""
from __future__ import annotations

import argparse
import base64
import contextlib
import hashlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HARVEST = ("test_degrade2_cli", "test_tables_cli", "test_restore_host", "test_psf_host", "test_usm_host", "test_jpeg_ref", "test_degrade_ref",
           "test_loss_ref", "test_fft_loss_ref", "test_tile_ref", "test_bench_metric_script", "test_augment_host", "test_wsmall_train_host",
           "test_resize_ref", "test_image_ops_host")
TRAIN_SPECS = ("degrade_spec", "psf_spec", "jpeg_spec", "usm_spec", "second_order_spec", "restore_spec")
EVAL_SPECS = ("eval_restore", "eval_usm", "eval_psf")
PSF = "@F/own_psf.npy"

_T = ["--data_root", "D", "--scale", "X2"]
_S = _T + ["--gpu_data", "--synth_lr"]
_B = _S + ["--degrade", "blind"]
_ON = _S + ["--degrade", "second_order"]
_E = ["--scale", "X2", "--ckpt", "F", "--arch", "swinir"]
_ES = _E + ["--synth_lr"]
EXTRA = [("finetune", a) for a in (
    # two faults each: the one reported is the one checked first
    ["--data_root", "D", "--scale", "X1", "--channels", "1"],
    _T + ["--task", "dn", "--arch", "hat"],
    ["--data_root", "D", "--scale", "X1", "--task", "dn", "--synth_lr"],
    ["--data_root", "D", "--scale", "X1", "--task", "car", "--jpeg_p", "0.5"],
    ["--data_root", "D", "--scale", "X1", "--task", "car", "--jpeg_quality", "10", "40", "--channels", "1", "--val_bench_metric", "y", "--dn_sigma",
     "5", "1"],
    _T + ["--synth_lr", "--degrade", "blind", "--blur_sigma", "0.2", "3.0"],
    _T + ["--degrade", "blind", "--sinc_p", "0.2"],
    _ON + ["--synth_lr_bits", "0", "--jpeg_p", "0.5"],
    _ON + ["--sinc_p", "1.5", "--degrade_margin", "65"],
    _ON + ["--degrade_margin", "65", "--gt_usm", "--usm_radius", "99"],
    _T + ["--sinc_p", "0.2", "--gt_usm"],
    _T + ["--gt_usm", "--usm_weight", "0.5", "--blur_kernel", "rotated"],
    _ON + ["--usm_weight", "0.5", "--blur_psf", "F.npy", "--blur_kernel", "mixed"],
    _B + ["--blur_ksize", "7", "9", "--degrade_tables", "device"],
    _B + ["--blur_kernel", "mixed", "--blur_ksize", "8", "9", "--jpeg_p", "0.5"],
    _T + ["--degrade_tables", "device", "--jpeg_p", "0.5"],
    _S + ["--jpeg_quality", "0", "90", "--synth_lr_bits", "0"],
    _T + ["--jpeg_quality", "30", "90", "--val_tile", "-1"],
    _T + ["--val_tile", "-1", "--val_crop_border", "2"],
    _T + ["--val_crop_border", "2", "--ssim_weight", "-1"],
    _T + ["--ssim_weight", "-1", "--fft_weight", "-1"],
    _T + ["--fft_weight", "0.1", "--lr_patch", "300", "--charbonnier_eps", "0"],
    _T + ["--charbonnier_eps", "0", "--ema_decay", "1"],
    _T + ["--ema_decay", "1", "--window_size", "9"],
    _T + ["--window_size", "9", "--arch", "hat"],
    _T + ["--window_size", "4", "--arch", "hat", "--graph"],
    # --blur_psf against a table of this tool's own
    _B + ["--blur_psf", PSF],
    _B + ["--blur_psf", PSF, "--degrade_tables", "device", "--jpeg_quality", "30", "95", "--degrade_seed", "3"],
    _ON + ["--blur_psf", PSF, "--gt_usm", "--resize_mode_prob", "0.2", "0.3", "0.5"],
    _S + ["--blur_psf", PSF, "--degrade_tables", "device"],
)] + [("evaluate", a) for a in (
    ["--scale", "X1", "--ckpt", "F", "--arch", "swinir", "--channels", "1"],
    _E + ["--task", "dn", "--arch", "hat"],
    ["--scale", "X1", "--ckpt", "F", "--arch", "swinir", "--task", "car", "--bench_metric", "y", "--channels", "1"],
    ["--scale", "X1", "--ckpt", "F", "--arch", "swinir", "--task", "dn", "--dn_sigma", "25", "--jpeg_quality", "40", "--crop_border", "-1"],
    ["--scale", "X1", "--ckpt", "F", "--arch", "swinir", "--task", "car", "--jpeg_quality", "400", "--crop_border", "2"],
    ["--scale", "X2", "--ckpt", "F", "--crop_border", "-1", "--synth_lr"],
    ["--scale", "X2", "--ckpt", "F", "--synth_lr", "--degrade", "second_order", "--synth_lr_bits", "0"],
    _ES + ["--degrade", "second_order", "--synth_lr_bits", "0", "--blur_sigma", "3", "3"],
    _E + ["--degrade", "blind", "--gt_usm"],
    _ES + ["--degrade", "blind", "--blur_sigma", "3", "3", "--gt_usm"],
    _ES + ["--gt_usm", "--usm_weight", "0.5", "--blur_theta", "30"],
    _ES + ["--degrade", "second_order", "--usm_weight", "0.5", "--blur_theta", "30", "--blur_psf", "F.npy"],
    _ES + ["--degrade", "second_order", "--gt_usm", "--usm_radius", "99", "--blur_theta", "nan"],
    _ES + ["--blur_theta", "30", "--jpeg_subsample", "420"],
    _ES + ["--jpeg_subsample", "420", "--tile", "-1"],
    _E + ["--jpeg_quality", "101", "--synth_lr_bits", "0"],
    _ES + ["--jpeg_quality", "101", "--synth_lr_bits", "0"],
    _ES + ["--jpeg_quality", "101", "--tile", "-1"],
    _E + ["--tile", "8", "--tile_overlap", "8", "--window_size", "9"],
    _ES + ["--degrade", "blind", "--blur_psf", PSF],
    _ES + ["--degrade", "second_order", "--blur_psf", PSF, "--gt_usm", "--jpeg_quality", "50"],
    _ES + ["--blur_psf", PSF],
)]


def own_psf_bytes() -> bytes:
    import numpy as np

    from tpu_superresolution_amd import blur_kernels as bk
    buf = io.BytesIO()
    np.save(buf, np.stack([bk.gaussian(5, 1.0, 2.0, 0.3), bk.gaussian(5, 0.7, 0.7)]))
    return buf.getvalue()


def modules():
    from tpu_superresolution_amd import evaluate, finetune_swinir
    return {"finetune": finetune_swinir, "evaluate": evaluate}


def write_files(files: dict, root: str) -> None:
    for name, b64 in files.items():
        with open(os.path.join(root, name), "wb") as f:
            f.write(base64.b64decode(b64))


def _plain(v, root):
    """JSON form of a recorded value; the directory of the replayed files reads '@F/' again."""
    import numpy as np
    if isinstance(v, np.ndarray):
        r = np.round(v.astype(np.float64), 6) + 0.0
        return f"ndarray{v.shape} {v.dtype} sum={float(r.sum()):.5f} sha1={hashlib.sha1(r.tobytes()).hexdigest()[:12]}"
    if isinstance(v, str):
        return v.replace(root + os.sep, "@F/")
    if isinstance(v, dict):
        return {k: _plain(x, root) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x, root) for x in v]
    return v


def _spec_repr(v, root):
    import numpy as np
    return _plain(v if isinstance(v, np.ndarray) else repr(v), root)


def eval_inline_specs(args):
    """The FixedDegrade and the SecondOrderSpec of an evaluation run, by the rule evaluate.main had inline when the record was made."""
    from tpu_superresolution_amd.sr_datasets import FixedDegrade, SecondOrderSpec
    fixed = second = None
    if args.synth_lr and args.degrade in ("blind", "second_order"):
        fixed = FixedDegrade(tuple(args.blur_sigma), (args.noise_sigma / 255.0, args.noise_gain))
    if args.synth_lr and args.degrade == "second_order":
        second = SecondOrderSpec() if args.jpeg_quality is None else SecondOrderSpec(jpeg_quality=(args.jpeg_quality,) * 2)
    return {"degrade": fixed, "second_order": second}


def describe(which: str, argv: list, root: str) -> dict:
    """What parser `which` makes of argv, with the '@F/' files under root: the record's entry for that line."""
    mod = modules()[which]
    real = [a.replace("@F/", root + os.sep) if isinstance(a, str) else a for a in argv]
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            args = mod.parse_args(real)
    except SystemExit as e:
        text = err.getvalue()
        return {"parser": which, "argv": argv, "ok": False, "code": e.code, "error": _plain(text[text.index("error: ") + 7:].rstrip("\n"), root)}
    # 'args' holds what differs from the defaults that "shape" records: vars(args) is those defaults updated with it
    d = defaults(which)
    out = {"parser": which, "argv": argv, "ok": True, "args": _plain({k: v for k, v in vars(args).items() if k not in d or v != d[k]}, root)}
    if which == "finetune":
        out["saved"] = _plain(mod.saved_args(args), root)
        out["specs"] = {n: _spec_repr(getattr(mod, n)(args), root) for n in TRAIN_SPECS}
    else:
        out["specs"] = {n: _spec_repr(getattr(mod, n)(args), root) for n in EVAL_SPECS}
        out["specs"].update({n: _spec_repr(v, root) for n, v in eval_inline_specs(args).items()})
    return out


def parser_shape(which: str) -> list:
    """Every action of the parser that parse_args builds: option strings, nargs, type name, choices, default, metavar, required, class."""
    class _Stop(Exception):
        pass

    seen = []

    def grab(self, argv=None, namespace=None):
        seen.append(self)
        raise _Stop

    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = grab
    try:
        modules()[which].parse_args([])
    except _Stop:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    return [{"options": list(a.option_strings), "dest": a.dest, "nargs": a.nargs, "type": getattr(a.type, "__name__", None),
             "choices": None if a.choices is None else list(a.choices), "default": a.default, "required": a.required,
             "metavar": list(a.metavar) if isinstance(a.metavar, tuple) else a.metavar, "action": type(a).__name__}
            for a in seen[0]._actions]


def defaults(which: str) -> dict:
    return {a["dest"]: a["default"] for a in parser_shape(which) if a["action"] != "_HelpAction"}


def harvest():
    """-> (lines, files): every (parser, argv) the HARVEST tests pass to a parse_args, in first-seen order, and the files they name."""
    import pytest
    lines, files, mods = [], {}, modules()

    def wrap(which, orig):
        def recording(argv=None):
            rec = []
            for a in argv:
                if isinstance(a, str) and os.path.isabs(a):
                    if os.path.isfile(a) and a.endswith(".npy"):          # what a parser opens: the tables of --blur_psf
                        data = open(a, "rb").read()
                        name = f"{hashlib.sha1(data).hexdigest()[:8]}_{os.path.basename(a)}"
                        files[name] = base64.b64encode(data).decode()
                    else:
                        name = "path_" + os.path.basename(a)
                    a = "@F/" + name
                rec.append(a)
            if (which, rec) not in lines:
                lines.append((which, rec))
            return orig(argv)
        return recording

    origs = {w: m.parse_args for w, m in mods.items()}
    for w, m in mods.items():
        m.parse_args = wrap(w, origs[w])
    try:
        code = pytest.main(["-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider", *[os.path.join(ROOT, "tests", n + ".py") for n in HARVEST]])
    finally:
        for w, m in mods.items():
            m.parse_args = origs[w]
    if code != 0:
        raise SystemExit(f"the harvested tests did not pass (pytest exit {code}): no record written")
    return lines, files


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help="record this checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "cli_corpus.json"))
    args = ap.parse_args(argv)
    if not args.write:
        ap.error("nothing to do without --write (tests/test_cli_corpus.py does the comparing)")
    import subprocess
    import tempfile
    lines, files = harvest()
    lines += [ln for ln in EXTRA if ln not in lines]
    files[PSF[3:]] = base64.b64encode(own_psf_bytes()).decode()
    with tempfile.TemporaryDirectory() as root:
        write_files(files, root)
        entries = [describe(w, a, root) for w, a in lines]
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True).stdout.strip()
    doc = {"recorded_at": commit + (" (modified)" if dirty else ""), "files": files, "shape": {w: parser_shape(w) for w in ("finetune", "evaluate")},
           "lines": entries}
    with open(args.out, "w") as f:
        body = {k: json.dumps(v, sort_keys=True) for k, v in doc.items() if k != "lines"}          # one line per entry: readable diffs
        body["lines"] = "[\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in entries) + "\n]"
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {v}" for k, v in sorted(body.items())) + "\n}\n")
    print(f"{len(entries)} lines ({sum(e['ok'] for e in entries)} accepted, {sum(not e['ok'] for e in entries)} refused), "
          f"{len(files)} files -> {args.out} at {doc['recorded_at']}")


if __name__ == "__main__":
    main()
