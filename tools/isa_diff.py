#!/usr/bin/env python
"""Device-code diff of two source trees: is a refactor neutral for the kernels?

    python tools/isa_diff.py PARENT_TREE BRANCH_TREE [--out report.json]

For every entry of build.SOURCES, in both trees, hipcc compiles the device side to assembly (build.FLAGS plus
--cuda-device-only -S; no GPU needed).  Lines with __hip_cuid_ (a hash of the source path) are dropped.  The report has, per
file (one that only the branch has is listed as new), the number of differing lines and, per kernel, .vgpr_count, .sgpr_count, LDS bytes, ScratchSize and Occupancy as the
assembly's own metadata states them.  Exit status 1 when anything differs.
"""
from __future__ import annotations

import argparse
import difflib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "tpu_superresolution_amd"


def load_build(root: str):
    spec = importlib.util.spec_from_file_location("_srk_build", os.path.join(root, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(build, root: str, src: str, out: str) -> list[str]:
    if not os.path.exists(os.path.join(root, PKG, "csrc", src)):          # a source the other tree does not have: reported as new
        return []
    cmd = [build._hipcc(), *build.FLAGS, "--cuda-device-only", "-S", os.path.join(root, PKG, "csrc", src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src} of {root}:\n{r.stderr}")
    with open(out) as f:
        return [ln.rstrip("\n") for ln in f if "__hip_cuid_" not in ln]


def kernel_stats(lines: list[str]) -> dict[str, dict[str, int]]:
    """{kernel: {vgpr_count, sgpr_count, lds, ScratchSize, Occupancy}} from the metadata note and the '; Kernel info' comments."""
    stats: dict[str, dict[str, int]] = {}
    # the comment block after a function belongs to the symbol of the .size line in front of it
    cur = None
    for ln in lines:
        m = re.match(r"\s*\.size\s+([^,\s]+),", ln)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r";\s*(ScratchSize|Occupancy):\s*(\d+)", ln)
        if m and cur:
            stats.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    # amdhsa.kernels metadata: one YAML item per kernel, .name among its keys
    keys = {".vgpr_count": "vgpr_count", ".sgpr_count": "sgpr_count", ".group_segment_fixed_size": "lds"}
    item: dict[str, int] = {}
    name = None
    kernels = set()

    def flush():
        if name:
            stats.setdefault(name, {}).update(item)
            kernels.add(name)

    in_meta = False
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            in_meta = True
            continue
        if not in_meta:
            continue
        if ln.startswith("amdhsa.") or ln.startswith("..."):
            break
        if re.match(r"\s+- \.", ln):            # first key of the next kernel's item (argument items are indented deeper, under .args)
            if len(ln) - len(ln.lstrip()) == 2:
                flush()
                item, name = {}, None
        m = re.match(r"\s+(?:- )?(\.[a-z_]+):\s*(\S+)", ln)
        if m and len(ln) - len(ln.lstrip()) <= 4:
            if m.group(1) == ".name":
                name = m.group(2)
            elif m.group(1) in keys:
                item[keys[m.group(1)]] = int(m.group(2))
    flush()
    return {k: v for k, v in stats.items() if k in kernels}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--out", help="write the JSON report here")
    ap.add_argument("--jobs", type=int, default=16)
    args = ap.parse_args()
    roots = [os.path.abspath(args.parent), os.path.abspath(args.branch)]
    builds = [load_build(r) for r in roots]
    sources = builds[1].SOURCES
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=max(1, min(16, args.jobs))) as ex:
        futs = {(s, i): ex.submit(assemble, builds[i], roots[i], s, os.path.join(tmp, f"{i}_{s}.s")) for s in sources for i in (0, 1)}
        asm = {k: f.result() for k, f in futs.items()}
    report = {"flags": builds[1].FLAGS + ["--cuda-device-only", "-S"], "files": {}, "kernels": {}}
    bad = 0
    for s in sources:
        a, b = asm[(s, 0)], asm[(s, 1)]
        ka, kb = kernel_stats(a), kernel_stats(b)
        if not a:          # new in the branch: nothing to compare with, and no difference to report
            report["files"][s] = {"lines": len(b), "new": True, "kernels": len(kb)}
            report["kernels"][s] = {k: kb[k] for k in sorted(kb)}
            print(f"{s:24s}    new in the branch, {len(kb):3d} kernels")
            continue
        ndiff = 0 if a == b else sum(1 for d in difflib.ndiff(a, b) if d[:2] in ("- ", "+ "))
        report["files"][s] = {"lines": len(b), "differing_lines": ndiff, "kernels": len(kb), "kernel_stats_equal": ka == kb}
        report["kernels"][s] = {k: ({"parent": ka.get(k), "branch": kb.get(k)} if ka.get(k) != kb.get(k) else kb[k])
                                for k in sorted(set(ka) | set(kb))}
        bad += ndiff > 0 or ka != kb
        print(f"{s:24s} {ndiff:6d} differing lines, {len(kb):3d} kernels, stats {'equal' if ka == kb else 'DIFFER'}")
    report["summary"] = {"files": len(sources), "files_that_differ": bad, "kernels": sum(f["kernels"] for f in report["files"].values())}
    print(json.dumps(report["summary"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
