"""Record tests/golden/g20_head_controls.npz: the output digests of the one-step head's control cases (16 and 12 head channels).

TEST INFRASTRUCTURE, run on the GPU with the library of the commit BEFORE the head was widened (a build of that commit's csrc, named by
SRK_LIB_PATH):

    SRK_LIB_PATH=/path/to/parent/libsrk.so python tools/record_head_controls.py [--out FILE]

tests/test_gpu_wide_head.py holds the current library to these digests: nothing changes for upscale^2 * in_chans <= 16.  The cases,
weights and inputs are those of tests/wide_head_case.py (seeded; nothing but the digests is stored).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import wide_head_case as W  # noqa: E402
from tpu_superresolution_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g20_head_controls.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the digests are those of the device's outputs (no CPU fallback)")
    print("library:", _lib.LIB_PATH)
    arrays = {}
    for s, c in W.CONTROLS:
        for hw in W.SIZES:
            m = W.model(s, c)
            with torch.no_grad():
                a, b = m(W.image(c, hw).cuda()), m(W.image(c, hw).cuda())
            assert torch.equal(a, b), "two runs differ: the digest would pin noise"
            arrays[W.key(s, c, hw)] = np.array(W.digest(a))
            print(W.key(s, c, hw), arrays[W.key(s, c, hw)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **arrays)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
