import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


class _JoinedGolden(dict):
    """The arrays of a golden vector stored in parts (oracle/make_golden.py::save keeps every file under 1 MiB), read like an npz."""

    @property
    def files(self):
        return list(self)


def load_golden(name):
    path = os.path.join(GOLDEN, name + ".npz")
    parts = glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz"))
    if os.path.exists(path) or not parts:
        return np.load(path, allow_pickle=False)
    out = _JoinedGolden()
    for part in sorted(parts, key=lambda p: int(p[:-len(".npz")].rsplit(".part", 1)[1])):
        with np.load(part, allow_pickle=False) as z:
            out.update((k, z[k]) for k in z.files)
    return out


@pytest.fixture(scope="session")
def golden():
    return load_golden


def sub_state_dict(npz, prefix):
    """Arrays stored as '<prefix>sd.<key>' -> {key: tensor}."""
    import torch
    out = {}
    for k in npz.files:
        if k.startswith(prefix):
            out[k[len(prefix):]] = torch.from_numpy(npz[k])
    return out
