"""Which C entries one call of the image ops and one `sample` of every device pool reach, in order: the launch sequences that
DESIGN.md states ("Module map of the data path") and that a change of the host code must keep.  Every `srk_*` attribute of the loaded
library is wrapped by a recorder that calls through; nothing is launched twice and nothing is compared numerically here (the bits are
pinned by the other GPU tests and by tools/pool_digest.py)."""
import importlib.util
import os
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AA, MODE = "srk_resize_aa_ragged_f32", "srk_resize_ragged_mode_f32"
NOISE, JPEG, JPEG_R, FILT, TABLES = "srk_noise_f32", "srk_jpeg_roundtrip_f32", "srk_jpeg_roundtrip_ragged_f32", "srk_filter2d_f32", "srk_kernel_tables_f32"
D4 = ["srk_dihedral_f32"] * 2          # the LR and the HR batch


def chain(r1=AA, r2=AA, r3=AA):
    """The eleven launches of ops.degrade_second_order's docstring."""
    return [FILT, r1, NOISE, JPEG_R, FILT, r2, NOISE, JPEG_R, r3, FILT, JPEG]


@pytest.fixture
def calls(monkeypatch):
    from tpu_superresolution_amd import _lib
    L, log = _lib.lib(), []

    def recorder(name, fn):
        def call(*a):
            log.append(name)
            return fn(*a)
        return call

    for name in _lib._SIGNATURES:
        monkeypatch.setattr(L, name, recorder(name, getattr(L, name)))
    return log


def _digest_tool():
    spec = importlib.util.spec_from_file_location("pool_digest", os.path.join(ROOT, "tools", "pool_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("modes,want", [(None, [AA]), ([0, 0, 0], [AA]), ([0, 1, 2], [MODE])], ids=["none", "zeros", "mixed"])
def test_resize_ragged_launch(calls, modes, want):
    from tpu_superresolution_amd import ops
    x = torch.rand(3, 3, 16, 20, device="cuda")
    ext = [(8, 10), (5, 7), (16, 20)]
    out = ops.resize_ragged(x, None, ext, modes)
    assert calls == want and tuple(out.shape) == (3, 3, 16, 20)


def test_resize_aa_ragged_is_the_same_launch(calls):
    from tpu_superresolution_amd import ops
    x = torch.rand(3, 3, 16, 20, device="cuda")
    ops.resize_aa_ragged(x, None, [(8, 10), (5, 7), (16, 20)])
    assert calls == [AA]


@pytest.mark.parametrize("quality,want", [(0, [NOISE]), ([0, 0], [NOISE]), ([0, 40], [NOISE, JPEG])], ids=["zero", "zeros", "one"])
def test_restore_degrade_skips_the_jpeg_launch_at_quality_zero(calls, quality, want):
    from tpu_superresolution_amd import ops
    x = torch.rand(2, 3, 24, 24, device="cuda")
    ops.restore_degrade(x, (0.05, 0.0), [1, 2], False, quality)
    assert calls == want


def test_restore_degrade_refuses_a_bool_quality(calls):
    from tpu_superresolution_amd import ops
    x = torch.rand(2, 3, 24, 24, device="cuda")
    with pytest.raises(ValueError, match="quality"):
        ops.restore_degrade(x, (0.05, 0.0), [1, 2], False, [0, False])
    assert JPEG not in calls


def _second_order(ops, bk, desc, modes=((0, 0, 0), (0, 0, 0))):
    T = bk.TableDesc if desc else bk
    return [ops.SecondOrder(T.gaussian(7, 1.5, 0.8, 0.3), 1.3, (0.03, 0.0), False, 60, T.sinc(2.0, 7), 0.7, (0.02, 0.01), True, 45, False,
                            T.sinc(2.5, 5), 11, modes[0]),
            ops.SecondOrder(T.sinc(1.8, 9), 0.6, (0.05, 0.02), True, 35, T.delta(), 1.1, (0.04, 0.0), False, 80, True, T.delta(), 12, modes[1])]


@pytest.mark.parametrize("desc,modes,want", [
    (False, ((0, 0, 0), (0, 0, 0)), chain()),
    (True, ((0, 0, 0), (0, 0, 0)), [TABLES] * 3 + chain()),
    (False, ((1, 2, 0), (0, 0, 0)), chain(MODE, MODE, AA)),
], ids=["arrays", "descriptors", "modes"])
def test_degrade_second_order_launches(calls, desc, modes, want):
    from tpu_superresolution_amd import blur_kernels as bk
    from tpu_superresolution_amd import ops
    x = torch.rand(2, 3, 24, 24, device="cuda")
    lr = ops.degrade_second_order(x, 2, _second_order(ops, bk, desc, modes))
    assert calls == want and tuple(lr.shape) == (2, 3, 12, 12)


POOL_LAUNCHES = {
    "pair": ["srk_paired_crop_u8"] + D4,
    "hr": ["srk_crop_degrade_u8"] + D4,
    "hr_degrade": ["srk_crop_degrade_blind_u8"] + D4,
    "hr_psf_host": ["srk_crop_degrade_psf_u8"] + D4,
    "hr_psf_device": [TABLES, "srk_crop_degrade_psf_u8"] + D4,
    "hr_jpeg": ["srk_crop_degrade_u8", JPEG] + D4,
    "hr2": ["srk_crop_u8", "srk_crop_u8"] + chain() + D4,
    "hr2_usm": ["srk_crop_u8", "srk_usm_sharpen_f32"] + chain() + D4,
    "restore": ["srk_crop_restore_u8"] + D4,
}


@pytest.mark.parametrize("name", list(POOL_LAUNCHES))
def test_one_sample_of_every_pool(calls, name):
    tool = _digest_tool()
    pool = tool.pool_configs()[name]()
    del calls[:]          # a pool's constructor launches nothing, but its uploads are not the subject
    random.seed(1)          # D4 codes (4, 7, 3) / (1, 7, 6): the dihedral branch is taken
    a, b = pool.sample(tool.INDICES)
    assert calls == POOL_LAUNCHES[name]
    P, S = tool.P, tool.S
    assert tuple(a.shape) == (3, 3, P, P) and tuple(b.shape) == ((3, 3, P, P) if name == "restore" else (3, 3, P * S, P * S))
