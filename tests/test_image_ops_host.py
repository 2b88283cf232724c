"""The host side of the image ops (image_ops.py, re-exported by ops.py): where the names live, what every batch op says to a CPU tensor,
and the helpers that never touch the device.  No GPU.  Except for the module map, every expectation here is the behaviour of the
commit before the ops moved into image_ops.py."""
import math
import struct

import numpy as np
import pytest
import torch

from tpu_superresolution_amd import blur_kernels as bk
from tpu_superresolution_amd import ops

SPEC_NAMES = ("FixedDegrade", "DegradeSpec", "JpegSpec", "PsfSpec", "UsmSpec", "SecondOrderSpec", "FixedRestore", "RestoreSpec", "PSF_MODES",
              "TABLE_MODES", "PSF_SIGMA_FLOOR", "SECOND_ORDER_VARIATES", "_check_range", "_check_prob3", "_check_factors")


def test_module_map():
    from tpu_superresolution_amd import _lib, degrade_specs, image_ops, sr_datasets
    assert len(image_ops.__all__) == len(set(image_ops.__all__)) >= 30
    for name in image_ops.__all__:
        assert getattr(ops, name) is getattr(image_ops, name), name
    assert ops._p is _lib._p is image_ops._p and ops._stream is _lib._stream is image_ops._stream
    for name in SPEC_NAMES:
        assert getattr(sr_datasets, name) is getattr(degrade_specs, name), name
    from tpu_superresolution_amd import evaluate, finetune_swinir
    args = evaluate.parse_args(["--scale", "X2", "--ckpt", "F", "--arch", "swinir", "--synth_lr", "--degrade", "second_order", "--gt_usm", "--usm_weight", "0.7"])
    assert evaluate.eval_usm(args) == finetune_swinir.usm_spec(args) == sr_datasets.UsmSpec(weight=0.7)


def test_names_resolve_through_ops_and_sr_datasets():
    from tpu_superresolution_amd import sr_datasets
    assert callable(ops._p) and callable(ops._stream) and ops._p(None) is None
    for name in SPEC_NAMES:
        assert hasattr(sr_datasets, name), name
    for name in ("resize_aa", "degrade_aa", "BLUR_SIGMA_MAX", "pack_degrade_params", "degrade_blind", "pack_psf", "DeviceTables", "kernel_tables",
                 "blur2d", "degrade_psf", "check_jpeg_quality", "jpeg_roundtrip", "pack_restore_params", "noise", "restore_degrade", "RaggedExt",
                 "pack_filter_tables", "filter2d", "resize_aa_ragged", "RESIZE_MODES", "resize_ragged", "usm_ks", "usm_taps", "usm_sharpen",
                 "jpeg_roundtrip_ragged", "SecondOrder", "second_order_sizes", "second_order_noise_ids", "degrade_second_order", "LUMA_COEF",
                 "to_gray"):
        assert hasattr(ops, name), name


# ---- what every public batch op says to a CPU fp32 [2,3,8,8] tensor ------------------------------------------------------------------
X = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(0))
G5 = bk.gaussian(5, 1.0, 0.7, 0.2)
NO_CPU = "GPU tensors only"          # ops._p: the op has no CUDA test of its own and the library's calling convention refuses the tensor


def _chain():
    return [ops.SecondOrder(G5, 1.0, (0.0, 0.0), False, 50, bk.delta(), 1.0, (0.0, 0.0), False, 50, False, bk.delta(), b) for b in range(2)]


CPU_ROWS = [
    ("resize_aa", lambda: ops.resize_aa(X, (4, 4)), RuntimeError, NO_CPU),
    ("degrade_aa", lambda: ops.degrade_aa(X, 2), RuntimeError, NO_CPU),
    ("degrade_blind", lambda: ops.degrade_blind(X, 2, (1.0, 1.0), (0.0, 0.0), [0, 1]), ValueError, "degrade_blind takes a"),
    ("blur2d", lambda: ops.blur2d(X, G5), ValueError, "blur2d takes a non-empty CUDA fp32"),
    ("degrade_psf", lambda: ops.degrade_psf(X, 2, G5), ValueError, "degrade_psf takes a"),
    ("jpeg_roundtrip", lambda: ops.jpeg_roundtrip(X, 50), ValueError, "jpeg_roundtrip takes a"),
    ("noise", lambda: ops.noise(X, (0.1, 0.0), [0, 1]), ValueError, "noise takes a"),
    ("restore_degrade", lambda: ops.restore_degrade(X, (0.1, 0.0), [0, 1]), ValueError, "noise takes a"),
    ("filter2d", lambda: ops.filter2d(X, G5), ValueError, "filter2d takes a non-empty CUDA fp32"),
    ("resize_aa_ragged", lambda: ops.resize_aa_ragged(X, None, [(4, 4), (3, 5)]), ValueError, "resize_aa_ragged takes a non-empty CUDA fp32"),
    ("resize_ragged", lambda: ops.resize_ragged(X, None, [(4, 4), (3, 5)], [1, 2]), ValueError, "resize_ragged takes a non-empty CUDA fp32"),
    ("resize_ragged-cubic", lambda: ops.resize_ragged(X, None, [(4, 4), (3, 5)], None), ValueError, "takes a non-empty CUDA fp32"),
    ("usm_sharpen", lambda: ops.usm_sharpen(X, 3), ValueError, "usm_sharpen takes a non-empty CUDA fp32"),
    ("jpeg_roundtrip_ragged", lambda: ops.jpeg_roundtrip_ragged(X, 50, [(8, 8), (5, 6)]), ValueError, "jpeg_roundtrip_ragged takes a"),
    ("degrade_second_order", lambda: ops.degrade_second_order(X, 2, _chain()), ValueError, "degrade_second_order takes a"),
]


@pytest.mark.parametrize("name,call,exc,text", CPU_ROWS, ids=[r[0] for r in CPU_ROWS])
def test_a_cpu_batch_is_refused(name, call, exc, text):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and text in str(e.value) and ("cpu" in str(e.value) or exc is RuntimeError)


def test_argument_checks_that_come_before_the_device():
    """Rows that fail on their arguments alone, whatever the tensor's device: the class and the op's name in the message."""
    for call, text in ((lambda: ops.resize_aa(X, (4, 4), quant_bits=4), "resize_aa: quant_bits"), (lambda: ops.resize_aa(X, 4), "resize_aa: size"),
                       (lambda: ops.resize_aa(X.double(), (4, 4)), "resize_aa takes"), (lambda: ops.resize_aa(X, (0, 4)), "resize_aa: every extent"),
                       (lambda: ops.resize_ragged(X, None, [(4, 4), (3, 5)], [0, 3]), "resize_ragged: a mode"),
                       (lambda: ops.resize_ragged(X, None, [(4, 4), (3, 5)], [0, True]), "resize_ragged: a mode"),
                       (lambda: ops.resize_ragged(X, None, [(4, 4), (3, 5)], [1]), "resize_ragged: one mode per sample"),
                       (lambda: ops.resize_ragged(X, None, [(4, 4), (3, 5)], 1), "resize_ragged: modes must be")):
        with pytest.raises(ValueError) as e:
            call()
        assert text in str(e.value)


# ---- helpers that never touch the device ---------------------------------------------------------------------------------------------
def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def test_pack_degrade_and_restore_params():
    assert ops.pack_degrade_params((1.0, 0.5), (0.1, 0.0), 7, True) == [_bits(1.0) | _bits(0.5) << 32, _bits(0.1), 7, 1]
    assert ops.pack_degrade_params((0.0, 2.5), (1.0, 1.0), (1 << 64) - 1, 0) == [_bits(2.5) << 32, _bits(1.0) | _bits(1.0) << 32, -1, 0]
    assert ops.pack_degrade_params((0, 0), (0, 0), -5, False)[2] == -5 and ops.pack_degrade_params((0, 0), (0, 0), 1 << 63, False)[2] == -(1 << 63)
    for bad, text in ((((2.6, 0.0), (0.0, 0.0), 0, False), "blur sigmas"), (((0.0, float("nan")), (0.0, 0.0), 0, False), "blur sigmas"),
                      (((0.0, 0.0), (1.5, 0.0), 0, False), "noise sigma and gain"), (((0.0, 0.0), (0.0, -0.1), 0, False), "noise sigma and gain"),
                      (((0.0, 0.0), (0.0, 0.0), 1 << 64, False), "64 bits")):
        with pytest.raises(ValueError, match=text):
            ops.pack_degrade_params(*bad)
    assert ops.pack_restore_params(40, (0.1, 0.0), 5, False) == [40, _bits(0.1), 5, 0]
    assert ops.pack_restore_params(0, (0.0, 0.0), 5, True) == [0, 0, 5, 1] and ops.pack_restore_params(0.0, (0.0, 0.0), 5, True)[0] == 0
    for q in (True, False, 101, -1, 50.5, "50", None):
        with pytest.raises(ValueError, match="jpeg quality"):
            ops.pack_restore_params(q, (0.0, 0.0), 0, False)
    with pytest.raises(ValueError, match="noise sigma and gain"):
        ops.pack_restore_params(50, (2.0, 0.0), 0, False)


def test_check_jpeg_quality():
    assert [ops.check_jpeg_quality(q) for q in (1, 100, 50.0, np.int64(7))] == [1, 100, 50, 7]
    assert all(type(ops.check_jpeg_quality(q)) is int for q in (50.0, np.int64(7)))
    for q in (True, False, 0, 101, 50.5, float("nan"), "50", None):
        with pytest.raises(ValueError, match="must be an integer in 1..100"):
            ops.check_jpeg_quality(q)
    with pytest.raises(ValueError, match="jpeg quality LO"):
        ops.check_jpeg_quality(0, "quality LO")


def test_usm_ks():
    assert [ops.usm_ks(r) for r in (1, 2, 3, 50, 51)] == [1, 3, 3, 51, 51]
    for r in (0, 52, True, 3.0, "3", None):
        with pytest.raises(ValueError, match="radius"):
            ops.usm_ks(r)


def test_second_order_sizes_and_noise_ids():
    p = _chain()[0]._replace(r1=1.5, r2=0.3, noise_id=5)
    assert ops.second_order_sizes(24, 20, 2, p) == ((36, 30), (4, 3), (12, 10))
    assert ops.second_order_sizes(24, 20, 4, p._replace(r1=0.15, r2=0.01)) == ((4, 3), (1, 1), (6, 5))
    assert ops.second_order_noise_ids(p) == (5, 5 ^ 0xFFFFFFFFFFFFFFFF)
    assert ops.second_order_noise_ids(p._replace(noise_id=-1)) == (0xFFFFFFFFFFFFFFFF, 0)
    assert p.modes == (0, 0, 0) and ops.RESIZE_MODES == ("cubic", "bilinear", "area")


def test_pack_psf_and_pack_filter_tables():
    a, b, s = bk.gaussian(3, 0.8, 0.5, 0.2), bk.plateau(7, 2.0, 1.0, 0.4, 1.2), bk.sinc(2.0, 5)
    # mixed sizes: padded, centred, to the largest; the 2-tuple and the 3-tuple
    tabs, ks = ops.pack_psf([a, b], 2)
    assert ks == 7 and tabs.dtype == np.float32 and np.array_equal(tabs[0], bk.pad_to(a, 7)) and np.array_equal(tabs[1], b)
    tabs, ks, own = ops.pack_filter_tables([a, s, b], 3)
    assert ks == 7 and own == [3, 5, 7] and tabs.dtype == np.float32 and tabs.shape == (3, 7, 7) and np.array_equal(tabs[1], bk.pad_to(s, 7))
    # one table for every sample; a tensor; an [n][ks][ks] array
    assert ops.pack_psf(a, 3)[0].shape == (3, 3, 3) and ops.pack_filter_tables(s, 2)[2] == [5, 5]
    assert np.array_equal(ops.pack_psf(torch.from_numpy(np.stack([b, b])), 2)[0], np.stack([b, b]))
    assert np.array_equal(ops.pack_filter_tables(torch.from_numpy(np.stack([s, s])), 2)[0], np.stack([s, s]))
    assert ops.pack_psf([a.tolist(), a.tolist()], 2)[1] == 3 and ops.pack_psf(a.astype(np.float64).tolist(), 2)[0].shape == (2, 3, 3)
    # the wrong count
    with pytest.raises(ValueError, match=r"psf: one table or one per sample \(B=3; got 2\)"):
        ops.pack_psf([a, b], 3)
    with pytest.raises(ValueError, match=r"filter tables: one table or one per sample \(B=3; got 2\)"):
        ops.pack_filter_tables([a, b], 3)
    # each its own rule: a sinc has negative taps
    with pytest.raises(ValueError, match=r"psf\[1\]: taps must be >= 0"):
        ops.pack_psf([a, s], 2)
    with pytest.raises(ValueError, match=r"table\[0\]: the taps must sum to 1"):
        ops.pack_filter_tables([2 * a, s], 2)
    with pytest.raises(ValueError, match="psf: a table is ks x ks"):
        ops.pack_psf(np.ones((2, 2), np.float32) / 4, 1)
    # checked=True: fp32 tables that blur_kernels made are only padded -- no rule is applied
    tabs, ks = ops.pack_psf([a, s, b], 3, checked=True)
    assert ks == 7 and tabs.dtype == np.float32 and all(np.array_equal(t, bk.pad_to(w, 7)) for t, w in zip(tabs, (a, s, b)))
    with pytest.raises(ValueError, match=r"psf: one table per sample \(B=2; got 3\)"):
        ops.pack_psf([a, s, b], 2, checked=True)


def test_to_gray():
    rng = np.random.RandomState(0)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        a = rng.randint(0, top + 1, (2, 5, 4, 3)).astype(dtype)
        a[0, 0, 0], a[0, 0, 1] = top, 0
        want = np.array([(4899 * int(r) + 9617 * int(g) + 1868 * int(b) + 8192) >> 14 for r, g, b in a.reshape(-1, 3)]).reshape(2, 5, 4)
        y = ops.to_gray(a)
        assert isinstance(y, np.ndarray) and y.dtype == dtype and y.shape == (2, 5, 4) and np.array_equal(y, want) and y[0, 0, 0] == top
        if dtype is np.uint8:
            t = ops.to_gray(torch.from_numpy(a))
            assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and np.array_equal(t.numpy(), want)
    assert ops.LUMA_COEF == (4899, 9617, 1868) and sum(ops.LUMA_COEF) == 16384
    with pytest.raises(ValueError, match="uint8 or uint16"):
        ops.to_gray(np.zeros((2, 2, 3), np.float32))
    with pytest.raises(ValueError, match=r"\[\.\.\., H, W, 3\]"):
        ops.to_gray(np.zeros((2, 2), np.uint8))


def test_bench_plane_shape_is_not_shadowed():
    assert ops.bench_plane_shape.__module__ == "tpu_superresolution_amd.ops"
    assert ops.bench_plane_shape((2, 3, 19, 23), 4, "y") == (2, 1, 11, 15) and ops.bench_plane_shape((2, 3, 19, 23), 0, "rgb") == (2, 3, 19, 23)
    with pytest.raises(ValueError, match="leaves nothing"):
        ops.bench_plane_shape((2, 3, 8, 8), 4, "y")
    assert math.isclose(ops.BLUR_SIGMA_MAX, 2.5)
