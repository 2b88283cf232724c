"""srk_psnrb / srk_msssim without a GPU: every refusal of the two entries and the zero returns of their workspace functions (include/srk.h
"Full-reference scores"; the addresses are dummies that are never dereferenced, every call differs from a valid one in exactly the argument
under test), and the CPU forms of metrics.psnrb / metrics.ms_ssim against the fp64 restatement of tests/fullref_ref.py."""
import numpy as np
import pytest
import torch

import fullref_ref as R

E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3
P, Q, WS, OUT = 1 << 20, 1 << 28, 1 << 30, 1 << 32          # far apart: nothing overlaps unless a test says so


@pytest.fixture(scope="module")
def lib():
    from tpu_superresolution_amd import build
    build.build(verbose=False)
    from tpu_superresolution_amd import _lib
    return _lib


def _sweep(h, fn, base, changes):
    """The valid call itself needs a GPU and is not made; each change must be refused on the host with its code and a message."""
    for name, bad, code in changes:
        assert name in base, name
        args = [bad if k == name else v for k, v in base.items()]
        rc = fn(*args, None)
        assert rc == code, (fn.__name__, name, bad, rc, code, h.srk_last_error())
        assert h.srk_last_error(), "no message"


def test_psnrb_refuses_bad_arguments_without_a_gpu(lib):
    h = lib.lib()
    base = dict(pred=P, target=Q, ws=WS, B=2, Cm=3, Hc=24, Wc=40, sums=OUT, psnrb=OUT + 4096)
    changes = [("pred", None, E_NULL), ("target", None, E_NULL), ("ws", None, E_NULL),
               ("B", 0, E_SHAPE), ("B", 1025, E_SHAPE), ("Cm", 0, E_SHAPE), ("Cm", 65536 // 2, E_SHAPE), ("Hc", 0, E_SHAPE), ("Wc", -16, E_SHAPE),
               ("Hc", 15, E_UNSUPPORTED), ("Wc", 15, E_UNSUPPORTED), ("Hc", 1, E_UNSUPPORTED),
               ("sums", P + 64, E_SHAPE), ("psnrb", Q, E_SHAPE), ("ws", P + 4, E_SHAPE), ("sums", Q + 4 * 2 * 3 * 24 * 40 - 4, E_SHAPE)]
    _sweep(h, h.srk_psnrb, base, changes)
    assert h.srk_psnrb(P, Q, WS, 2, 3, 24, 40, None, None, None) == E_NULL                  # no output at all
    assert h.srk_psnrb(P, Q, WS, 2, 3, 24, 15, OUT, None, None) == E_UNSUPPORTED
    assert b"block boundary" in h.srk_last_error()
    # the workspace: five floats per (plane, run of rows); 0 for everything the entry refuses
    assert h.srk_psnrb_workspace(2, 3, 24, 40) == 4 * 5 * 2 * 3 * 1
    assert h.srk_psnrb_workspace(1, 1, 65, 33) == 4 * 5 * 3                                # 32 + 32 + 1 rows
    assert h.srk_psnrb_workspace(1, 1, 1024, 1024) == 4 * 5 * 512                      # runs of 2 rows
    for bad in [(0, 1, 24, 40), (1025, 1, 24, 40), (2, 0, 24, 40), (2, 32768, 24, 40), (2, 3, 15, 40), (2, 3, 24, 15), (2, 3, 0, 40), (2, 3, 24, -1)]:
        assert h.srk_psnrb_workspace(*bad) == 0, bad


def test_msssim_refuses_bad_arguments_without_a_gpu(lib):
    h = lib.lib()
    base = dict(x=P, y=Q, ws=WS, B=2, C=3, H=176, W=163, levels=5, data_range=255.0, means=OUT)
    in_bytes = 4 * 2 * 3 * 176 * 163
    ws_bytes = h.srk_msssim_workspace(2, 3, 176, 163, 5)
    changes = [("x", None, E_NULL), ("y", None, E_NULL), ("ws", None, E_NULL), ("means", None, E_NULL),
               ("B", 0, E_SHAPE), ("B", 1025, E_SHAPE), ("C", 0, E_SHAPE), ("C", 32768, E_SHAPE), ("H", 0, E_SHAPE), ("W", -3, E_SHAPE),
               ("W", (1 << 20) + 1, E_SHAPE), ("levels", 0, E_SHAPE), ("levels", 6, E_SHAPE), ("data_range", 0.0, E_SHAPE),
               ("data_range", -1.0, E_SHAPE),
               ("H", 160, E_UNSUPPORTED), ("W", 160, E_UNSUPPORTED), ("H", 10, E_UNSUPPORTED), ("W", 1, E_UNSUPPORTED),
               ("means", P + 8, E_SHAPE), ("means", Q + in_bytes - 4, E_SHAPE), ("ws", Q + 16, E_SHAPE), ("ws", P - ws_bytes + 4, E_SHAPE),
               ("means", WS + 64, E_SHAPE)]
    _sweep(h, h.srk_msssim, base, changes)
    # the smaller side must exceed 10 * 2^(levels - 1)
    for levels, side in [(1, 10), (2, 20), (3, 40), (4, 80), (5, 160)]:
        assert h.srk_msssim(P, Q, WS, 1, 1, side, 400, levels, 255.0, OUT, None) == E_UNSUPPORTED, (levels, side)
        assert h.srk_msssim_workspace(1, 1, side, 400, levels) == 0 and h.srk_msssim_workspace(1, 1, side + 1, 400, levels) > 0
    # the workspace: both pooled pyramids, then two floats per tile and plane of every level; 0 for everything the entry refuses
    planes = 2 * 3
    dims = [(176, 163), (88, 82), (44, 41), (22, 21), (11, 11)]
    tiles = [((hh - 10 + 31) // 32) * ((ww - 10 + 31) // 32) for hh, ww in dims]
    assert ws_bytes == 4 * (2 * planes * sum(hh * ww for hh, ww in dims[1:]) + 2 * planes * sum(tiles))
    assert h.srk_msssim_workspace(2, 3, 11, 11, 1) == 4 * 2 * planes
    for bad in [(0, 3, 176, 163, 5), (1025, 1, 176, 163, 5), (2, 0, 176, 163, 5), (2, 32768, 176, 163, 5), (2, 3, 176, 163, 0), (2, 3, 176, 163, 6),
                (2, 3, 160, 163, 5), (2, 3, 176, 0, 5), (2, 3, 176, (1 << 20) + 1, 1)]:
        assert h.srk_msssim_workspace(*bad) == 0, bad


# ---- the CPU forms ---------------------------------------------------------------------------------------------------------------------
def _images(B, C, H, W, sigma, seed):
    x = np.stack([np.stack([R.pink_image(seed + 10 * b + c, H, W) for c in range(C)]) for b in range(B)])
    y = np.stack([np.stack([R.noised(x[b, c], sigma, b + c) for c in range(C)]) for b in range(B)])
    return x, y


@pytest.mark.parametrize("mode,C,border", [("y", 3, 0), ("rgb", 3, 3), ("y", 1, 2)])
def test_cpu_psnrb_equals_the_restatement_on_the_bench_planes(mode, C, border):
    from tpu_superresolution_amd import metrics as M
    x, y = _images(2, C, 40, 51, 12, 5)
    gt, sr = torch.from_numpy(x / 255.0).float(), torch.from_numpy(y / 255.0).float()
    got = M.psnrb(sr, gt, border, mode)
    assert got.dtype == torch.float32 and got.shape == (2,)
    pp, pt = M.bench_planes_pair(sr, gt, border, mode)
    want = R.psnrb(pp.numpy(), pt.numpy())
    np.testing.assert_allclose(got.double().numpy(), want, rtol=2e-7)
    assert not np.allclose(want, R.psnrb(pt.numpy(), pp.numpy()), rtol=1e-4)      # pred is the restored image: the order matters
    with pytest.raises(ValueError, match="at least 16 x 16"):
        M.psnrb(sr, gt, 13, mode)
    with pytest.raises(ValueError, match="one shape"):
        M.psnrb(sr, gt[:, :, :-1], border, mode)


def test_cpu_psnrb_special_values():
    from tpu_superresolution_amd import metrics as M
    yy, xx = np.meshgrid(np.arange(24), np.arange(32), indexing="ij")
    ramp = torch.from_numpy((20.0 + xx + yy) / 255.0).float()[None, None]
    assert float(M.psnrb(ramp, ramp, 0)[0]) == float("inf")
    bad = ramp.clone()
    bad[0, 0, 5, 7] = float("nan")
    assert torch.isnan(M.psnrb(bad, ramp, 0)[0]) and torch.isnan(M.psnrb(ramp, bad, 0)[0])


@pytest.mark.parametrize("C,H,W", [(1, 161, 161), (3, 176, 163)])
def test_cpu_ms_ssim_equals_the_restatement(C, H, W):
    from tpu_superresolution_amd import metrics as M
    x, y = _images(2, C, H, W, 12, 7)
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    want = R.msssim(x, y)                                        # fp64 taps; the package's window holds fp32 taps: some 4e-7
    np.testing.assert_allclose(M.ms_ssim(X, Y, size_average=False).numpy(), want, rtol=2e-6)
    assert float(M.ms_ssim(X, Y)) == pytest.approx(want.mean(), rel=2e-6)
    np.testing.assert_allclose(M.ms_ssim(X.float(), Y.float(), size_average=False).double().numpy(), want, rtol=5e-5)
    w3 = (0.2, 0.3, 0.5)
    np.testing.assert_allclose(M.ms_ssim(X[:, :, :60, :50], Y[:, :, :60, :50], size_average=False, weights=w3).numpy(),
                               R.msssim(x[:, :, :60, :50], y[:, :, :60, :50], weights=w3), rtol=2e-6)


def test_cpu_ms_ssim_refusals_and_gradient():
    from tpu_superresolution_amd import metrics as M
    x, y = _images(1, 1, 161, 161, 12, 9)
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    with pytest.raises(ValueError, match="smaller side above 160"):
        M.ms_ssim(X[:, :, :160], Y[:, :, :160])
    with pytest.raises(ValueError, match="same dimensions"):
        M.ms_ssim(X, Y[:, :, :-1])
    with pytest.raises(ValueError, match="4-d"):
        M.ms_ssim(X[0], Y[0])
    Xg = X.clone().requires_grad_(True)
    M.ms_ssim(Xg, Y).backward()                                  # the torch form carries the gradient
    assert Xg.grad is not None and bool(torch.isfinite(Xg.grad).all()) and float(Xg.grad.abs().max()) > 0
