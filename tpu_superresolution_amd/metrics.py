"""Image-quality metrics used by the reference's scripts.

``batch_psnr``   train.py:46-56 / finetune_swinir.py:69-74   clamp to [0,1], 20 log10(max / sqrt(mse + 1e-8)), per image
``psnr``         evaluate.py:24-29                            no clamp, mse floored at 1e-10, mean over the batch (float)
``ssim``         ``pytorch_msssim.ssim`` (pin pytorch-msssim==1.0.0, sr_environment.yml:165; call sites train.py:169,
                 evaluate.py:127,195).  The package is not part of the reference tree and not installed here, so this is
                 a restatement of its published algorithm -- Wang et al. 2004 with an 11-tap Gaussian (sigma 1.5)
                 applied separably as a VALID (unpadded) depth-wise filter, K = (0.01, 0.03), per-channel map mean,
                 then mean over channels (and over the batch when size_average) -- **parity unpinned**: no
                 reference-produced fixture exists; tests check it against the closed form on cases with a known answer
                 (identical images -> 1, constant shift, scipy's gaussian_filter1d windows).
``bench_metrics`` nothing in the reference: PSNR / SSIM by the protocol of the SwinIR / HAT / DAT papers (8-bit, border-cropped, BT.601
                 luma or RGB, 0..255 scale, per image; include/srk.h) -> ``srk_bench_planes_f32`` / ``srk_bench_psnr`` and
                 ``srk_ssim`` on the planes; its SSIM shares the restatement above, parity with the third-party test scripts unpinned.

``niqe``         nothing in the reference: the no-reference score of the real-SR papers (BasicSR's calculate_niqe restated, **parity
                 unpinned**; niqe.py, include/srk.h) -> ``srk_niqe_*`` stages on the device, AGGD fit and distance in host fp64.

``psnrb``        nothing in the reference: PSNR-B of the JPEG-artifact tables (Yim & Bovik; SwinIR's calculate_psnrb restated, **parity
                 unpinned**; include/srk.h) on the planes of ``bench_metrics`` -> ``srk_psnrb`` (csrc/fullref.hip).
``ms_ssim``      nothing in the reference: ``pytorch_msssim.ms_ssim`` (Wang et al. 2003) restated, **parity unpinned**  ->
                 ``srk_msssim``: the level means on the device, the power product in host fp64; no gradient on the device path.

CPU tensors use the torch-operator forms below (evaluate.py / train.py run BASELINE cfg1 on the CPU).  fp32 GPU tensors go to
the libsrk kernels: ``psnr`` -> ``srk_eval_psnr``, ``batch_psnr`` -> ``srk_batch_psnr``, ``ssim`` (4-D,
H, W >= 11, default window) -> ``srk_ssim`` (csrc/metrics.hip, csrc/misc.hip): one fused pass, fixed-order sums, no per-pixel
intermediates in HBM.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .niqe import (load_niqe_params, niqe, niqe_distance, niqe_features, niqe_fit, niqe_moments,          # noqa: F401  no-reference
                   save_niqe_params)                                                                       # quality (niqe.py)


def _on_device(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def batch_psnr(pred: torch.Tensor, target: torch.Tensor, max_val: float = 1.0) -> torch.Tensor:
    if _on_device(pred, target) and pred.size(0) <= 1024:
        from . import ops
        return ops.batch_psnr(pred.detach(), target.detach(), max_val)
    pred, target = pred.clamp(0.0, 1.0), target.clamp(0.0, 1.0)
    mse = ((pred - target) ** 2).reshape(pred.size(0), -1).mean(dim=1)
    return 20.0 * torch.log10(max_val / torch.sqrt(mse + 1e-8))


def psnr(x: torch.Tensor, y: torch.Tensor, max_val: float = 1.0) -> float:
    if _on_device(x, y) and x.size(0) <= 1024:
        from . import ops
        return float(ops.eval_psnr(x.detach(), y.detach(), max_val)[1])
    mse = torch.mean((x - y) ** 2, dim=[1, 2, 3]).clamp(min=1e-10)
    return float((20.0 * torch.log10(max_val / torch.sqrt(mse))).mean())


def gaussian_window(size: int = 11, sigma: float = 1.5, dtype=torch.float32, device=None) -> torch.Tensor:
    coords = torch.arange(size, dtype=torch.float32, device=device) - size // 2
    g = torch.exp(-(coords ** 2) / (2.0 * sigma ** 2))
    return (g / g.sum()).to(dtype)


def _blur_valid(x: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    """Separable depth-wise VALID filtering of [B, C, H, W]; an axis shorter than the window is left unfiltered (the
    published implementation warns and skips it)."""
    C = x.shape[1]
    k = win.numel()
    if x.shape[2] >= k:
        x = F.conv2d(x, win.view(1, 1, k, 1).expand(C, 1, k, 1), groups=C)
    if x.shape[3] >= k:
        x = F.conv2d(x, win.view(1, 1, 1, k).expand(C, 1, 1, k), groups=C)
    return x


def _ssim_channel_means(X: torch.Tensor, Y: torch.Tensor, win: torch.Tensor, data_range: float, K):
    """-> (mean of the SSIM map, mean of its contrast-structure factor), each [B, C]."""
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = _blur_valid(X, win), _blur_valid(Y, win)
    s11 = _blur_valid(X * X, win) - mu1 * mu1
    s22 = _blur_valid(Y * Y, win) - mu2 * mu2
    s12 = _blur_valid(X * Y, win) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    smap = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
    return smap.flatten(2).mean(-1), cs.flatten(2).mean(-1)


def ssim_torch(X: torch.Tensor, Y: torch.Tensor, data_range: float = 255.0, size_average: bool = True, win_size: int = 11,
               win_sigma: float = 1.5, K=(0.01, 0.03), nonnegative_ssim: bool = False) -> torch.Tensor:
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if X.ndim != 4:
        raise ValueError(f"Input images should be 4-d tensors [B, C, H, W], but got {X.shape}")
    if win_size % 2 != 1:
        raise ValueError("Window size should be odd.")
    win = gaussian_window(win_size, win_sigma, X.dtype, X.device)
    per_channel, _ = _ssim_channel_means(X, Y, win, data_range, K)           # [B, C]
    if nonnegative_ssim:
        per_channel = torch.relu(per_channel)
    return per_channel.mean() if size_average else per_channel.mean(1)


class _SsimMean(torch.autograd.Function):
    """Batch-mean SSIM that carries a gradient for X (csrc/loss.hip: value and dS/dX from one fused kernel); none for Y."""

    @staticmethod
    def forward(ctx, X, Y, data_range):
        from . import ops
        mean, d_x, _ = ops.ssim_loss_fwd_bwd(X.contiguous(), Y.detach().contiguous(), data_range, alpha=-1.0)      # d_x = +dS/dX
        ctx.save_for_backward(d_x)
        return mean.reshape(())

    @staticmethod
    def backward(ctx, g):
        (d_x,) = ctx.saved_tensors
        return d_x * g, None, None


def ssim(X: torch.Tensor, Y: torch.Tensor, data_range: float = 255.0, size_average: bool = True, **kw) -> torch.Tensor:
    """``pytorch_msssim.ssim`` signature (data_range default 255, as published).  On the device path the batch mean
    (size_average=True) of an X that requires grad is differentiable in X (``1 - ssim(model(x), hr)`` trains); Y gets no gradient.
    The per-image form (size_average=False) of such an X goes through the torch operators."""
    if (_on_device(X, Y) and not kw and X.ndim == 4 and X.shape == Y.shape and X.shape[2] >= 11 and X.shape[3] >= 11 and X.size(0) <= 1024
            and X.size(0) * X.size(1) < 65536):
        from . import ops
        if torch.is_grad_enabled() and X.requires_grad:
            if size_average:
                return _SsimMean.apply(X, Y, float(data_range))
            return ssim_torch(X, Y, data_range=data_range, size_average=False)
        per, mean = ops.ssim(X.detach(), Y.detach(), data_range)
        return mean.reshape(()) if size_average else per
    return ssim_torch(X, Y, data_range=data_range, size_average=size_average, **kw)


# ---- benchmark-protocol PSNR / SSIM (include/srk.h) -------------------------------------------------------------------
def bench_planes_torch(x: torch.Tensor, crop_border: int, mode: str = "y") -> torch.Tensor:
    """The torch-operator form of srk_bench_planes_f32 for one tensor: fp32 [B, C, H, W] -> fp32 [B, Cm, Hc, Wc].  The clamp is by
    comparisons (torch.where), so a NaN stays; each fmaf of the luma chain is an fp64 multiply-add of fp32 operands -- exact there --
    rounded once to fp32, which is what a fused multiply-add returns."""
    from .ops import bench_plane_shape
    bench_plane_shape(x.shape, crop_border, mode)
    x = x.to(torch.float32)
    b = int(crop_border)
    x = x[:, :, b:x.shape[2] - b, b:x.shape[3] - b]
    c = torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))
    q = (c * 255.0).round()                                  # one fp32 multiply, round-half-to-even
    if mode == "rgb" or q.shape[1] == 1:
        return q.contiguous()
    k = [torch.tensor(v, dtype=torch.float32).double() for v in (65.481, 128.553, 24.966)]
    t = q[:, 0] * torch.tensor(65.481, dtype=torch.float32)
    t = (k[1] * q[:, 1].double() + t.double()).float()
    t = (k[2] * q[:, 2].double() + t.double()).float()
    return (16.0 + t / 255.0).unsqueeze(1).contiguous()


def bench_metrics(pred: torch.Tensor, target: torch.Tensor, crop_border: int, mode: str = "y", with_ssim: bool = True):
    """PSNR and SSIM as the SwinIR / HAT / DAT papers report them -> (psnr [B], ssim [B] or None), fp32, per image: both images
    clamped and rounded to 8 bits, `crop_border` pixels cropped on every side, the BT.601 luma of RGB images (mode 'y'; a
    single-channel image is its own luma) or every channel (mode 'rgb'), on the 0..255 scale; equal planes give +inf.  fp32 GPU
    tensors take the kernels (ops.bench_planes / ops.bench_psnr, then ops.ssim on the planes), anything else the torch operators.
    The SSIM is ``ssim`` above on the planes with data_range 255: restated, **parity with the third-party test scripts unpinned**."""
    from .ops import bench_plane_shape
    if pred.shape != target.shape:
        raise ValueError(f"bench metric: pred / target must have one shape (got {tuple(pred.shape)}, {tuple(target.shape)})")
    shape = bench_plane_shape(pred.shape, crop_border, mode)
    if with_ssim and min(shape[2:]) < 11:
        raise ValueError(f"bench metric: the SSIM window needs cropped planes of at least 11 x 11 (border {crop_border} leaves "
                         f"{shape[2]} x {shape[3]} of {pred.shape[2]} x {pred.shape[3]})")
    if _on_device(pred, target):
        from . import ops
        pp, pt, ws = ops.bench_planes(pred.detach(), target.detach(), crop_border, mode, planes=with_ssim)
        ps = ops.bench_psnr(ws, shape)[1]
        return ps, (ops.ssim(pp, pt, 255.0)[0] if with_ssim else None)
    pp, pt = bench_planes_torch(pred.detach(), crop_border, mode), bench_planes_torch(target.detach(), crop_border, mode)
    mse = ((pp - pt) ** 2).flatten(1).mean(1)
    ps = torch.where(mse == 0, torch.full_like(mse, float("inf")), 10.0 * torch.log10(65025.0 / mse))
    return ps, (ssim_torch(pp, pt, data_range=255.0, size_average=False) if with_ssim else None)


# ---- full-reference scores on the benchmark-protocol planes: PSNR-B, MS-SSIM (include/srk.h) ----------------------------
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def bench_planes_pair(pred: torch.Tensor, target: torch.Tensor, crop_border: int, mode: str = "y"):
    """The benchmark-protocol planes of both images -> (planes of pred, planes of target), fp32 [B, Cm, Hc, Wc]: the kernel for fp32
    GPU tensors, the torch operators for anything else."""
    if pred.shape != target.shape:
        raise ValueError(f"bench metric: pred / target must have one shape (got {tuple(pred.shape)}, {tuple(target.shape)})")
    if _on_device(pred, target):
        from . import ops
        pp, pt, _ = ops.bench_planes(pred.detach(), target.detach(), crop_border, mode)
        return pp, pt
    return bench_planes_torch(pred.detach(), crop_border, mode), bench_planes_torch(target.detach(), crop_border, mode)


def psnrb_planes_torch(pp: torch.Tensor, pt: torch.Tensor) -> torch.Tensor:
    """PSNR-B of planes [B, Cm, Hc, Wc] in fp64 torch operators -> fp64 [B] (the definition: include/srk.h)."""
    p, t = pp.double(), pt.double()
    Hc, Wc = p.shape[2:]
    mse = ((p - t) ** 2).flatten(2).mean(-1)                                  # [B, Cm]
    dh, dv = (p[..., :, :-1] - p[..., :, 1:]) ** 2, (p[..., :-1, :] - p[..., 1:, :]) ** 2
    bh, bv = torch.arange(Wc - 1) % 8 == 7, torch.arange(Hc - 1) % 8 == 7
    n_bh, n_bv = Hc * (Wc // 8 - 1), Wc * (Hc // 8 - 1)                      # the published counts
    n_nh, n_nv = Hc * (Wc - 1) - n_bh, Wc * (Hc - 1) - n_bv
    d_b = (dh[..., bh].sum((-1, -2)) + dv[..., bv, :].sum((-1, -2))) / (n_bh + n_bv)
    d_n = (dh[..., ~bh].sum((-1, -2)) + dv[..., ~bv, :].sum((-1, -2))) / (n_nh + n_nv)
    bef = torch.where(d_b > d_n, (3.0 / math.log2(min(Hc, Wc))) * (d_b - d_n), torch.zeros_like(d_b))
    den = mse + bef
    per = torch.where(den == 0, torch.full_like(den, float("inf")), 10.0 * torch.log10(65025.0 / den))
    return per.mean(1)


def psnrb(pred: torch.Tensor, target: torch.Tensor, crop_border: int, mode: str = "y") -> torch.Tensor:
    """PSNR-B (Yim & Bovik; SwinIR's calculate_psnrb restated, **parity unpinned**) of `pred`, the restored image, against `target`
    -> fp32 [B]: the benchmark-protocol planes of ``bench_metrics`` (8-bit, `crop_border` cropped, BT.601 luma or every channel), then
    PSNR with the blocking-effect factor of pred's 8 x 8 grid added to the squared error.  The cropped planes must be at least
    16 x 16.  fp32 GPU tensors take the kernels (ops.bench_planes, ops.psnrb_planes), anything else the torch operators."""
    from .ops import bench_plane_shape
    if pred.shape != target.shape:
        raise ValueError(f"psnrb: pred / target must have one shape (got {tuple(pred.shape)}, {tuple(target.shape)})")
    shape = bench_plane_shape(pred.shape, crop_border, mode)
    if min(shape[2:]) < 16:
        raise ValueError(f"psnrb: the 8 x 8 block grid needs cropped planes of at least 16 x 16 (border {crop_border} leaves "
                         f"{shape[2]} x {shape[3]} of {pred.shape[2]} x {pred.shape[3]})")
    pp, pt = bench_planes_pair(pred, target, crop_border, mode)
    if pp.is_cuda:
        from . import ops
        return ops.psnrb_planes(pp, pt)[1]
    return psnrb_planes_torch(pp, pt).float()


def _ms_ssim_weights(weights):
    w = [float(v) for v in (MS_SSIM_WEIGHTS if weights is None else weights)]
    if not w:
        raise ValueError("ms_ssim: weights must hold at least one level")
    return w


def _ms_ssim_check(X, Y, levels: int, win_size: int = 11):
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if X.ndim != 4:
        raise ValueError(f"Input images should be 4-d tensors [B, C, H, W], but got {X.shape}")
    need = (win_size - 1) * 2 ** (levels - 1)
    if min(X.shape[2:]) <= need:
        raise ValueError(f"ms_ssim: {levels} levels need a smaller side above {need} (got {X.shape[2]} x {X.shape[3]})")


def ms_ssim_torch(X: torch.Tensor, Y: torch.Tensor, data_range: float = 255.0, size_average: bool = True, win_size: int = 11,
                  win_sigma: float = 1.5, weights=None, K=(0.01, 0.03)) -> torch.Tensor:
    """MS-SSIM in torch operators: ``ssim_torch``'s map means per level, ``F.avg_pool2d`` (kernel 2, padding = extent % 2) between."""
    w = _ms_ssim_weights(weights)
    if win_size % 2 != 1:
        raise ValueError("Window size should be odd.")
    _ms_ssim_check(X, Y, len(w), win_size)
    win = gaussian_window(win_size, win_sigma, X.dtype, X.device)
    vals = []
    for s in range(len(w)):
        S, CS = _ssim_channel_means(X, Y, win, data_range, K)
        vals.append(torch.relu(CS if s < len(w) - 1 else S))
        if s < len(w) - 1:
            pad = [n % 2 for n in X.shape[2:]]
            X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    per_channel = torch.prod(torch.stack(vals) ** torch.tensor(w, dtype=X.dtype, device=X.device).view(-1, 1, 1), dim=0)       # [B, C]
    return per_channel.mean() if size_average else per_channel.mean(1)


def ms_ssim(X: torch.Tensor, Y: torch.Tensor, data_range: float = 255.0, size_average: bool = True, weights=None, **kw) -> torch.Tensor:
    """``pytorch_msssim.ms_ssim`` signature (Wang et al. 2003; restated, **parity unpinned**): per channel the product over the levels of
    max(CS_s, 0)^w_s -- max(S, 0)^w at the coarsest -- per image the mean over channels, and over the batch when size_average.  The
    smaller side must exceed 10 * 2^(levels - 1): 160 for the default five levels.  fp32 GPU tensors with the default window and K and up
    to five levels take ``srk_msssim`` (ops.msssim_means) and one download of the level means; the product is formed in host fp64.
    Anything else -- and an X that requires grad: the device path carries no gradient -- takes ``ms_ssim_torch``."""
    w = _ms_ssim_weights(weights)
    if (_on_device(X, Y) and not kw and len(w) <= 5 and X.ndim == 4 and X.shape == Y.shape and X.size(0) <= 1024
            and X.size(0) * X.size(1) < 65536 and not (torch.is_grad_enabled() and X.requires_grad)):
        from . import ops
        _ms_ssim_check(X, Y, len(w))
        m = ops.msssim_means(X.detach(), Y.detach(), len(w), data_range).double().cpu().clamp(min=0.0)            # [L, B, C, 2] = (S, CS)
        vals = torch.cat([m[:-1, :, :, 1], m[-1:, :, :, 0]])
        per = torch.prod(vals ** torch.tensor(w, dtype=torch.float64).view(-1, 1, 1), dim=0).mean(1).float().to(X.device)
        return per.mean() if size_average else per
    return ms_ssim_torch(X, Y, data_range=data_range, size_average=size_average, weights=weights, **kw)
