"""fp64 restatement of the frequency loss (include/srk.h: srk_fft_loss_fwd_bwd) with explicit DFT matrices and a mask for
the structurally real bins; tests/test_fft_loss_ref.py pins it to fp64 autograd of the torch.fft.rfft2 expression, the GPU tests
compare the kernels against it.

    d = pred - target,  D = rfft2(d) unnormalised,  Wh = W // 2 + 1,  s = 1 | 1 / sqrt(H W) (ortho),  N = 2 B C H Wh
    L = (s / N) sum |Re D| + |Im D|
    dL/dpred[y, x] = (s / N) Re sum_{u < H, v < Wh} G[u, v] exp(+2 pi i (u y / H + v x / W)),  G = sign(Re D) + i sign(Im D)

`flaw` selects one of the mistakes the pin must catch (negative controls); None is the definition."""
import math

import torch

NORMS = ("backward", "ortho")
FLAWS = ("hermitian", "n_without_2", "n_full_width", "ortho_grad_unscaled", "structural_sign")


def dft_cos_sin(n: int, cols: int):
    """cos, sin of 2 pi (j k mod n) / n as [n][cols] fp64 by the reduced index"""
    j = torch.arange(n, dtype=torch.int64)[:, None]
    k = torch.arange(cols, dtype=torch.int64)[None, :]
    idx = (j * k) % n
    ang = 2.0 * math.pi * idx.to(torch.float64) / n
    c, s = torch.cos(ang), torch.sin(ang)
    zero, one = torch.zeros_like(c), torch.ones_like(c)          # quarter turns exactly, as the device tables have them
    c = torch.where((4 * idx == n) | (4 * idx == 3 * n), zero, torch.where(2 * idx == n, -one, c))
    s = torch.where((idx == 0) | (2 * idx == n), zero, torch.where(4 * idx == n, one, torch.where(4 * idx == 3 * n, -one, s)))
    return c, s


def structural_mask(H: int, W: int) -> torch.Tensor:
    """[H][Wh] bool: the self-conjugate bins u in {0, H/2}, v in {0, W/2} (halves of even extents only), where Im D is zero by structure"""
    Wh = W // 2 + 1
    u = torch.arange(H)[:, None]
    v = torch.arange(Wh)[None, :]
    return ((u == 0) | (2 * u == H)) & ((v == 0) | (2 * v == W))


def spectrum(d: torch.Tensor):
    """-> (Re D, Im D) fp64 [..., H, Wh] of the half spectrum, Im forced to 0 at the structural bins"""
    d = d.double()
    H, W = d.shape[-2:]
    Wh = W // 2 + 1
    cw, sw = dft_cos_sin(W, Wh)
    ch, sh = dft_cos_sin(H, H)
    t_re, t_im = d @ cw, -(d @ sw)
    d_re = ch @ t_re + sh @ t_im
    d_im = ch @ t_im - sh @ t_re
    return d_re, torch.where(structural_mask(H, W), torch.zeros_like(d_im), d_im)


def adjoint(g_re: torch.Tensor, g_im: torch.Tensor, W: int) -> torch.Tensor:
    """Re sum_{u, v < Wh} (g_re + i g_im)[u, v] exp(+2 pi i (u y / H + v x / W)) -> [..., H, W]: the adjoint of `spectrum`"""
    H, Wh = g_re.shape[-2:]
    cw, sw = dft_cos_sin(W, Wh)
    ch, sh = dft_cos_sin(H, H)
    p_re = ch @ g_re - sh @ g_im
    p_im = ch @ g_im + sh @ g_re
    return p_re @ cw.T - p_im @ sw.T


def fft_loss_ref(pred: torch.Tensor, target: torch.Tensor, norm: str = "backward", flaw=None):
    """-> (L, dL/dpred) fp64"""
    assert norm in NORMS and (flaw is None or flaw in FLAWS)
    B, C, H, W = pred.shape
    Wh = W // 2 + 1
    d_re, d_im = spectrum(pred.double() - target.double())
    s = 1.0 / math.sqrt(H * W) if norm == "ortho" else 1.0
    n = 2.0 * B * C * H * Wh
    if flaw == "n_without_2":
        n = 1.0 * B * C * H * Wh
    if flaw == "n_full_width":
        n = 2.0 * B * C * H * W
    loss = (s / n) * (d_re.abs().sum() + d_im.abs().sum())
    g_re, g_im = torch.sign(d_re), torch.sign(d_im)
    if flaw == "structural_sign":
        g_im = torch.where(structural_mask(H, W), torch.ones_like(g_im), g_im)
    if flaw == "hermitian":          # the irfft2-style operator: interior columns counted twice
        v = torch.arange(Wh)
        twice = torch.where((v == 0) | (2 * v == W), 1.0, 2.0).to(torch.float64)
        g_re, g_im = g_re * twice, g_im * twice
    grad = adjoint(g_re, g_im, W) * ((1.0 if flaw == "ortho_grad_unscaled" else s) / n)
    return loss, grad


def fft_loss_autograd(pred: torch.Tensor, target: torch.Tensor, norm: str = "backward"):
    """fp64 autograd of F.l1_loss(stack([rfft2(pred).real, rfft2(pred).imag], -1), the same of target) -> (L, dL/dpred, rfft2(pred - target))"""
    leaf = pred.double().clone().requires_grad_(True)
    fp, ft = torch.fft.rfft2(leaf, norm=norm), torch.fft.rfft2(target.double(), norm=norm)
    loss = torch.nn.functional.l1_loss(torch.stack([fp.real, fp.imag], -1), torch.stack([ft.real, ft.imag], -1))
    (g,) = torch.autograd.grad(loss, leaf)
    return loss.detach(), g, (fp - ft).detach()


def random_inputs(shape, seed: int):
    """target ~ U[0, 1), pred = target + 0.05 randn, fp32"""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(shape, generator=g, dtype=torch.float32)
    pred = target + 0.05 * torch.randn(shape, generator=g, dtype=torch.float32)
    return pred, target


def designed_inputs(shape, seed: int):
    """Inputs whose difference has a half spectrum with every Re, Im = +-U[1, 2): the columns v = 0 and v = W / 2 are made
    conjugate-symmetric in u (so that the spectrum is one of a real image), d = irfft2(D) in fp64, pred = target + d in fp32."""
    B, C, H, W = shape
    Wh = W // 2 + 1
    g = torch.Generator().manual_seed(seed)

    def draw():
        mag = 1.0 + torch.rand((B, C, H, Wh), generator=g, dtype=torch.float64)
        sgn = torch.where(torch.rand((B, C, H, Wh), generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
        return mag * sgn

    re, im = draw(), draw()
    mirror = (-torch.arange(H)) % H
    for v in ([0] + ([W // 2] if W % 2 == 0 else [])):
        for u in range(H):
            m = int(mirror[u])
            if m == u:
                im[..., u, v] = 0.0
            elif m > u:
                re[..., m, v] = re[..., u, v]
                im[..., m, v] = -im[..., u, v]
    d = torch.fft.irfft2(torch.complex(re, im), s=(H, W))
    target = torch.rand(shape, generator=g, dtype=torch.float32)
    pred = (target.double() + d).float()
    return pred, target
