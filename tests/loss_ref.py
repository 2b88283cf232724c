"""fp64 restatement of the training objectives of csrc/loss.hip, for tests/test_loss_ref.py (pins it to torch) and tests/test_gpu_loss.py
(compares the kernels with it).

Pixel losses: mean |d|, mean d^2, mean sqrt(d^2 + eps^2), d = pred - target, and their gradients for pred.

SSIM term: S = the batch mean of metrics.ssim_torch (11-tap Gaussian, sigma 1.5, VALID separable filter, K = (0.01, 0.03)) and dS/dx in
closed form.  Per valid position p, with mu / sigma from the five filtered moments:

    B1 = mux^2 + muy^2 + C1      B2 = sx^2 + sy^2 + C2      L = (2 mux muy + C1) / B1      CS = (2 sxy + C2) / B2      S_p = L CS
    a_p = 2 CS (muy - L mux) / B1 - 2 L muy / B2 + 2 S_p mux / B2          b_p = -2 S_p / B2          c_p = 2 L / B2
    dS/dx_q = (1 / N) [ (G a)(q) + x_q (G b)(q) + y_q (G c)(q) ],      N = B C (H - 10) (W - 10)

G is the adjoint of the valid filter: the full (zero-extended) separable filtering with the symmetric window; a, b, c are zero outside
the valid domain [0, H - 10) x [0, W - 10).  The two ``wrong_*`` switches build the restatements that the negative controls must catch.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32
KINDS = ("l1", "mse", "charbonnier")


def pixel_loss_ref(pred, target, kind, eps=1e-3):
    """-> (loss, d loss / d pred) in fp64, written out (no autograd)."""
    d = pred.double() - target.double()
    n = d.numel()
    if kind == "l1":
        return d.abs().mean(), torch.sign(d) / n
    if kind == "mse":
        return (d * d).mean(), 2.0 * d / n
    if kind == "charbonnier":
        r = torch.sqrt(d * d + float(eps) ** 2)
        return r.mean(), d / r / n
    raise ValueError(kind)


def pixel_terms_abs_sum(pred, target, kind, eps=1e-3):
    """sum of the absolute terms of the loss sum (fp64): the S of the 2 K u S / n accumulation bound"""
    d = pred.double() - target.double()
    if kind == "l1":
        return float(d.abs().sum())
    if kind == "mse":
        return float((d * d).sum())
    return float(torch.sqrt(d * d + float(eps) ** 2).sum())


def window64():
    """the window of metrics.ssim_torch: evaluated in fp32 (as the published implementation and the kernels do), then widened"""
    from tpu_superresolution_amd.metrics import gaussian_window
    return gaussian_window(11, 1.5, torch.float64)


def _filter_valid(x, g):
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, 11, 1).expand(C, 1, 11, 1), groups=C)
    return F.conv2d(x, g.view(1, 1, 1, 11).expand(C, 1, 1, 11), groups=C)


def ssim_value_grad_ref(x, y, data_range=1.0, wrong_halo=False, wrong_count=False):
    """-> (S, dS/dx) in fp64 by the closed form.  wrong_halo: a, b, c are also evaluated on the zero-extended halo instead of being
    zero there; wrong_count: N misses the channel count."""
    x, y = x.double(), y.double()
    B, C, H, W = x.shape
    g = window64()
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    xi, yi = (F.pad(x, (10, 10, 10, 10)), F.pad(y, (10, 10, 10, 10))) if wrong_halo else (x, y)
    m1, m2 = _filter_valid(xi, g), _filter_valid(yi, g)
    s11 = _filter_valid(xi * xi, g) - m1 * m1
    s22 = _filter_valid(yi * yi, g) - m2 * m2
    s12 = _filter_valid(xi * yi, g) - m1 * m2
    B1, B2 = m1 * m1 + m2 * m2 + C1, s11 + s22 + C2
    L, CS = (2 * m1 * m2 + C1) / B1, (2 * s12 + C2) / B2
    Sp = L * CS
    a = 2 * CS * (m2 - L * m1) / B1 - 2 * L * m2 / B2 + 2 * Sp * m1 / B2
    b = -2 * Sp / B2
    c = 2 * L / B2
    if wrong_halo:
        S = Sp[:, :, 10:10 + H - 10, 10:10 + W - 10].mean()
        maps = (a, b, c)                                             # positions -10 .. H - 1: already the extended frame
    else:
        S = Sp.mean()
        maps = tuple(F.pad(t, (10, 10, 10, 10)) for t in (a, b, c))      # zero outside the valid domain
    N = B * (H - 10) * (W - 10) * (1 if wrong_count else C)
    Ga, Gb, Gc = (_filter_valid(t, g) for t in maps)                # symmetric window: the full filtering is the adjoint
    return S, (Ga + x * Gb + y * Gc) / N


def ssim_autograd(x, y, data_range=1.0, dtype=torch.float64):
    """(S, dS/dx) by autograd of metrics.ssim_torch on the CPU in `dtype`, returned as fp64"""
    from tpu_superresolution_amd.metrics import ssim_torch
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    S = ssim_torch(xl, y.detach().to(dtype), data_range=data_range, size_average=True)
    (gr,) = torch.autograd.grad(S, xl)
    return S.detach().double(), gr.double()


SSIM_SHAPES = [(1, 1, 11, 11), (2, 3, 12, 45), (1, 3, 43, 44), (2, 1, 75, 33)]
SSIM_INPUTS = ("smooth", "random", "flat")


def ssim_inputs(kind, shape, seed=0):
    """(pred, target) fp32 in [0, 1]-ish: 'smooth' = 5x5 box-blurred uniform target, pred = target + 0.05 randn; 'random' = two
    uniforms; 'flat' = 0.5 / 0.9 half-planes, pred = target + 0.001 randn (ill-conditioned: C2 carries the denominator)."""
    g = torch.Generator().manual_seed(1000 * SSIM_INPUTS.index(kind) + seed)
    B, C, H, W = shape
    if kind == "smooth":
        t = F.avg_pool2d(torch.rand(B, C, H + 4, W + 4, generator=g), 5, stride=1)
        return t + 0.05 * torch.randn(shape, generator=g), t
    if kind == "random":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if kind == "flat":
        t = torch.full(shape, 0.5)
        t[..., W // 2:] = 0.9
        return t + 0.001 * torch.randn(shape, generator=g), t
    raise ValueError(kind)
