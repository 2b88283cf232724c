"""2-D blur tables for the PSF degradation (include/srk.h "General 2-D blur"; ops.blur2d, ops.degrade_psf, sr_datasets.PsfSpec): the
kernel pool of BSRGAN / Real-ESRGAN -- rotated anisotropic Gaussians, generalized Gaussians, plateau kernels -- evaluated in fp64 numpy,
normalised in fp64 and rounded once to fp32.

A table is ks x ks, ks odd in 1..21, R = (ks - 1) / 2, row a <-> y = a - R, column b <-> x = b - R.  With q = (x, y) and
Sigma = Rot(theta) diag(s1^2, s2^2) Rot(theta)^T, theta counter-clockwise in the (x, y) frame of the array (y grows downwards):
    gaussian     exp(-0.5 q^T Sigma^-1 q)
    generalized  exp(-0.5 (q^T Sigma^-1 q)^beta)
    plateau      1 / ((q^T Sigma^-1 q)^beta + 1)
At theta = 0, s1 is the sigma along x (columns) and s2 the one along y (rows); theta = pi / 2 swaps them.  The device applies a table as a
correlation, so what matters for an asymmetric table is this orientation and nothing is flipped anywhere."""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import numpy as np

KS_MAX = 21


def check_ks(ks) -> int:
    if isinstance(ks, bool) or int(ks) != ks or not 1 <= int(ks) <= KS_MAX or int(ks) % 2 == 0:
        raise ValueError(f"a blur table is ks x ks with ks odd in 1..{KS_MAX} (got {ks!r})")
    return int(ks)


_GRIDS: dict = {}


def _grid(ks: int):
    """(x^2, x y, y^2) of the integer grid of a ks x ks table, made once per size."""
    if ks not in _GRIDS:
        r = (ks - 1) // 2
        y, x = np.meshgrid(np.arange(-r, r + 1, dtype=np.float64), np.arange(-r, r + 1, dtype=np.float64), indexing="ij")
        _GRIDS[ks] = (x * x, x * y, y * y)
    return _GRIDS[ks]


def _quad_coef(s1: float, s2: float, theta: float):
    """(A, B2, C) of q^T Sigma^-1 q = A x^2 + B2 x y + C y^2 with Sigma^-1 = Rot diag(1 / s1^2, 1 / s2^2) Rot^T written out.  The
    device builds its tables from these three doubles (TableDesc.row), so its q has the bits of `_quad`'s."""
    s1, s2, theta = float(s1), float(s2), float(theta)
    if not (s1 > 0.0 and s2 > 0.0 and math.isfinite(s1) and math.isfinite(s2) and math.isfinite(theta)):
        raise ValueError(f"blur sigmas must be finite and > 0, theta finite (got {(s1, s2, theta)})")
    c, s = math.cos(theta), math.sin(theta)
    i1, i2 = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    return c * c * i1 + s * s * i2, 2.0 * c * s * (i1 - i2), s * s * i1 + c * c * i2


def _quad(ks: int, s1: float, s2: float, theta: float) -> np.ndarray:
    """q^T Sigma^-1 q on the grid of a ks x ks table: (A x^2 + B2 x y) + C y^2."""
    ks = check_ks(ks)
    a, b2, c = _quad_coef(s1, s2, theta)
    xx, xy, yy = _grid(ks)
    return a * xx + b2 * xy + c * yy


def _finish(k: np.ndarray) -> np.ndarray:
    return (k / k.sum()).astype(np.float32)


def gaussian(ks: int, s1: float, s2: float, theta: float = 0.0) -> np.ndarray:
    return _finish(np.exp(-0.5 * _quad(ks, s1, s2, theta)))


USM_KS_MAX = 51


def gaussian1d(ks: int, sigma: float) -> np.ndarray:
    """The 1-D Gaussian taps of the unsharp mask (ops.usm_sharpen), cv2.getGaussianKernel's closed form: exp(-(i - R)^2 / (2 sigma^2)),
    ks odd in 1..51, normalised in fp64 and rounded once to fp32.  The 2-D table of Real-ESRGAN's USMSharp is the outer product."""
    if isinstance(ks, bool) or int(ks) != ks or not 1 <= int(ks) <= USM_KS_MAX or int(ks) % 2 == 0:
        raise ValueError(f"unsharp-mask taps: ks odd in 1..{USM_KS_MAX} (got {ks!r})")
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"unsharp-mask taps: sigma must be finite and > 0 (got {sigma!r})")
    r = (int(ks) - 1) // 2
    d = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


def _beta(beta) -> float:
    beta = float(beta)
    if not (beta > 0.0 and np.isfinite(beta)):
        raise ValueError(f"beta must be finite and > 0 (got {beta!r})")
    return beta


def generalized(ks: int, s1: float, s2: float, theta: float, beta: float) -> np.ndarray:
    return _finish(np.exp(-0.5 * _quad(ks, s1, s2, theta) ** _beta(beta)))


def plateau(ks: int, s1: float, s2: float, theta: float, beta: float) -> np.ndarray:
    return _finish(1.0 / (_quad(ks, s1, s2, theta) ** _beta(beta) + 1.0))


def pad_to(table, ks: int) -> np.ndarray:
    """`table` zero-padded, centred, to ks x ks: the device gives identical bits for both on finite images."""
    t = np.asarray(table, dtype=np.float32)
    ks = check_ks(ks)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] % 2 == 0 or t.shape[0] > ks:
        raise ValueError(f"pad_to: an odd square table of at most {ks} x {ks} (got {t.shape})")
    return np.pad(t, (ks - t.shape[0]) // 2)


def check_table(table, what: str = "psf") -> np.ndarray:
    """The host rule of a table -> fp32 [ks][ks]: odd square with ks <= 21, taps finite and >= 0, a centre > 0 (so that the mass is > 0 at
    every pixel), an fp64 sum within 1e-3 of 1."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] % 2 == 0 or not 1 <= t.shape[0] <= KS_MAX:
        raise ValueError(f"{what}: a table is ks x ks with ks odd in 1..{KS_MAX} (got shape {t.shape})")
    t = t.astype(np.float32)
    if not np.isfinite(t).all():
        raise ValueError(f"{what}: taps must be finite")
    if (t < 0).any():
        raise ValueError(f"{what}: taps must be >= 0 (kernels with negative lobes need another mass rule)")
    r = t.shape[0] // 2
    if not t[r, r] > 0:
        raise ValueError(f"{what}: the centre tap must be > 0")
    total = float(t.astype(np.float64).sum())
    if abs(total - 1.0) > 1e-3:
        raise ValueError(f"{what}: the taps must sum to 1 within 1e-3 (got {total:.6f})")
    return t


# ---- signed tables of the second-order degradation (include/srk.h: srk_filter2d_f32; ops.filter2d) ------------------------------
_J1_N = 512          # intervals of the trapezoid rule below


def j1(z) -> np.ndarray:
    """The Bessel function J1 in fp64 numpy: the trapezoid rule on Bessel's integral (1 / pi) int_0^pi cos(t - z sin t) dt.  The
    integrand is an even 2 pi-periodic entire function of t, so the rule converges geometrically once the intervals outnumber |z|:
    512 of them give fp64 rounding error for |z| < 200 (a 21 x 21 sinc table needs |z| <= 10 sqrt(2) pi < 45)."""
    z = np.asarray(z, dtype=np.float64)
    if not np.isfinite(z).all() or (np.abs(z) >= 200.0).any():
        raise ValueError("j1: arguments must be finite and below 200 in magnitude")
    t = np.linspace(0.0, math.pi, _J1_N + 1)
    f = np.cos(t - z[..., None] * np.sin(t))
    return (f[..., 1:-1].sum(-1) + 0.5 * (f[..., 0] + f[..., -1])) / _J1_N


def sinc(cutoff: float, ks: int) -> np.ndarray:
    """Real-ESRGAN's circular low-pass (sinc) kernel, the source of ringing and overshoot: off-centre taps cutoff J1(cutoff r) / (2 pi r)
    at r = |(x, y)|, the centre tap cutoff^2 / (4 pi); normalised to sum 1 in fp64 and rounded once to fp32.  cutoff in (0, pi] radians
    per pixel.  The table has negative lobes: it goes through ops.filter2d (reflect border, no mass), never through ops.blur2d."""
    ks = check_ks(ks)
    cutoff = float(cutoff)
    if not 0.0 < cutoff <= math.pi:          # also refuses NaN
        raise ValueError(f"sinc: the cutoff must be in (0, pi] (got {cutoff!r})")
    xx, _, yy = _grid(ks)
    r = np.sqrt(xx + yy)
    c = (ks - 1) // 2
    r[c, c] = 1.0          # any value: the tap is replaced below
    k = cutoff * j1(cutoff * r) / (2.0 * math.pi * r)
    k[c, c] = cutoff * cutoff / (4.0 * math.pi)
    return _finish(k)


def delta(ks: int = 1) -> np.ndarray:
    """The identity table: ops.filter2d passes a sample with it through bit for bit."""
    t = np.zeros((check_ks(ks),) * 2, dtype=np.float32)
    t[ks // 2, ks // 2] = 1.0
    return t


def check_filter_table(table, what: str = "table") -> np.ndarray:
    """The host rule of a table for ops.filter2d -> fp32 [ks][ks]: odd square with ks <= 21, taps finite, an fp64 sum within 1e-3 of 1.
    No sign rule: the reflect border needs no mass."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] % 2 == 0 or not 1 <= t.shape[0] <= KS_MAX:
        raise ValueError(f"{what}: a table is ks x ks with ks odd in 1..{KS_MAX} (got shape {t.shape})")
    t = t.astype(np.float32)
    if not np.isfinite(t).all():
        raise ValueError(f"{what}: taps must be finite")
    total = float(t.astype(np.float64).sum())
    if abs(total - 1.0) > 1e-3:
        raise ValueError(f"{what}: the taps must sum to 1 within 1e-3 (got {total:.6f})")
    return t


def load_psf_file(path: str) -> np.ndarray:
    """A measured PSF: .npy of shape [k][k] or [n][k][k] -> checked fp32 [n][k][k]."""
    a = np.load(path, allow_pickle=False)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] < 1:
        raise ValueError(f"{path}: a PSF file holds [k][k] or [n][k][k] (got shape {a.shape})")
    return np.stack([check_table(t, f"{path}[{i}]") for i, t in enumerate(a)])


# ---- descriptors: a table as eight numbers, for the device to build (include/srk.h: srk_kernel_tables_f32; ops.kernel_tables) ------
KIND_DELTA, KIND_GAUSSIAN, KIND_GENERALIZED, KIND_PLATEAU, KIND_SINC, KIND_BANK = range(6)


class TableDesc(NamedTuple):
    """What one table is made from: the arguments of `delta` / `gaussian` / `generalized` / `plateau` / `sinc`, or the index of a
    measured PSF in a bank (`load_psf_file`).  The constructors below take the arguments of those functions and refuse what they
    refuse, with their errors; `table()` IS that function's table, `row()` the eight doubles the device reads."""
    kind: int
    ks: int
    s1: float = 1.0
    s2: float = 1.0
    theta: float = 0.0
    beta: float = 1.0
    cutoff: float = 0.0
    bank_index: int = 0

    @classmethod
    def delta(cls, ks: int = 1) -> "TableDesc":
        return cls(KIND_DELTA, check_ks(ks))

    @classmethod
    def gaussian(cls, ks: int, s1: float, s2: float, theta: float = 0.0) -> "TableDesc":
        ks = check_ks(ks)
        _quad_coef(s1, s2, theta)
        return cls(KIND_GAUSSIAN, ks, float(s1), float(s2), float(theta))

    @classmethod
    def generalized(cls, ks: int, s1: float, s2: float, theta: float, beta: float) -> "TableDesc":
        ks = check_ks(ks)
        _quad_coef(s1, s2, theta)
        return cls(KIND_GENERALIZED, ks, float(s1), float(s2), float(theta), _beta(beta))

    @classmethod
    def plateau(cls, ks: int, s1: float, s2: float, theta: float, beta: float) -> "TableDesc":
        ks = check_ks(ks)
        _quad_coef(s1, s2, theta)
        return cls(KIND_PLATEAU, ks, float(s1), float(s2), float(theta), _beta(beta))

    @classmethod
    def sinc(cls, cutoff: float, ks: int) -> "TableDesc":
        ks = check_ks(ks)
        cutoff = float(cutoff)
        if not 0.0 < cutoff <= math.pi:          # also refuses NaN
            raise ValueError(f"sinc: the cutoff must be in (0, pi] (got {cutoff!r})")
        return cls(KIND_SINC, ks, cutoff=cutoff)

    @classmethod
    def bank(cls, index: int, ks: int) -> "TableDesc":
        """Table `index` of a bank of checked ks x ks tables (PsfSpec's `file`)."""
        if isinstance(index, bool) or int(index) != index or int(index) < 0:
            raise ValueError(f"a bank index is an integer >= 0 (got {index!r})")
        return cls(KIND_BANK, check_ks(ks), bank_index=int(index))

    def table(self, bank=None) -> np.ndarray:
        """The host table: the very function of this module (kind 5: the bank's table, which `bank` must then hold)."""
        if self.kind == KIND_DELTA:
            return delta(self.ks)
        if self.kind == KIND_GAUSSIAN:
            return gaussian(self.ks, self.s1, self.s2, self.theta)
        if self.kind == KIND_GENERALIZED:
            return generalized(self.ks, self.s1, self.s2, self.theta, self.beta)
        if self.kind == KIND_PLATEAU:
            return plateau(self.ks, self.s1, self.s2, self.theta, self.beta)
        if self.kind == KIND_SINC:
            return sinc(self.cutoff, self.ks)
        if self.kind == KIND_BANK:
            if bank is None or not 0 <= self.bank_index < len(bank) or tuple(np.shape(bank[self.bank_index])) != (self.ks, self.ks):
                raise ValueError(f"a bank descriptor needs the bank that holds its {self.ks} x {self.ks} table {self.bank_index}")
            return np.asarray(bank[self.bank_index], dtype=np.float32)
        raise ValueError(f"unknown table kind {self.kind!r}")

    def row(self) -> Tuple[float, ...]:
        """(kind, ks, A, B2, C, beta, cutoff, bank_index) as eight doubles; A, B2, C are `_quad`'s coefficients."""
        if not (isinstance(self.kind, int) and KIND_DELTA <= self.kind <= KIND_BANK):
            raise ValueError(f"unknown table kind {self.kind!r}")
        a, b2, c = _quad_coef(self.s1, self.s2, self.theta) if KIND_GAUSSIAN <= self.kind <= KIND_PLATEAU else (0.0, 0.0, 0.0)
        return (float(self.kind), float(check_ks(self.ks)), a, b2, c, float(self.beta), float(self.cutoff), float(self.bank_index))
