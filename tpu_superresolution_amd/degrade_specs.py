"""The degradation specs of the on-device data path: what a training sample's blur, noise, JPEG, PSF, unsharp mask, second-order chain
and scale-1 restoration are drawn from (each from a generator of its own, never the global `random`), and the `Fixed*` tuples that
validation scores.  Pure Python: nothing here touches the device.  sr_datasets.py, whose pools consume them, imports every name back,
so `sr_datasets.DegradeSpec` and the rest stay valid spellings.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch


class FixedDegrade(NamedTuple):
    """One fixed blind degradation (validation, evaluation): blur = (sigma_y, sigma_x) in HR pixels, noise = (sigma_n, gain) in [0, 1]
    units, gray_noise = one draw for the three channels of a colour image (a gray image always gets one)."""
    blur: Tuple[float, float]
    noise: Tuple[float, float]
    gray_noise: bool = False


def _check_range(name: str, r, hi: float) -> Tuple[float, float]:
    try:
        a, b = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two numbers LO HI (got {r!r})") from None
    if not 0.0 <= a <= b <= hi:          # also refuses NaN
        raise ValueError(f"{name} must satisfy 0 <= LO <= HI <= {hi:g} (got {a} {b})")
    return a, b


@dataclass(frozen=True)
class DegradeSpec:
    """The random first-order degradation of `--degrade blind`: per training sample a Gaussian blur with sigma_y uniform in
    `blur_sigma` HR pixels and, with probability `blur_aniso_p`, an independent sigma_x (else sigma_x = sigma_y); noise
    `sqrt(sigma_n^2 + gain v) z` with sigma_n uniform in `noise_sigma` and gain uniform in `noise_gain` (image units, [0, 1]); for a
    colour image one draw for all channels with probability `gray_noise_p`; a 64-bit noise id.  Everything comes from the spec's OWN
    generator `random.Random(seed + rank)`: the global `random` state, which places the crops, never sees it."""
    blur_sigma: Tuple[float, float] = (0.2, 2.0)
    blur_aniso_p: float = 0.5
    noise_sigma: Tuple[float, float] = (0.0, 10.0 / 255.0)
    noise_gain: Tuple[float, float] = (0.0, 0.0)
    gray_noise_p: float = 0.4
    seed: int = 0

    def __post_init__(self):
        from .ops import BLUR_SIGMA_MAX
        object.__setattr__(self, "blur_sigma", _check_range("blur_sigma", self.blur_sigma, BLUR_SIGMA_MAX))
        object.__setattr__(self, "noise_sigma", _check_range("noise_sigma", self.noise_sigma, 1.0))
        object.__setattr__(self, "noise_gain", _check_range("noise_gain", self.noise_gain, 1.0))
        for name in ("blur_aniso_p", "gray_noise_p"):
            if not 0.0 <= float(getattr(self, name)) <= 1.0:
                raise ValueError(f"{name} must be a probability (got {getattr(self, name)!r})")

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(int(self.seed) + int(rank))

    def draw(self, rng: random.Random, colour: bool):
        """-> (blur, noise, noise_id, gray_noise) of one sample; always the same seven variates, whatever they decide."""
        sy, sx = rng.uniform(*self.blur_sigma), rng.uniform(*self.blur_sigma)
        aniso = rng.random() < self.blur_aniso_p
        noise = (rng.uniform(*self.noise_sigma), rng.uniform(*self.noise_gain))
        gray = rng.random() < self.gray_noise_p
        return (sy, sx if aniso else sy), noise, rng.getrandbits(64), gray or not colour

    def fixed(self) -> FixedDegrade:
        """The midpoints of the ranges: what validation scores, every epoch and every run."""
        mid = lambda r: 0.5 * (r[0] + r[1])          # noqa: E731
        return FixedDegrade((mid(self.blur_sigma),) * 2, (mid(self.noise_sigma), mid(self.noise_gain)), self.gray_noise_p >= 0.5)


@dataclass(frozen=True)
class JpegSpec:
    """The JPEG stage of `--jpeg_quality`: per training sample, with probability `p`, a round trip through baseline JPEG at
    a quality uniform in the integers `quality` = (lo, hi), 1 <= lo <= hi <= 100; otherwise the sample passes through (quality 0).
    `subsample`: chroma at 4:2:0 instead of 4:4:4.  The qualities come from the spec's OWN generator
    `random.Random(f"jpeg:{seed + rank}")`: neither the global `random` state nor a DegradeSpec's generator sees it."""
    quality: Tuple[int, int] = (30, 95)
    p: float = 1.0
    subsample: bool = False
    seed: int = 0

    def __post_init__(self):
        from .ops import check_jpeg_quality
        try:
            lo, hi = self.quality
        except (TypeError, ValueError):
            raise ValueError(f"jpeg quality must be two integers LO HI (got {self.quality!r})") from None
        lo, hi = check_jpeg_quality(lo, "quality LO"), check_jpeg_quality(hi, "quality HI")
        if lo > hi:
            raise ValueError(f"jpeg quality must satisfy 1 <= LO <= HI <= 100 (got {lo} {hi})")
        if not 0.0 <= float(self.p) <= 1.0:          # also refuses NaN
            raise ValueError(f"jpeg p must be a probability (got {self.p!r})")
        object.__setattr__(self, "quality", (lo, hi))
        object.__setattr__(self, "subsample", bool(self.subsample))

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"jpeg:{int(self.seed) + int(rank)}")

    def draw(self, rng: random.Random) -> int:
        """-> the quality of one sample, 0 = pass-through; always the same two variates, whatever they decide."""
        lo, hi = self.quality
        take, q = rng.random() < self.p, min(lo + int(rng.random() * (hi - lo + 1)), hi)
        return q if take else 0

    def fixed(self) -> int:
        """The middle of the range: what validation scores, every epoch and every run."""
        return round((self.quality[0] + self.quality[1]) / 2)


PSF_MODES = ("rotated", "mixed", "file")
TABLE_MODES = ("host", "device")          # where a pool's blur / sinc tables are evaluated
PSF_SIGMA_FLOOR = 1e-3          # a sigma of 0 (no blur on that axis) as a Gaussian: every tap off the axis underflows to 0


@dataclass(frozen=True)
class PsfSpec:
    """The 2-D blur of `--blur_kernel rotated|mixed` / `--blur_psf FILE`: per training sample one ks x ks table
    (blur_kernels) in place of the axis-aligned Gaussian.  It takes the (sigma_y, sigma_x) that `DegradeSpec.draw` produced -- as
    (s2, s1): at theta = 0 the table is the separable path's Gaussian -- and draws the rest from its OWN generator
    `random.Random(f"psf:{seed + rank}")`, six variates per sample whatever they decide.
    `rotated`: a Gaussian, theta uniform in [-pi/2, pi/2), ks = 2 min(ceil(3 max(s1, s2)), 10) + 1.
    `mixed`: Real-ESRGAN's six kinds {iso, aniso, generalized iso / aniso, plateau iso / aniso} with probabilities `kernel_prob`
    (iso: s2 = s1), beta uniform in `beta_g` / `beta_p`, an odd ks uniform in `ksize`.
    `file`: one table, uniformly, of the .npy `file` ([k][k] or [n][k][k]), a measured point-spread function."""
    mode: str = "rotated"
    kernel_prob: Tuple[float, ...] = (0.45, 0.25, 0.12, 0.03, 0.12, 0.03)
    beta_g: Tuple[float, float] = (0.5, 4.0)
    beta_p: Tuple[float, float] = (1.0, 2.0)
    ksize: Tuple[int, int] = (7, 21)
    file: Optional[str] = None
    seed: int = 0

    def __post_init__(self):
        from . import blur_kernels as bk
        if self.mode not in PSF_MODES:
            raise ValueError(f"psf mode must be one of {PSF_MODES} (got {self.mode!r})")
        try:
            prob = tuple(float(v) for v in self.kernel_prob)
        except (TypeError, ValueError):
            raise ValueError(f"kernel_prob must be six numbers (got {self.kernel_prob!r})") from None
        if len(prob) != 6 or not all(0.0 <= v <= 1.0 for v in prob) or abs(sum(prob) - 1.0) > 1e-6:
            raise ValueError(f"kernel_prob must be six probabilities that sum to 1 (got {self.kernel_prob!r})")
        object.__setattr__(self, "kernel_prob", prob)
        for name in ("beta_g", "beta_p"):
            try:
                lo, hi = (float(v) for v in getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be two numbers LO HI (got {getattr(self, name)!r})") from None
            if not 0.0 < lo <= hi <= 16.0:          # also refuses NaN
                raise ValueError(f"{name} must satisfy 0 < LO <= HI <= 16 (got {lo} {hi})")
            object.__setattr__(self, name, (lo, hi))
        try:
            lo, hi = self.ksize
            lo, hi = bk.check_ks(lo), bk.check_ks(hi)
        except (TypeError, ValueError):
            raise ValueError(f"ksize must be two odd integers LO HI in 1..{bk.KS_MAX} (got {self.ksize!r})") from None
        if lo > hi:
            raise ValueError(f"ksize must satisfy LO <= HI (got {lo} {hi})")
        object.__setattr__(self, "ksize", (lo, hi))
        if (self.mode == "file") != (self.file is not None):
            raise ValueError("psf mode 'file' needs file=, and the other modes take none")
        object.__setattr__(self, "_tables", bk.load_psf_file(self.file) if self.file is not None else None)

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"psf:{int(self.seed) + int(rank)}")

    @property
    def tables(self):
        """The checked tables of `file`, fp32 [n][k][k] (None in the other modes)."""
        return self._tables

    def draw(self, rng: random.Random, blur, as_desc: bool = False):
        """-> the fp32 table of one sample with blur = (sigma_y, sigma_x); always the same six variates, whatever they decide.
        as_desc: the `blur_kernels.TableDesc` of that table instead (`file`: a kind-5 descriptor into `tables`), for
        `ops.kernel_tables` to build on the device; same variates, same decisions."""
        from . import blur_kernels as bk
        if as_desc:
            bk = bk.TableDesc
        u_kind, u_theta, u_bg, u_bp, u_ks, u_idx = (rng.random() for _ in range(6))
        if self.mode == "file":
            idx = min(int(u_idx * len(self._tables)), len(self._tables) - 1)
            return bk.bank(idx, self._tables.shape[1]) if as_desc else self._tables[idx]
        s2, s1 = (max(float(v), PSF_SIGMA_FLOOR) for v in blur)
        theta = math.pi * (u_theta - 0.5)
        if self.mode == "rotated":
            return bk.gaussian(2 * min(math.ceil(3.0 * max(0.0, *(float(v) for v in blur))), 10) + 1, s1, s2, theta)          # sigma 0: R = 0
        kind, acc = 5, 0.0
        for i, pr in enumerate(self.kernel_prob):
            acc += pr
            if u_kind < acc:
                kind = i
                break
        lo, hi = self.ksize
        n = (hi - lo) // 2 + 1
        ks = lo + 2 * min(int(u_ks * n), n - 1)
        if kind % 2 == 0:          # the isotropic kinds
            s2 = s1
        if kind < 2:
            return bk.gaussian(ks, s1, s2, theta)
        if kind < 4:
            return bk.generalized(ks, s1, s2, theta, self.beta_g[0] + u_bg * (self.beta_g[1] - self.beta_g[0]))
        return bk.plateau(ks, s1, s2, theta, self.beta_p[0] + u_bp * (self.beta_p[1] - self.beta_p[0]))

    def fixed(self):
        """Table 0 of `file` (what validation scores); None in the other modes: validation keeps the isotropic midpoints, for which a
        rotation is moot."""
        return self._tables[0] if self._tables is not None else None


def _check_prob3(name: str, p, what: str = "UP DOWN KEEP") -> Tuple[float, float, float]:
    try:
        prob = tuple(float(v) for v in p)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three numbers {what} (got {p!r})") from None
    if len(prob) != 3 or not all(0.0 <= v <= 1.0 for v in prob) or abs(sum(prob) - 1.0) > 1e-6:
        raise ValueError(f"{name} must be three probabilities {what} that sum to 1 (got {p!r})")
    return prob


def _check_factors(name: str, r) -> Tuple[float, float]:
    try:
        lo, hi = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two numbers LO HI (got {r!r})") from None
    if not 0.125 <= lo <= 1.0 <= hi <= 2.0:          # also refuses NaN; below 1/8 the resize has more than 33 taps
        raise ValueError(f"{name} must satisfy 0.125 <= LO <= 1 <= HI <= 2 (got {lo} {hi})")
    return lo, hi


@dataclass(frozen=True)
class UsmSpec:
    """The unsharp mask of `--gt_usm` (Real-ESRGAN's `gt_usm`; `ops.usm_sharpen`): `radius` 1..51 (ks = radius + 1 if it is even),
    `sigma` (<= 0: OpenCV's rule from ks), `weight` of the residual, `threshold` of the mask in 8-bit levels."""
    radius: int = 50
    sigma: float = 0.0
    weight: float = 0.5
    threshold: float = 10.0

    def __post_init__(self):
        from .ops import usm_ks
        usm_ks(self.radius)
        for name, lo, hi in (("sigma", -math.inf, 100.0), ("weight", 0.0, 10.0), ("threshold", 0.0, 255.0)):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"usm {name} must be a number (got {getattr(self, name)!r})") from None
            if not (lo <= v <= hi) or (name == "sigma" and not math.isfinite(v)):          # also refuses NaN
                raise ValueError(f"usm {name} must be in [{lo}, {hi}] (got {v!r})")
            object.__setattr__(self, name, v)
        object.__setattr__(self, "radius", int(self.radius))

    @property
    def ks(self) -> int:
        from .ops import usm_ks
        return usm_ks(self.radius)

    def sharpen(self, x: torch.Tensor) -> torch.Tensor:
        from .ops import usm_sharpen
        return usm_sharpen(x, self.radius, self.sigma, self.weight, self.threshold)


SECOND_ORDER_VARIATES = 23          # per SecondOrderSpec.draw, whatever they decide


@dataclass(frozen=True)
class SecondOrderSpec:
    """The random second-order degradation of `--degrade second_order` (Real-ESRGAN's chain and defaults): what one
    `ops.SecondOrder` is drawn from, on top of the first-order draws that stage 1 reuses -- the blur table of the 7n pool (PsfSpec on
    DegradeSpec's sigmas) and DegradeSpec's noise, gray flag and noise id.
    Stage 1: with probability `sinc_p` the table is a sinc filter instead; a resize by a factor that goes up / down / stays with
    probabilities `resize_prob`, uniform in [1, HI] / [LO, 1] of `resize_range`; JPEG at a quality uniform in `jpeg_quality`.
    Stage 2: with probability `blur2_p` a filter -- a sinc with probability `sinc_p`, else a rotated anisotropic Gaussian with sigmas
    uniform in `blur2_sigma` -- else none (a table that would not fit the size it filters, R >= an extent, is dropped at any stage);
    `resize2_prob` / `resize2_range` relative to the LR size; noise uniform in `noise2_sigma` / `noise2_gain`, gray with `gray_noise_p`;
    JPEG at `jpeg2_quality`, before or after the final resize and filter with equal probability.
    Final: with probability `final_sinc_p` a sinc filter.  A sinc table has an odd side uniform in `ksize` and a cutoff uniform in
    [pi/3, pi] for sides below 13, else [pi/5, pi].
    Everything comes from the spec's OWN generator `random.Random(f"degrade2:{seed + rank}")`, 23 variates per draw whatever they
    decide: the global `random` state and the other specs' generators never see it.
    `resize_mode_prob` = the probabilities AREA BILINEAR BICUBIC of the rule of each of the three resizes (`ops.resize_ragged`;
    Real-ESRGAN draws among the three), from a generator of their own, `random.Random(f"degrade2mode:{seed + rank}")`, three variates
    per draw: the 23 variates above and their generator are the same whatever it holds.  The default (0, 0, 1) is the antialiased
    cubic at every resize."""
    resize_prob: Tuple[float, float, float] = (0.2, 0.7, 0.1)
    resize_range: Tuple[float, float] = (0.15, 1.5)
    resize2_prob: Tuple[float, float, float] = (0.3, 0.4, 0.3)
    resize2_range: Tuple[float, float] = (0.3, 1.2)
    blur2_p: float = 0.8
    blur2_sigma: Tuple[float, float] = (0.2, 1.5)
    sinc_p: float = 0.1
    final_sinc_p: float = 0.8
    ksize: Tuple[int, int] = (7, 21)
    noise2_sigma: Tuple[float, float] = (1.0 / 255.0, 25.0 / 255.0)
    noise2_gain: Tuple[float, float] = (0.0, 0.0)
    gray_noise_p: float = 0.4
    jpeg_quality: Tuple[int, int] = (30, 95)
    jpeg2_quality: Tuple[int, int] = (30, 95)
    seed: int = 0
    resize_mode_prob: Tuple[float, float, float] = (0.0, 0.0, 1.0)

    def __post_init__(self):
        from . import blur_kernels as bk
        from .ops import check_jpeg_quality
        object.__setattr__(self, "resize_mode_prob", _check_prob3("resize_mode_prob", self.resize_mode_prob, "AREA BILINEAR BICUBIC"))
        object.__setattr__(self, "resize_prob", _check_prob3("resize_prob", self.resize_prob))
        object.__setattr__(self, "resize2_prob", _check_prob3("resize2_prob", self.resize2_prob))
        object.__setattr__(self, "resize_range", _check_factors("resize_range", self.resize_range))
        object.__setattr__(self, "resize2_range", _check_factors("resize2_range", self.resize2_range))
        for name in ("blur2_p", "sinc_p", "final_sinc_p", "gray_noise_p"):
            if not 0.0 <= float(getattr(self, name)) <= 1.0:          # also refuses NaN
                raise ValueError(f"{name} must be a probability (got {getattr(self, name)!r})")
        lo, hi = _check_range("blur2_sigma", self.blur2_sigma, 10.0)
        if lo <= 0.0:
            raise ValueError(f"blur2_sigma must be > 0 (got {lo} {hi})")
        object.__setattr__(self, "blur2_sigma", (lo, hi))
        object.__setattr__(self, "noise2_sigma", _check_range("noise2_sigma", self.noise2_sigma, 1.0))
        object.__setattr__(self, "noise2_gain", _check_range("noise2_gain", self.noise2_gain, 1.0))
        try:
            lo, hi = self.ksize
            lo, hi = bk.check_ks(lo), bk.check_ks(hi)
        except (TypeError, ValueError):
            raise ValueError(f"ksize must be two odd integers LO HI in 1..{bk.KS_MAX} (got {self.ksize!r})") from None
        if lo > hi:
            raise ValueError(f"ksize must satisfy LO <= HI (got {lo} {hi})")
        object.__setattr__(self, "ksize", (lo, hi))
        for name in ("jpeg_quality", "jpeg2_quality"):
            try:
                lo, hi = getattr(self, name)
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be two integers LO HI (got {getattr(self, name)!r})") from None
            lo, hi = check_jpeg_quality(lo, f"{name} LO"), check_jpeg_quality(hi, f"{name} HI")
            if lo > hi:
                raise ValueError(f"{name} must satisfy 1 <= LO <= HI <= 100 (got {lo} {hi})")
            object.__setattr__(self, name, (lo, hi))

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"degrade2:{int(self.seed) + int(rank)}")

    def mode_rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"degrade2mode:{int(self.seed) + int(rank)}")

    def draw_modes(self, mode_rng: Optional[random.Random]) -> Tuple[int, int, int]:
        """The `ops.SecondOrder.modes` of one sample: three variates of `mode_rng`, whatever they decide; None = the cubic."""
        if mode_rng is None:
            return (0, 0, 0)
        pa, pb, _ = self.resize_mode_prob
        pb += pa
        u0, u1, u2 = mode_rng.random(), mode_rng.random(), mode_rng.random()
        return (2 if u0 < pa else (1 if u0 < pb else 0), 2 if u1 < pa else (1 if u1 < pb else 0), 2 if u2 < pa else (1 if u2 < pb else 0))

    def _ks(self, u: float) -> int:
        lo, hi = self.ksize
        n = (hi - lo) // 2 + 1
        return lo + 2 * min(int(u * n), n - 1)

    @staticmethod
    def _cutoff(ks: int, u: float) -> float:
        lo = math.pi / 3.0 if ks < 13 else math.pi / 5.0
        return lo + u * (math.pi - lo)

    @staticmethod
    def _factor(prob, rng_, u_kind: float, u: float) -> float:
        lo, hi = rng_
        if u_kind < prob[0]:
            return 1.0 + u * (hi - 1.0)
        if u_kind < prob[0] + prob[1]:
            return lo + u * (1.0 - lo)
        return 1.0

    @staticmethod
    def _quality(q, u: float) -> int:
        return min(q[0] + int(u * (q[1] - q[0] + 1)), q[1])

    def draw(self, rng: random.Random, table1, noise1, noise_id: int, gray1: bool, colour: bool, extent: int, scale: int,
             as_desc: bool = False, mode_rng: Optional[random.Random] = None):
        """-> the `ops.SecondOrder` of one sample (as_desc: with `blur_kernels.TableDesc` descriptors for k1 / k2 / k3 -- table1 is then
        one too -- from the same variates and decisions).  table1, noise1, noise_id, gray1: the first-order draws (PsfSpec.draw or a Gaussian
        of DegradeSpec's sigmas; DegradeSpec.draw).  extent: the side of the square window the chain runs on at factor `scale`: it
        bounds filter 2, and factor 2 is raised where the second resize would shrink by more than the resampler's 8x (an upscale by
        1.5 followed by 0.3 / 4 is 20x; Real-ESRGAN's resize has no such limit because it does not antialias).  mode_rng: the
        generator of `mode_rng()`, which `draw_modes` reads; None leaves every resize the cubic."""
        from . import blur_kernels as bk
        from .ops import SecondOrder
        if as_desc:
            bk = bk.TableDesc
        u = [rng.random() for _ in range(SECOND_ORDER_VARIATES)]
        ks1 = self._ks(u[2])
        k1 = bk.sinc(self._cutoff(ks1, u[1]), ks1) if (u[0] < self.sinc_p and ks1 // 2 < extent) else table1
        r1 = self._factor(self.resize_prob, self.resize_range, u[3], u[4])
        ks2 = self._ks(u[9])
        if u[6] >= self.blur2_p or ks2 // 2 >= max(1, int(extent * r1 + 0.5)):
            k2 = bk.delta()
        elif u[7] < self.sinc_p:
            k2 = bk.sinc(self._cutoff(ks2, u[8]), ks2)
        else:
            lo, hi = self.blur2_sigma
            k2 = bk.gaussian(ks2, lo + u[10] * (hi - lo), lo + u[11] * (hi - lo), math.pi * (u[12] - 0.5))
        r2 = self._factor(self.resize2_prob, self.resize2_range, u[13], u[14])
        h1 = max(1, int(extent * r1 + 0.5))
        r2 = max(r2, (-(-h1 // 8) * int(scale) + 1e-6) / extent)
        noise2 = (self.noise2_sigma[0] + u[15] * (self.noise2_sigma[1] - self.noise2_sigma[0]),
                  self.noise2_gain[0] + u[16] * (self.noise2_gain[1] - self.noise2_gain[0]))
        ks3 = self._ks(u[22])
        k3 = bk.sinc(self._cutoff(ks3, u[21]), ks3) if (u[20] < self.final_sinc_p and ks3 // 2 < extent // int(scale)) else bk.delta()
        return SecondOrder(k1, r1, tuple(noise1), bool(gray1), self._quality(self.jpeg_quality, u[5]), k2, r2, noise2,
                           u[17] < self.gray_noise_p or not colour, self._quality(self.jpeg2_quality, u[18]), u[19] < 0.5, k3, int(noise_id),
                           self.draw_modes(mode_rng))

    def fixed(self, table1, noise1, gray1: bool = False, noise_id: int = 0):
        """What validation scores, every epoch and every run: no sinc at stages 1 and 2 (sinc_p < 0.5, else a sinc at the middle
        cutoff of a 13-tap table), the middle of the DOWN range at both resizes, an isotropic Gaussian at the middle `blur2_sigma`
        when blur2_p >= 0.5, the middle noise and qualities, order A (JPEG before the final resize), and when final_sinc_p >= 0.5 a
        13-tap final sinc at the middle of its cutoff range.  table1 / noise1 / gray1: the fixed first-order stage (FixedDegrade)."""
        from . import blur_kernels as bk
        from .ops import SecondOrder
        mid = lambda r: 0.5 * (r[0] + r[1])          # noqa: E731
        sinc13 = bk.sinc(self._cutoff(13, 0.5), 13)
        k2 = bk.delta() if self.blur2_p < 0.5 else (sinc13 if self.sinc_p >= 0.5 else bk.gaussian(13, mid(self.blur2_sigma), mid(self.blur2_sigma)))
        return SecondOrder(sinc13 if self.sinc_p >= 0.5 else table1, 0.5 * (self.resize_range[0] + 1.0), tuple(noise1), bool(gray1),
                           round(mid(self.jpeg_quality)), k2, 0.5 * (self.resize2_range[0] + 1.0),
                           (mid(self.noise2_sigma), mid(self.noise2_gain)), self.gray_noise_p >= 0.5, round(mid(self.jpeg2_quality)), False,
                           sinc13 if self.final_sinc_p >= 0.5 else bk.delta(), int(noise_id))


class FixedRestore(NamedTuple):
    """One fixed scale-1 degradation (validation, evaluation): the noise sigma in image units (0..1), the JPEG quality (0 = no JPEG
    stage), gray_noise = one draw for the three channels of a colour image, subsample = chroma at 4:2:0."""
    sigma: float
    jpeg_quality: int = 0
    gray_noise: bool = False
    subsample: bool = False


@dataclass(frozen=True)
class RestoreSpec:
    """The random degradation of `--task dn | car`: per training sample Gaussian noise with sigma uniform in `sigma`
    (image units, 0..1) and, with `jpeg_quality` = (lo, hi), a round trip through baseline JPEG at a quality uniform in the integers
    lo..hi (None = no JPEG stage); for a colour image one noise draw for all channels with probability `gray_noise_p`; `subsample`:
    chroma at 4:2:0; a 64-bit noise id.  Everything comes from the spec's OWN generator `random.Random(f"restore:{seed + rank}")`:
    neither the global `random` state, which places the crops, nor a DegradeSpec's or JpegSpec's generator sees it."""
    sigma: Tuple[float, float] = (0.0, 0.0)
    jpeg_quality: Optional[Tuple[int, int]] = None
    gray_noise_p: float = 0.0
    subsample: bool = False
    seed: int = 0

    def __post_init__(self):
        from .ops import check_jpeg_quality
        object.__setattr__(self, "sigma", _check_range("sigma", self.sigma, 1.0))
        if self.jpeg_quality is not None:
            try:
                lo, hi = self.jpeg_quality
            except (TypeError, ValueError):
                raise ValueError(f"jpeg quality must be two integers LO HI or None (got {self.jpeg_quality!r})") from None
            lo, hi = check_jpeg_quality(lo, "quality LO"), check_jpeg_quality(hi, "quality HI")
            if lo > hi:
                raise ValueError(f"jpeg quality must satisfy 1 <= LO <= HI <= 100 (got {lo} {hi})")
            object.__setattr__(self, "jpeg_quality", (lo, hi))
        if not 0.0 <= float(self.gray_noise_p) <= 1.0:          # also refuses NaN
            raise ValueError(f"gray_noise_p must be a probability (got {self.gray_noise_p!r})")
        object.__setattr__(self, "subsample", bool(self.subsample))

    def rng(self, rank: int = 0) -> random.Random:
        return random.Random(f"restore:{int(self.seed) + int(rank)}")

    def draw(self, rng: random.Random, colour: bool):
        """-> (sigma, quality, noise_id, gray_noise) of one sample, quality 0 = no JPEG stage; always the same four variates, whatever
        they decide."""
        sigma, u_q = rng.uniform(*self.sigma), rng.random()
        gray = rng.random() < self.gray_noise_p
        q = 0
        if self.jpeg_quality is not None:
            lo, hi = self.jpeg_quality
            q = min(lo + int(u_q * (hi - lo + 1)), hi)
        return sigma, q, rng.getrandbits(64), gray or not colour

    def fixed(self) -> FixedRestore:
        """The midpoint sigma and the middle quality: what validation scores, every epoch and every run."""
        q = 0 if self.jpeg_quality is None else round((self.jpeg_quality[0] + self.jpeg_quality[1]) / 2)
        return FixedRestore(0.5 * (self.sigma[0] + self.sigma[1]), q, self.gray_noise_p >= 0.5, self.subsample)
