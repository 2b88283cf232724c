"""A second, independent statement of the device-built tables (include/srk.h "Blur and sinc tables built on the device";
csrc/tables.hip) and the bound its GPU test holds the kernel to.  Plain Python `math`, no numpy arithmetic: `restate` evaluates the
eight doubles of `TableDesc.row()` the way srk.h words it -- q = (A x^2 + B2 x y) + C y^2, a sequential row-major sum, one division and
one rounding per tap, J1 by the 512-interval trapezoid rule summed in ascending order ONCE per distinct x^2 + y^2.  The GPU test compares
the kernel with the HOST tables (blur_kernels), not with this; this file's job is the bound, and showing that the bound is not slack:
`restate(..., fault=...)` makes the mistakes a kernel could make, and tests/test_tables_ref.py checks that the bound catches them (all but the
reciprocal multiply, which moves a tap by at most the one fp32 spacing that the bound has to admit: that one is shown in fp64).

The bound, per tap:   |dev - host| <= spacing32(host) + [kind 4] 2^-36 max|host table|
with spacing32(v) the distance from |v| to the next fp32 above it (2^-149 at and below the denormals).

Derivation.  Both sides compute e / S in fp64 and round ONCE to fp32, so they differ by at most one fp32 spacing provided the fp64
quotients differ by less than half a spacing, i.e. agree to a relative ~2^-25 (in the denormal range: an absolute 2^-150).
  Kinds 1-3.  q is bit-identical (the host forms A, B2, C; x^2, x y, y^2 are exact integers; same three products and two sums, no
    contraction).  exp, pow are accurate to a few ulp (2^-52 relative) in either libm.  In exp(-0.5 q^beta) an input error is amplified
    by |0.5 q^beta| for exp and by beta for pow: at most |0.5 q^beta| beta.  A tap that survives fp32 at all has e / S >= 2^-150 with
    S >= 1 (the centre tap is 1), so 0.5 q^beta < 150 ln 2 = 104, and beta <= 16: the relative error of e stays below
    104 * 16 * 2^-50 < 2^-39, in practice (beta <= 4) near 2^-44.  The plateau 1 / (q^beta + 1) amplifies by at most beta.  S is a
    sum of <= 441 non-negative terms: any summation order is within 441 * 2^-53 < 2^-44 relative.  Together far below 2^-25: the two
    fp32 roundings land on the same or on adjacent values, never further.  Hence spacing32(host), and nothing more.
  Kind 4.  J1 is a sum of 513 cosines of magnitude <= 1 at arguments below 48 (|z| <= 10 sqrt(2) pi < 45, plus t <= pi): each term is
    within a few ulp of 64 (2^-46) in absolute terms whatever the libm, argument rounding included, and 513 of them in any order stay
    below 513 * 2^-45 / 512 < 2^-43 absolute after the division by 512.  The tap multiplies J1 by cutoff / (2 pi r) <= 0.5 (cutoff <= pi,
    r >= 1): below 2^-44 absolute in e.  Off-centre taps pass through zero, so there the error is NOT relative to the tap; it is
    relative to the table's maximum, the centre tap cutoff^2 / (4 pi) >= (pi / 5)^2 / (4 pi) = 0.0314 > 2^-5: 2^-44 / 2^-5 = 2^-39
    of max|table| (S is within a relative 2^-40 of the host's by the same count and moves every tap by that fraction of itself).  The
    bound allows 2^-36: a factor of 8 over the worst case, and still 2^11 below the fp32 spacing of the maximum, so it admits no
    real defect -- 16 quadrature intervals miss it by ten orders of magnitude.
Re-derive this if the rule changes; never tune it to an observed figure."""
import math

import numpy as np

J1_N = 512


def spacing32(host):
    """The distance from |v| to the next fp32 above, as fp64: 2^-149 for zero and the denormals."""
    return np.spacing(np.abs(np.asarray(host, dtype=np.float32))).astype(np.float64)


def bound(host, kind):
    """The per-tap bound of the module docstring for one host table (fp32 [ks][ks]) of the given kind."""
    h = np.asarray(host, dtype=np.float32)
    extra = 2.0 ** -36 * float(np.abs(h).max()) if int(kind) == 4 else 0.0
    return spacing32(h) + extra


def within(dev, host, kind):
    """-> (every tap is inside the bound, the number of taps whose words differ at all)."""
    d, h = np.asarray(dev, dtype=np.float32), np.asarray(host, dtype=np.float32)
    err = np.abs(d.astype(np.float64) - h.astype(np.float64))
    ok = bool((err <= bound(h, kind)).all()) and not bool(np.isnan(err).any())
    return ok, int((d.view(np.uint32) != h.view(np.uint32)).sum())


def _j1(z, n=J1_N):
    acc = 0.0
    for j in range(1, n):
        t = j * (math.pi / n)
        acc += math.cos(t - z * math.sin(t))
    ends = math.cos(0.0 - z * math.sin(0.0)) + math.cos(math.pi - z * math.sin(math.pi))
    return (acc + 0.5 * ends) / n


def _f32(v, ftz=False):
    f = np.float32(v)
    if ftz and f != 0 and abs(float(f)) < 2.0 ** -126:
        return np.float32(0.0)
    return f


FAULTS = (None, "recip", "j1_16", "ftz", "transpose", "uncentred")


def restate(row, ks, bank=None, fault=None, as_f64=False):
    """The fp32 [ks][ks] table of one descriptor row (kind, ks_own, A, B2, C, beta, cutoff, bank_index), by srk.h's wording.
    fault: one deliberate mistake -- 'recip' multiplies by 1 / S instead of dividing, 'j1_16' takes 16 quadrature intervals, 'ftz'
    flushes fp32 denormal results, 'transpose' swaps x and y, 'uncentred' pads at the top left.  as_f64 (kinds 1-4): the fp64 quotients
    before the rounding instead, [ks][ks] fp64."""
    assert fault in FAULTS, fault
    kind, own = int(row[0]), int(row[1])
    A, B2, C, beta, cutoff = (float(v) for v in row[2:7])
    out = np.zeros((ks, ks), dtype=np.float32)
    pad = 0 if fault == "uncentred" else (ks - own) // 2
    R = (own - 1) // 2
    if kind == 0:
        out[pad + R, pad + R] = 1.0
        return out
    if kind == 5:
        src = np.asarray(bank[int(row[7])], dtype=np.float32)
        pad = 0 if fault == "uncentred" else (ks - src.shape[0]) // 2
        out.view(np.uint32)[pad:pad + src.shape[0], pad:pad + src.shape[0]] = src.view(np.uint32)
        return out
    j1_by_d2 = {}
    e = []
    for a in range(own):
        for b in range(own):
            y, x = a - R, b - R
            if fault == "transpose":
                x, y = y, x
            if kind == 4:
                d2 = x * x + y * y
                if d2 == 0:
                    e.append(cutoff * cutoff / (4.0 * math.pi))
                    continue
                if d2 not in j1_by_d2:
                    j1_by_d2[d2] = _j1(cutoff * math.sqrt(float(d2)), 16 if fault == "j1_16" else J1_N)
                e.append(cutoff * j1_by_d2[d2] / (2.0 * math.pi * math.sqrt(float(d2))))
                continue
            q = (A * float(x * x) + B2 * float(x * y)) + C * float(y * y)
            if kind == 1:
                e.append(math.exp(-0.5 * q))
            elif kind == 2:
                e.append(math.exp(-0.5 * math.pow(q, beta)))
            else:
                e.append(1.0 / (math.pow(q, beta) + 1.0))
    S = 0.0
    for v in e:
        S += v
    inv = 1.0 / S
    if as_f64:
        out = np.zeros((ks, ks), dtype=np.float64)
    for i, v in enumerate(e):
        t = v * inv if fault == "recip" else v / S
        out[pad + i // own, pad + i % own] = t if as_f64 else _f32(t, ftz=fault == "ftz")
    return out
