"""The NIQE stages of csrc/niqe.hip -- srk_niqe_plane_f32, srk_niqe_half_f32, srk_niqe_mscn_f32, srk_niqe_moments_f32 -- one by one against
tests/niqe_ref.py, then metrics.niqe end to end and predict --niqe.  Inputs and outputs of the direct calls sit between the NaN guard rows
of tests/guarded.py: a read outside an input reaches the output as a NaN, a write outside an output changes a guard row."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import niqe_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3
U = 2.0 ** -24
# bs, H, W, border, B, C: one block with a crop remainder on both axes | 2 x 3 blocks behind a border | single channel, 2 x 3 blocks of 16
# | bs / 2 = 6 (no power of two), odd extents
CASES = [(96, 197, 113, 0, 1, 3), (96, 200, 296, 4, 2, 3), (16, 40, 56, 0, 3, 1), (12, 31, 50, 3, 2, 3)]
CONTENTS = ["uniform", "smooth"]
PARAMS = [(c, k) for c in CASES for k in CONTENTS]
IDS = ["-".join(str(v) for v in c) + "-" + k for c, k in PARAMS]


def _L():
    from tpu_superresolution_amd import _lib
    return _lib.lib()


def _stream():
    from tpu_superresolution_amd import ops
    return ops._stream()


def _w32():
    return R.window().astype(np.float32)


@functools.lru_cache(maxsize=None)
def _input(case, content):
    bs, H, W, border, B, C = case
    rng = np.random.RandomState(H * 7 + W + len(content))
    if content == "uniform":
        x = rng.rand(B, C, H, W)
    else:
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        field = 0.5 + 0.3 * np.sin(xx / 17.0 + np.arange(C)[:, None, None]) * np.cos(yy / 23.0)
        x = field[None] + rng.standard_normal((B, C, H, W)) / 255.0
    if content == "flat":          # the (16, 40, 56, 0, 3, 1) case with an exactly flat 20 x 20 patch
        x = rng.rand(B, C, H, W)
        x[:, :, 10:30, 20:40] = 0.5
    return x.astype(np.float32)


def _guarded_in(a):
    """An input [rows, cols] in a guarded buffer: NaN rows before and after it."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    a2 = a.reshape(-1, a.shape[-1])
    return Guarded("f32", a2.shape[0], a2.shape[1], a2.shape[1], fill=torch.from_numpy(a2))


def _check(rc):
    from tpu_superresolution_amd._lib import check
    check(rc)


def _run_plane(x, border, bs):
    B, C, H, W = x.shape
    Hk, Wk = (H - 2 * border) // bs * bs, (W - 2 * border) // bs * bs
    gin, out = _guarded_in(x), Guarded("f32", B * Hk, Wk, Wk)
    _check(_L().srk_niqe_plane_f32(gin.ptr, out.ptr, B, C, H, W, border, bs, _stream()))
    torch.cuda.synchronize()
    out.assert_guards("plane")
    gin.assert_untouched("x")
    return out.data().view(B, Hk, Wk)


def _run_half(plane):
    B, H, W = plane.shape
    gin, out = _guarded_in(plane.numpy()), Guarded("f32", B * H // 2, W // 2, W // 2)
    _check(_L().srk_niqe_half_f32(gin.ptr, out.ptr, B, H, W, _stream()))
    torch.cuda.synchronize()
    out.assert_guards("half")
    return out.data().view(B, H // 2, W // 2)


def _run_mscn(plane, want_sigma=True):
    B, H, W = plane.shape
    gin, gw = _guarded_in(plane.numpy()), _guarded_in(_w32().reshape(1, 49))
    m, sg = Guarded("f32", B * H, W, W), Guarded("f32", B * H, W, W)
    _check(_L().srk_niqe_mscn_f32(gin.ptr, gw.ptr, m.ptr, sg.ptr if want_sigma else None, B, H, W, _stream()))
    torch.cuda.synchronize()
    m.assert_guards("mscn")
    if want_sigma:
        sg.assert_guards("sigma")
    else:
        sg.assert_untouched("sigma")
    return m.data().view(B, H, W), (sg.data().view(B, H, W) if want_sigma else None)


def _run_moments(m, sigma, bs):
    B, H, W = m.shape
    nb = (H // bs) * (W // bs)
    gm, gs = _guarded_in(m.numpy()), (_guarded_in(sigma.numpy()) if sigma is not None else None)
    mom, sharp = Guarded("f32", B * nb, 25, 25), Guarded("f32", 1, B * nb, B * nb)
    _check(_L().srk_niqe_moments_f32(gm.ptr, gs.ptr if gs else None, mom.ptr, sharp.ptr if gs else None, B, H, W, bs, _stream()))
    torch.cuda.synchronize()
    mom.assert_guards("mom")
    if gs:
        sharp.assert_guards("sharp")
    else:
        sharp.assert_untouched("sharp")
    return mom.data().view(B, nb, 5, 5), (sharp.data().view(B, nb) if gs else None)


@functools.lru_cache(maxsize=None)
def _stages(case, content):
    """Every stage of one case on the device, once; the tests read (and do not change) the results."""
    bs, H, W, border, B, C = case
    plane = _run_plane(_input(case, content), border, bs)
    half = _run_half(plane)
    m1, s1 = _run_mscn(plane)
    m2, _ = _run_mscn(half, want_sigma=False)
    mom1, sharp = _run_moments(m1, s1, bs)
    mom2, _ = _run_moments(m2, None, bs // 2)
    return dict(plane=plane, half=half, m1=m1, s1=s1, m2=m2, mom1=mom1, sharp=sharp, mom2=mom2)


# ---- plane, half -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,content", PARAMS, ids=IDS)
def test_plane_equals_the_fp32_restatement(case, content):
    bs, H, W, border, B, C = case
    got = _stages(case, content)["plane"]
    want = torch.from_numpy(R.plane_f32(_input(case, content), border, bs))
    assert got.shape == want.shape and torch.equal(got, want)
    assert float(got.min()) >= 0 and float(got.max()) <= 255 and torch.equal(got, got.round())


@pytest.mark.parametrize("case,content", PARAMS, ids=IDS)
def test_half_equals_the_fp64_restatement_cast_to_fp32(case, content):
    s = _stages(case, content)
    want = torch.from_numpy(R.half_ref(s["plane"].numpy()).astype(np.float32))
    assert torch.equal(s["half"], want)


# ---- MSCN ------------------------------------------------------------------------------------------------------------------------------
def _mscn_check(v, m_dev, s_dev, what):
    """Bound (tests/niqe_ref.py::mscn_bounds): a = sum w d and b = sum w d^2 are 49-term fmaf sums of exact d, d^2 with the fp32 taps:
    |da| <= 2 K u Sa, |db| <= 2 K u Sb, K = 49, u = 2^-24, Sa / Sb the sums of the absolute terms; through t = b - a^2 (two roundings),
    sqrt|t| (|d sqrt| <= min(sqrt(dt), dt / sigma), one rounding) and m = -a / (sigma + 1) (two roundings).  The centred fp64 reference
    uses the device's fp32 taps.  The naive fp64 form needs sum w = 1 to mean the same thing, so it takes the fp32 taps divided by their
    fp64 sum s; that rescales a and b by 1 / s: |1 - s| Sa and |1 - s| Sb join the bound, with the naive form's own fp64 rounding
    (49 terms of at most 255 w, 255^2 w at 2^-53: 49 2^-52 255 and 49 2^-52 255^2, and 2^-52 255^2 more for mu^2).
    -> worst error / bound over both references."""
    w32 = _w32().astype(np.float64)
    s = w32.sum()
    worst = 0.0
    for b in range(v.shape[0]):
        m, sg, a, Sa, Sb = R.mscn_centred(v[b], w32)
        ds, dm = R.mscn_bounds(sg, a, Sa, Sb)
        em, es = np.abs(m_dev[b].astype(np.float64) - m), np.abs(s_dev[b].astype(np.float64) - sg) if s_dev is not None else None
        assert np.all(em <= dm), f"{what}[{b}]: centred m error / bound max {np.max(em / dm):.3f} at {np.unravel_index(np.argmax(em / dm), em.shape)}"
        worst = max(worst, float(np.max(em / dm)))
        if es is not None:
            assert np.all(es <= ds), f"{what}[{b}]: sigma error / bound max {np.max(es / ds):.3f}"
            worst = max(worst, float(np.max(es / np.maximum(ds, 1e-300))))
        mn, _ = R.mscn_naive(v[b], w32.reshape(7, 7) / s)
        _, dmn = R.mscn_bounds(sg, a, Sa, Sb, da_extra=abs(1 - s) * Sa + 49 * 2.0 ** -52 * 255, db_extra=abs(1 - s) * Sb + 50 * 2.0 ** -52 * 255 ** 2)
        en = np.abs(m_dev[b].astype(np.float64) - mn)
        assert np.all(en <= dmn), f"{what}[{b}]: naive m error / bound max {np.max(en / dmn):.3f}"
        worst = max(worst, float(np.max(en / dmn)))
    return worst


@pytest.mark.parametrize("case,content", PARAMS, ids=IDS)
def test_mscn_is_within_the_derived_bound_of_the_fp64_forms(case, content):
    s = _stages(case, content)
    r1 = _mscn_check(s["plane"].numpy(), s["m1"].numpy(), s["s1"].numpy(), "scale 1")
    r2 = _mscn_check(s["half"].numpy(), s["m2"].numpy(), None, "scale 2")
    print(f"MSCN worst error / bound: scale 1 {r1:.4f}, scale 2 {r2:.4f}")


# ---- moments ---------------------------------------------------------------------------------------------------------------------------
def _moments_ref(m, bs):
    """From an fp32 map [B, H, W] (the device's own): products as ONE fp32 multiply; -> counts (exact), fp64 sums [B, nb, 5, 5]."""
    B, H, W = m.shape
    nbh, nbw = H // bs, W // bs
    out = np.zeros((B, nbh * nbw, 5, 5))
    for b in range(B):
        for i in range(nbh):
            for j in range(nbw):
                blk = m[b, i * bs:(i + 1) * bs, j * bs:(j + 1) * bs]
                for k, p in enumerate([blk] + [(blk * np.roll(blk, sh, axis=(0, 1))).astype(np.float32) for sh in R.SHIFTS]):
                    p = p.astype(np.float64)
                    out[b, i * nbw + j, k] = [(p < 0).sum(), (p[p < 0] ** 2).sum(), (p > 0).sum(), (p[p > 0] ** 2).sum(), np.abs(p).sum()]
    return out


def _moments_check(mom, m, bs, exact=False):
    """Counts equal; the three sums within 2 n u S, n the block's pixel count and S the sum of the (non-negative) terms itself."""
    ref = _moments_ref(m.numpy(), bs)
    got = mom.numpy().astype(np.float64)
    assert np.array_equal(got[..., [0, 2]], ref[..., [0, 2]]), "counts differ"
    n = bs * bs
    for col in (1, 3, 4):
        err, bound = np.abs(got[..., col] - ref[..., col]), 2 * n * U * ref[..., col]
        assert np.all(err <= bound), f"sum {col}: error / bound max {np.max(err / np.maximum(bound, 1e-300)):.3f}"
        if exact:
            assert np.array_equal(got[..., col], ref[..., col])
    return ref


@pytest.mark.parametrize("case,content", PARAMS, ids=IDS)
def test_moments_against_the_devices_own_map(case, content):
    bs = case[0]
    s = _stages(case, content)
    _moments_check(s["mom1"], s["m1"], bs)
    _moments_check(s["mom2"], s["m2"], bs // 2)
    B, H, W = s["s1"].shape
    want = s["s1"].numpy().astype(np.float64).reshape(B, H // bs, bs, W // bs, bs).transpose(0, 1, 3, 2, 4).reshape(B, -1, bs * bs).mean(-1)
    err = np.abs(s["sharp"].numpy().astype(np.float64) - want)
    assert np.all(err <= (2 * bs * bs + 1) * U * want)


def test_two_runs_give_equal_bits():
    case = CASES[1]
    s = _stages(case, "smooth")
    mom1, sharp = _run_moments(s["m1"], s["s1"], case[0])
    mom2, _ = _run_moments(s["m2"], None, case[0] // 2)
    assert torch.equal(mom1, s["mom1"]) and torch.equal(sharp, s["sharp"]) and torch.equal(mom2, s["mom2"])


def test_moments_of_small_dyadic_values_are_exact_whatever_the_order():
    rng = np.random.RandomState(5)
    m = torch.from_numpy((rng.randint(-4, 5, size=(2, 96, 192)) / 8.0).astype(np.float32))
    sg = torch.from_numpy((rng.randint(0, 9, size=(2, 96, 192)) / 4.0).astype(np.float32))
    mom, sharp = _run_moments(m, sg, 96)
    _moments_check(mom, m, 96, exact=True)
    want = sg.numpy().astype(np.float64).reshape(2, 1, 96, 2, 96).transpose(0, 1, 3, 2, 4).reshape(2, 2, -1).mean(-1)
    assert np.array_equal(sharp.numpy(), want.astype(np.float32))
    mom6, _ = _run_moments(m[:, :90, :186].contiguous(), None, 6)          # 15 x 31 blocks of 6 x 6: fewer pixels than threads
    _moments_check(mom6, m[:, :90, :186], 6, exact=True)


def test_flat_neighbourhoods_give_exact_zeros_that_count_on_neither_side():
    case = (16, 40, 56, 0, 3, 1)
    s = _stages(case, "flat")
    assert torch.equal(s["plane"][:, 10:30, 20:40], torch.full((3, 20, 20), 128.0))
    inner = s["m1"][:, 13:27, 23:37]
    assert torch.equal(inner, torch.zeros_like(inner)) and torch.equal(s["s1"][:, 13:27, 23:37], torch.zeros_like(inner))
    ref = _moments_check(s["mom1"], s["m1"], 16)
    nz = int((s["m1"][:, 16:32, 32:48] == 0).sum(dim=(1, 2))[0])          # block (1, 2) lies in rows 16..32, columns 32..48
    assert nz >= 11 * 5 and ref[0, 1 * 3 + 2, 0, 0] + ref[0, 1 * 3 + 2, 0, 2] == 256 - nz
    _mscn_check(s["plane"].numpy(), s["m1"].numpy(), s["s1"].numpy(), "flat")


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
# |device score - fp64 reference score| measured on the MI355X for the seven images of tests/niqe_ref.py::suite: the gate is
# four times the largest, the margin for the one-grid-step jitter of alpha when another image is used.
E2E_MEASURED_MAX = 5.498e-05          # blur1.5; the others: 8.1e-6 clean, 4.9e-6 / 8.8e-7 / 4.7e-5 noise, 2.7e-5 / 5.2e-5 blur 0.8 / 3
E2E_CEILING = 5e-3          # above this the feature fails its purpose: half a unit of the second decimal the papers print


def test_end_to_end_scores_against_the_fp64_restatement():
    from tpu_superresolution_amd import metrics
    from tpu_superresolution_amd.niqe import niqe_moments
    S = R.suite()
    names = list(S["images"])
    x = torch.from_numpy(np.concatenate([S["images"][k] for k in names])).cuda()
    params = (S["mu"], S["cov"], R.window())
    got = metrics.niqe(x, params).numpy()
    dev = {k: abs(got[i] - S["scores"][k]) for i, k in enumerate(names)}
    print("end-to-end |device - fp64 reference|:", {k: f"{v:.3e}" for k, v in dev.items()}, "scores", {k: round(S["scores"][k], 3) for k in names})
    mom1, mom2, _ = niqe_moments(x, 0, 96, R.window())
    for i, k in enumerate(names):          # the host fp64 chain of the package against the restatement's, on the same downloaded moments
        rows = np.concatenate([R.features_from_moments(mom1[i], 96 * 96), R.features_from_moments(mom2[i], 48 * 48)], axis=1)
        want = R.distance(rows, S["mu"], S["cov"])
        assert abs(got[i] - want) <= 1e-12 * max(1.0, want), (k, got[i], want)
    assert max(dev.values()) <= E2E_CEILING
    assert E2E_MEASURED_MAX is not None and max(dev.values()) <= 4 * E2E_MEASURED_MAX


def test_fit_on_the_device_gives_the_cpu_fit():
    from tpu_superresolution_amd import metrics
    S = R.suite()
    mu, cov = metrics.niqe_fit([torch.from_numpy(R.as_batch(R.pink_image(s))).cuda() for s in range(6)])
    assert np.abs(mu - S["mu"]).max() <= 2e-3 * np.abs(S["mu"]).max() and np.abs(cov - S["cov"]).max() <= 2e-2 * np.abs(S["cov"]).max()


# ---- predict --niqe ----------------------------------------------------------------------------------------------------------------------
def test_predict_niqe_scores_what_is_written_and_changes_nothing_else(tmp_path, capsys):
    from tpu_superresolution_amd import metrics
    from tpu_superresolution_amd import predict as P
    S = R.suite()
    metrics.save_niqe_params(tmp_path / "p.npz", S["mu"], S["cov"], R.window())
    src = tmp_path / "lq"
    src.mkdir()
    rng = np.random.RandomState(9)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, size=(100, 150, 3), dtype=np.uint8), mode="RGB").save(src / f"f{i}.png")

    def model(x):
        return torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")

    base = ["--input", str(src), "--arch", "swinir", "--scale", "X2", "--ckpt", "unused.pt", "--batch_size", "2"]
    plain = P.run(model, P.parse_args(base + ["--output", str(tmp_path / "a")]), 2, torch.device("cuda"))
    lines_plain = capsys.readouterr().out.splitlines()
    scored = P.run(model, P.parse_args(base + ["--output", str(tmp_path / "b"), "--niqe", str(tmp_path / "p.npz")]), 2, torch.device("cuda"))
    lines = capsys.readouterr().out.splitlines()
    assert "niqe" not in plain and not any("niqe" in ln for ln in lines_plain)
    for k in ("n", "groups", "clipped", "output_mp"):
        assert plain[k] == scored[k]
    params = metrics.load_niqe_params(tmp_path / "p.npz")
    for i in range(2):
        a, b = (tmp_path / "a" / f"f{i}_sr.png").read_bytes(), (tmp_path / "b" / f"f{i}_sr.png").read_bytes()
        assert a == b
        img = np.asarray(Image.open(tmp_path / "b" / f"f{i}_sr.png"))
        assert img.shape == (200, 300, 3)
        x = torch.from_numpy(img.astype(np.float32) / np.float32(255.0)).permute(2, 0, 1)[None].contiguous().cuda()
        want = float(metrics.niqe(x, params)[0])
        assert scored["niqe"]["scores"][f"f{i}.png"] == want
        assert f"[niqe] f{i}.png {want:.4f}" in lines
    assert scored["niqe"]["mean"] == float(np.mean(list(scored["niqe"]["scores"].values())))
    assert any(ln.startswith("[done] 2 images") and "niqe mean" in ln for ln in lines)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_a_launch_and_leaves_the_outputs_untouched():
    L, st = _L(), _stream()
    x, big = Guarded("f32", 3 * 200, 296, 296), Guarded("f32", 3 * 200, 296, 296)
    win = _guarded_in(_w32().reshape(1, 49))
    small = Guarded("f32", 64, 25, 25)
    xp, op, wp, sp = x.ptr, big.ptr, win.ptr, small.ptr
    calls = [
        # plane(x, plane, B, C, H, W, border, bs)
        (E_NULL, lambda: L.srk_niqe_plane_f32(None, op, 1, 3, 200, 296, 0, 96, st)),
        (E_NULL, lambda: L.srk_niqe_plane_f32(xp, None, 1, 3, 200, 296, 0, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 0, 3, 200, 296, 0, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 0, 296, 0, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 200, -1, 0, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 1, 2, 200, 296, 0, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 200, 296, -1, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 200, 296, 0, 95, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 200, 296, 0, 6, st)),
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, op, 70000, 3, 200, 296, 0, 96, st)),          # B does not fit the grid
        (E_SHAPE, lambda: L.srk_niqe_plane_f32(xp, xp + 4 * 296 * 10, 1, 3, 200, 296, 0, 96, st)),          # plane inside x
        (E_UNSUPPORTED, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 95, 296, 0, 96, st)),
        (E_UNSUPPORTED, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 200, 296, 53, 96, st)),          # the border leaves 94 rows
        (E_UNSUPPORTED, lambda: L.srk_niqe_plane_f32(xp, op, 1, 3, 200, 296, 150, 96, st)),         # the border leaves nothing
        # half(plane, half, B, H, W)
        (E_NULL, lambda: L.srk_niqe_half_f32(None, op, 1, 96, 96, st)),
        (E_NULL, lambda: L.srk_niqe_half_f32(xp, None, 1, 96, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_half_f32(xp, op, 0, 96, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_half_f32(xp, op, 1, 95, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_half_f32(xp, op, 1, 96, 97, st)),
        (E_SHAPE, lambda: L.srk_niqe_half_f32(xp, op, 1, 2, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_half_f32(xp, op, 1, 96, 0, st)),
        (E_SHAPE, lambda: L.srk_niqe_half_f32(xp, xp + 64, 1, 96, 96, st)),
        # mscn(plane, win49, mscn, sigma, B, H, W)
        (E_NULL, lambda: L.srk_niqe_mscn_f32(None, wp, op, None, 1, 96, 96, st)),
        (E_NULL, lambda: L.srk_niqe_mscn_f32(xp, None, op, None, 1, 96, 96, st)),
        (E_NULL, lambda: L.srk_niqe_mscn_f32(xp, wp, None, None, 1, 96, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_mscn_f32(xp, wp, op, None, 1, 0, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_mscn_f32(xp, wp, op, None, -2, 96, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_mscn_f32(xp, wp, xp, None, 1, 96, 96, st)),          # in place
        (E_SHAPE, lambda: L.srk_niqe_mscn_f32(xp, wp, op, op + 4 * 96, 1, 96, 96, st)),          # sigma inside mscn
        (E_SHAPE, lambda: L.srk_niqe_mscn_f32(xp, wp, op, xp, 1, 96, 96, st)),
        # moments(mscn, sigma, mom, sharp, B, H, W, bs)
        (E_NULL, lambda: L.srk_niqe_moments_f32(None, None, sp, None, 1, 96, 192, 96, st)),
        (E_NULL, lambda: L.srk_niqe_moments_f32(xp, None, None, None, 1, 96, 192, 96, st)),
        (E_NULL, lambda: L.srk_niqe_moments_f32(xp, op, sp, None, 1, 96, 192, 96, st)),          # sigma without sharp
        (E_NULL, lambda: L.srk_niqe_moments_f32(xp, None, sp, sp + 4 * 200, 1, 96, 192, 96, st)),          # sharp without sigma
        (E_SHAPE, lambda: L.srk_niqe_moments_f32(xp, None, sp, None, 0, 96, 192, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_moments_f32(xp, None, sp, None, 1, 96, 192, 3, st)),
        (E_SHAPE, lambda: L.srk_niqe_moments_f32(xp, None, sp, None, 1, 96, 192, 5000, st)),
        (E_SHAPE, lambda: L.srk_niqe_moments_f32(xp, None, sp, None, 1, 100, 192, 96, st)),          # H no multiple of bs
        (E_SHAPE, lambda: L.srk_niqe_moments_f32(xp, None, sp, None, 1, 96, 200, 96, st)),
        (E_SHAPE, lambda: L.srk_niqe_moments_f32(xp, None, xp + 64, None, 1, 96, 192, 96, st)),          # mom inside mscn
        (E_SHAPE, lambda: L.srk_niqe_moments_f32(xp, op, sp, sp + 4 * 10, 1, 96, 192, 96, st)),          # sharp inside mom
        (E_UNSUPPORTED, lambda: L.srk_niqe_moments_f32(xp, None, sp, None, 1, 95, 192, 96, st)),
        (E_UNSUPPORTED, lambda: L.srk_niqe_moments_f32(xp, None, sp, None, 1, 96, 50, 96, st)),
    ]
    for i, (code, call) in enumerate(calls):
        rc = call()
        assert rc == code, f"call {i}: returned {rc}, expected {code}: {L.srk_last_error().decode()}"
        assert L.srk_last_error().decode().startswith("niqe_")
    torch.cuda.synchronize()
    for g, what in ((x, "x"), (big, "the large output"), (small, "the small output"), (win, "the window")):
        g.assert_untouched(what)


def test_python_wrappers_refuse_with_value_errors():
    from tpu_superresolution_amd import metrics
    S = R.suite()
    params = (S["mu"], S["cov"], R.window())
    for shape, kw, msg in (((1, 3, 90, 200), {}, "holds no block"), ((1, 2, 96, 192), {}, "C 1 or 3"), ((1, 3, 96, 192), dict(bs=7), "block side"),
                           ((1, 3, 96, 192), dict(crop_border=-1), "crop border")):
        with pytest.raises(ValueError, match=msg):
            metrics.niqe(torch.zeros(shape, device="cuda"), params, **kw)
    with pytest.raises(ValueError, match="at least 2"):          # one block: no covariance
        metrics.niqe(torch.rand(1, 3, 100, 100, device="cuda"), params)
