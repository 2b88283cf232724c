"""The image file <-> tensor conventions without a GPU: tests/image_io_ref.py (the numpy restatement that tests/test_gpu_image_io.py
holds the kernels to) pinned against the package's existing host forms, the rounding rule pinned on every 8-bit level, the planted
specials and searched ties, negative controls, and the CPU branches of ops.image_unpack / ops.image_pack.  Every comparison of
samples is bit equality."""
import numpy as np
import pytest
import torch
from PIL import Image

import image_io_ref as R
from tpu_superresolution_amd import ops
from tpu_superresolution_amd.sr_datasets import clean_to_tensor, ensure_3ch, pil_to_tensor01

DTYPES = {8: np.uint8, 16: np.uint16}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _samples(bits, shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256 if bits == 8 else 65536, size=shape, dtype=np.uint32).astype(DTYPES[bits])
    a.reshape(-1)[:2] = (0, np.iinfo(DTYPES[bits]).max)          # both ends of the range are present
    return a


def _torch_samples(a):
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)


def _np_samples(t):
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def _values(shape, seed):
    """fp32 in about [-0.1, 1.1]: most values inside [0, 1], some clipped on either side."""
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)


# ---- unpack equals the existing host forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_unpack_equals_host_forms(bits, ch):
    a = _samples(bits, (2, 9, 7, ch), seed=10 * bits + ch)
    x3, al = R.unpack_ref(a, 3, want_alpha=True)
    x1, _ = R.unpack_ref(a, 1)
    assert (al is not None) == (ch in (2, 4))
    for b in range(a.shape[0]):
        colour = a[b, :, :, 0] if ch <= 2 else a[b, :, :, :3]          # what a decoder hands over once alpha is split off
        t = pil_to_tensor01(colour)                                     # it reads np.asarray(img): an array stands in for the PIL image
        assert np.array_equal(_bits(x3[b]), _bits(ensure_3ch(t).numpy()))
        assert np.array_equal(_bits(x1[b]), _bits(clean_to_tensor(colour, 1).numpy()))
        if ch >= 3:
            g = ops.to_gray(np.ascontiguousarray(a[b, :, :, :3]))
            assert np.array_equal(_bits(x1[b, 0]), _bits(g.astype(np.float32) / np.float32(255.0 if bits == 8 else 65535.0)))
        if al is not None:
            assert np.array_equal(_bits(al[b, 0]), _bits(pil_to_tensor01(a[b, :, :, ch - 1]).numpy()[0]))


def test_unpack_8bit_through_pil():
    """The same through real PIL images of the modes predict keeps."""
    a = _samples(8, (1, 6, 5, 4), seed=3)
    for mode, ch in (("L", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4)):
        img = Image.fromarray(a[0, :, :, 0] if ch == 1 else a[0, :, :, :ch], mode=mode)
        arr = np.asarray(img)
        arr = arr[None, :, :, None] if arr.ndim == 2 else arr[None]
        x3, _ = R.unpack_ref(arr, 3)
        want = ensure_3ch(pil_to_tensor01(img.convert("L") if ch == 2 else img.convert("RGB") if ch == 4 else img))
        if ch in (1, 3):
            assert np.array_equal(_bits(x3[0]), _bits(want.numpy()))
        else:          # PIL's own alpha drop keeps the colour samples
            assert np.array_equal(_bits(x3[0]), _bits(ensure_3ch(pil_to_tensor01(arr[0, :, :, 0] if ch == 2 else arr[0, :, :, :3])).numpy()))


# ---- pack: the rounding rule -----------------------------------------------------------------------------------------------------------
def _rint_rule(v, mx):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.float32(v) * np.float32(mx))
        r = np.where(v >= 1, mx, np.where(v > 0, r, 0))
    return r.astype(np.uint32)


@pytest.mark.parametrize("bits", [8, 16])
def test_pack_every_8bit_level_and_its_neighbours(bits):
    mx = 255 if bits == 8 else 65535
    k = np.arange(256, dtype=np.float32)
    centre = (k / np.float32(255.0)).astype(np.float32)
    v = np.concatenate([centre, np.nextafter(centre, np.float32(-1)), np.nextafter(centre, np.float32(2))]).astype(np.float32)
    out, _ = R.pack_ref(v.reshape(1, 1, 3, 256), bits=bits)
    assert np.array_equal(out.reshape(-1).astype(np.uint32), _rint_rule(v, mx))
    if bits == 8:          # k / 255 decodes back to k: what a file written by pack reads as
        assert np.array_equal(out.reshape(3, 256)[0], np.arange(256))


@pytest.mark.parametrize("bits", [8, 16])
def test_pack_specials(bits):
    mx = 255 if bits == 8 else 65535
    sp = R.specials()
    out, (nf, cl) = R.pack_ref(sp.reshape(1, 1, 1, -1), bits=bits)
    assert out.reshape(-1).tolist() == [0, mx, 0, 0, mx, 0, 0, mx]          # NaN +Inf -Inf -0.0 1+ulp -ulp 0 1
    assert (nf, cl) == (3, 2)                                                # -0.0, 0 and 1 are inside [0, 1]
    assert np.array_equal(out.reshape(-1).astype(np.uint32), _rint_rule(sp, mx))


@pytest.mark.parametrize("bits", [8, 16])
def test_pack_ties_round_to_even(bits):
    mx = np.float32(255.0 if bits == 8 else 65535.0)
    v, k = R.ties(bits)
    assert len(v) > 0 and (k % 2 == 0).any(), "the search found no tie with an even k: the test would be vacuous"
    assert np.array_equal((v * mx).astype(np.float32), (k + 0.5).astype(np.float32))          # the fp32 product IS k + 0.5
    out, _ = R.pack_ref(v.reshape(1, 1, 1, -1), bits=bits)
    want = np.where(k % 2 == 0, k, k + 1)
    assert np.array_equal(out.reshape(-1).astype(np.int64), want)
    # the controls differ exactly where they should
    up, _ = R.pack_ref(v.reshape(1, 1, 1, -1), bits=bits, variant="half_up")
    assert np.array_equal(up.reshape(-1).astype(np.int64), k + 1) and (up != out).any()
    tr, _ = R.pack_ref(v.reshape(1, 1, 1, -1), bits=bits, variant="trunc")
    assert np.array_equal(tr.reshape(-1).astype(np.int64), k) and (tr != out).any()


def test_counters_exact():
    y = _values((2, 3, 5, 7), seed=1)
    a = _values((2, 1, 5, 7), seed=2)
    y.reshape(-1)[[0, 11, 50]] = (np.nan, np.inf, -np.inf)
    a.reshape(-1)[[3]] = np.nan
    want_nf = 4
    want_cl = int(((y < 0) | (y > 1)).sum() + ((a < 0) | (a > 1)).sum()) - 2          # the two infinities compare outside but are not finite
    with np.errstate(invalid="ignore"):
        _, (nf, cl) = R.pack_ref(y, a, out_chans=4)
    assert (nf, cl) == (want_nf, want_cl) and cl > 0
    _, (nf3, cl3) = R.pack_ref(y, a, out_chans=3)                                       # alpha is not written: not counted
    assert nf3 == 3 and cl3 < cl


# ---- negative controls: each wrong convention changes at least one sample on these inputs ----------------------------------------------
def test_negative_controls_pack():
    y = _values((2, 3, 6, 9), seed=5)
    a = _values((2, 1, 6, 9), seed=6)
    for bits in (8, 16):
        ref4, _ = R.pack_ref(y, a, out_chans=4, bits=bits)
        ref1, _ = R.pack_ref(y, out_chans=1, bits=bits)
        for variant, oc in (("trunc", 4), ("half_up", 4), ("swap_rb", 4), ("no_alpha", 4), ("luma_first", 1)):
            if variant == "half_up":          # random values meet no tie: use the searched ones
                v, _ = R.ties(bits)
                got, _ = R.pack_ref(v.reshape(1, 1, 1, -1), bits=bits, variant=variant)
                want, _ = R.pack_ref(v.reshape(1, 1, 1, -1), bits=bits)
            else:
                got, _ = R.pack_ref(y, a if oc == 4 else None, out_chans=oc, bits=bits, variant=variant)
                want = ref4 if oc == 4 else ref1
            assert got.shape == want.shape and (got != want).any(), f"control '{variant}' at {bits} bits changed nothing"


def test_negative_controls_unpack():
    for bits in (8, 16):
        a4, a2 = _samples(bits, (1, 5, 6, 4), seed=7), _samples(bits, (1, 5, 6, 2), seed=8)
        x, al = R.unpack_ref(a4, 3, want_alpha=True)
        xs, _ = R.unpack_ref(a4, 3, variant="swap_rb")
        assert (_bits(x) != _bits(xs)).any()
        g, ga = R.unpack_ref(a2, 1, want_alpha=True)
        gs, gsa = R.unpack_ref(a2, 1, want_alpha=True, variant="alpha_slot0")
        assert (_bits(g) != _bits(gs)).any() and (_bits(ga) != _bits(gsa)).any()
        assert R.unpack_ref(a4, 3, want_alpha=False)[1] is None and al is not None          # alpha dropped only when not asked for
        assert (_bits(al) != _bits(np.ones_like(al))).any()


# ---- the CPU branches of the ops equal the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("oc", [1, 3])
def test_ops_unpack_cpu_equals_ref(bits, ch, oc):
    a = _samples(bits, (2, 5, 7, ch), seed=100 + 10 * ch + oc + bits)
    for want_alpha in (False, True):
        x, al = ops.image_unpack(_torch_samples(a), oc, want_alpha=want_alpha)
        rx, ral = R.unpack_ref(a, oc, want_alpha=want_alpha)
        assert x.dtype == torch.float32 and tuple(x.shape) == rx.shape and np.array_equal(_bits(x.numpy()), _bits(rx))
        assert (al is None) == (ral is None)
        if al is not None:
            assert tuple(al.shape) == ral.shape and np.array_equal(_bits(al.numpy()), _bits(ral))


def test_ops_unpack_cpu_single_image_shapes():
    a = _samples(8, (4, 6, 3), seed=2)
    x, _ = ops.image_unpack(torch.from_numpy(a), 3)
    assert np.array_equal(_bits(x.numpy()), _bits(R.unpack_ref(a[None], 3)[0]))
    g, _ = ops.image_unpack(torch.from_numpy(a[:, :, 0].copy()), 1)
    assert tuple(g.shape) == (1, 1, 4, 6) and np.array_equal(_bits(g.numpy()), _bits(R.unpack_ref(a[None, :, :, :1], 1)[0]))


def _planted(C, bits, seed):
    y = _values((2, C, 6, 11), seed=seed)
    sp = R.specials()
    tv, _ = R.ties(bits, limit=16)
    flat = y.reshape(-1)
    flat[:len(sp)] = sp
    flat[20:20 + len(tv)] = tv
    return y


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("oc", [1, 2, 3, 4])
def test_ops_pack_cpu_equals_ref(bits, C, oc):
    y = _planted(C, bits, seed=200 + 10 * C + oc + bits)
    a = _planted(1, bits, seed=300 + oc) if oc in (2, 4) else None
    counters = torch.tensor([5, 7], dtype=torch.int32)
    out = ops.image_pack(torch.from_numpy(y), None if a is None else torch.from_numpy(a), out_chans=oc, bits=bits, counters=counters)
    ref, (nf, cl) = R.pack_ref(y, a, out_chans=oc, bits=bits)
    assert out.dtype == (torch.uint8 if bits == 8 else torch.uint16) and tuple(out.shape) == ref.shape
    assert np.array_equal(_np_samples(out), ref)
    assert counters.tolist() == [5 + nf, 7 + cl] and nf >= 3          # accumulated, not overwritten
    one = ops.image_pack(torch.from_numpy(y[0]), None if a is None else torch.from_numpy(a[0]), out_chans=oc, bits=bits)
    assert np.array_equal(_np_samples(one), ref[0])


def test_ops_pack_default_out_chans():
    y, a = torch.rand(1, 3, 4, 5), torch.rand(1, 1, 4, 5)
    assert ops.image_pack(y).shape[-1] == 3 and ops.image_pack(y, a).shape[-1] == 4
    assert ops.image_pack(y[:, :1]).shape[-1] == 1 and ops.image_pack(y[:, :1], a).shape[-1] == 2


def test_ops_argument_errors_are_value_errors(monkeypatch):
    from tpu_superresolution_amd import image_ops

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(image_ops, "lib", no_lib)
    u8 = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    for bad in (lambda: ops.image_unpack(u8.float(), 3), lambda: ops.image_unpack(u8, 2), lambda: ops.image_unpack(torch.zeros((1, 4, 4, 5), dtype=torch.uint8), 3),
                lambda: ops.image_unpack(torch.zeros((1, 0, 4, 3), dtype=torch.uint8), 3), lambda: ops.image_unpack(u8[None], 3)):
        with pytest.raises(ValueError):
            bad()
    y = torch.zeros((1, 3, 4, 4))
    for bad in (lambda: ops.image_pack(y.double()), lambda: ops.image_pack(y[:, :2]), lambda: ops.image_pack(y, out_chans=5),
                lambda: ops.image_pack(y, out_chans=4), lambda: ops.image_pack(y, bits=12), lambda: ops.image_pack(y, torch.zeros((1, 1, 4, 5))),
                lambda: ops.image_pack(y, counters=torch.zeros(2)), lambda: ops.image_pack(y[0, 0])):
        with pytest.raises(ValueError):
            bad()
