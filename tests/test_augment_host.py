"""D4 augmentation and self-ensemble, host side (tpu_superresolution_amd/augment.py): the op-code algebra against an explicit index
permutation, the draw order of the paired train transform, the two command lines, and the argument checks of srk_dihedral_f32 that
return before any launch.  The kernel itself: tests/test_gpu_dihedral.py."""
import ctypes as C
import random

import numpy as np
import pytest
import torch
from PIL import Image

from tpu_superresolution_amd import augment as A


def permute_numpy(a, k):
    """T_k = Tr^b2 . V^b1 . H^b0 written as an index map on the last two axes, one element at a time."""
    H, W = a.shape[-2:]
    out = np.empty(a.shape[:-2] + ((W, H) if k & 4 else (H, W)), a.dtype)
    for y in range(H):
        for x in range(W):
            xf = W - 1 - x if k & 1 else x          # H: the element at x lands at W-1-x
            yf = H - 1 - y if k & 2 else y
            if k & 4:
                out[..., xf, yf] = a[..., y, x]
            else:
                out[..., yf, xf] = a[..., y, x]
    return out


@pytest.mark.parametrize("k", range(8))
def test_apply_op_host_is_the_specified_permutation(k):
    t = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    got = A.apply_op_host(t, k)
    assert got.is_contiguous() and torch.equal(got, torch.from_numpy(permute_numpy(t.numpy(), k)))
    assert tuple(got.shape) == ((2, 3, 7, 5) if k & 4 else (2, 3, 5, 7))


@pytest.mark.parametrize("k", range(8))
def test_inverse_op_undoes_the_op(k):
    t = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    inv = A.inverse_op(k)
    assert 0 <= inv <= 7 and A.inverse_op(inv) == k
    assert torch.equal(A.apply_op_host(A.apply_op_host(t, k), inv), t)
    assert inv == (k if k < 4 else 4 | ((k & 1) << 1) | ((k >> 1) & 1))


def test_the_eight_transforms_are_pairwise_distinct_and_codes_are_checked():
    t = torch.arange(16, dtype=torch.float32).reshape(1, 4, 4)          # no symmetry: every transform moves some element
    imgs = [A.apply_op_host(t, k) for k in range(8)]
    assert A.apply_op_host(t, 0) is t
    for i in range(8):
        for j in range(i + 1, 8):
            assert not torch.equal(imgs[i], imgs[j]), (i, j)
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="0..7"):
            A.apply_op_host(t, bad)
        with pytest.raises(ValueError, match="0..7"):
            A.inverse_op(bad)


def test_draw_op_modes_and_random_consumption():
    random.seed(5)
    state = random.getstate()
    assert A.draw_op("none") == 0 and random.getstate() == state          # no generator call at all
    random.seed(5)
    want4, want8 = random.randrange(4), random.randrange(8)
    random.seed(5)
    assert A.draw_op("flip") == want4 and A.draw_op("d4") == want8
    random.seed(0)
    assert {A.draw_op("flip") for _ in range(200)} == {0, 1, 2, 3}
    assert {A.draw_op("d4") for _ in range(400)} == set(range(8))
    with pytest.raises(ValueError, match="augment must be one of"):
        A.draw_op("rot")


def _pil_pair(scale=2, h=20, w=27, seed=0):
    rng = np.random.default_rng(seed)
    return (Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
            Image.fromarray(rng.integers(0, 256, (h * scale, w * scale, 3), dtype=np.uint8)))


def test_pair_transform_default_is_what_it_was_and_d4_uses_the_third_draw():
    from tpu_superresolution_amd import sr_datasets as D
    lr_pil, hr_pil = _pil_pair()
    P, s = 8, 2
    lr_t, hr_t = D.ensure_3ch(D.pil_to_tensor01(lr_pil)), D.ensure_3ch(D.pil_to_tensor01(hr_pil))

    def crop_as_ever():                     # the transform before the option existed: two randint draws, two slices
        top, left = random.randint(0, 20 - P), random.randint(0, 27 - P)
        return lr_t[:, top:top + P, left:left + P], hr_t[:, top * s:(top + P) * s, left * s:(left + P) * s]

    for tf in (D.PairTransformTrain(P, s), D.PairTransformTrain(P, s, augment="none")):
        random.seed(11)
        want = crop_as_ever()
        end = random.getstate()
        random.seed(11)
        got = tf(lr_pil, hr_pil)
        assert random.getstate() == end
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    for mode, n in (("flip", 4), ("d4", 8)):
        seen = set()
        for seed in range(40):
            random.seed(seed)
            clr, chr_ = crop_as_ever()
            k = random.randrange(n)           # the third draw
            end = random.getstate()
            random.seed(seed)
            got = D.PairTransformTrain(P, s, augment=mode)(lr_pil, hr_pil)
            assert random.getstate() == end
            assert torch.equal(got[0], A.apply_op_host(clr, k)) and torch.equal(got[1], A.apply_op_host(chr_, k))
            seen.add(k)
        assert seen == set(range(n))
    with pytest.raises(ValueError, match="augment must be one of"):
        D.PairTransformTrain(P, s, augment="rot90")
    with pytest.raises(ValueError, match="augment must be one of"):
        D.DevicePairPool([(np.zeros((20, 24), np.uint8), np.zeros((80, 96), np.uint8))], 16, 4, device="cpu", augment="rot90")


def test_self_ensemble_on_cpu_tensors_averages_the_inverse_transformed_passes():
    """An equivariant 'model' (a pointwise map) gives back model(x); one that is not gives the written-out mean."""
    x = torch.rand(2, 3, 5, 7, generator=torch.Generator().manual_seed(0))
    assert torch.allclose(A.self_ensemble(lambda t: t * 2 + 1, x), x * 2 + 1, atol=1e-6)
    shift = lambda t: torch.roll(t, 1, dims=-1) * 3          # noqa: E731
    want = sum(A.apply_op_host(shift(A.apply_op_host(x, k)), A.inverse_op(k)) * 0.125 for k in range(8))
    got = A.self_ensemble(shift, x)
    assert got.shape == x.shape and torch.equal(got, want) and not torch.allclose(got, shift(x))
    assert torch.equal(A.self_ensemble(shift, x, ops=[0]), shift(x))
    with pytest.raises(ValueError):
        A.self_ensemble(shift, x, ops=[])


def test_command_lines_parse_the_new_flags():
    from tpu_superresolution_amd import evaluate, finetune_swinir
    base = ["--data_root", "d", "--scale", "X2"]
    assert finetune_swinir.parse_args(base).augment == "none"
    for mode in ("none", "flip", "d4"):
        assert finetune_swinir.parse_args(base + ["--augment", mode]).augment == mode
    with pytest.raises(SystemExit):
        finetune_swinir.parse_args(base + ["--augment", "rot90"])
    ev = ["--scale", "X2", "--ckpt", "c.pt"]
    assert evaluate.parse_args(ev).self_ensemble is False
    assert evaluate.parse_args(ev + ["--self_ensemble", "--arch", "dat"]).self_ensemble is True


def test_dihedral_entry_point_validates_arguments_without_a_gpu():
    """Every call here returns on the host before any launch; the addresses are dummies that are never dereferenced."""
    from tpu_superresolution_amd import _lib, build
    build.build(verbose=False)
    assert "srk_dihedral_f32" in _lib.declared_symbols() and "srk_dihedral_f32" in _lib._SIGNATURES
    h = _lib.lib()
    a, b, codes = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    f = h.srk_dihedral_f32
    assert f(None, b, None, 0, 1, 1, 4, 4, 1.0, 0, None) == -2
    assert f(a, None, None, 0, 1, 1, 4, 4, 1.0, 0, None) == -2
    assert f(a, b, None, 8, 1, 3, 4, 4, 1.0, 0, None) == -1 and b"0..7" in h.srk_last_error()
    assert f(a, b, None, -1, 1, 3, 4, 4, 1.0, 0, None) == -1
    for shape in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0), (-1, 3, 4, 4)):
        assert f(a, b, None, 0, *shape, 1.0, 0, None) == -1, shape
    assert f(a, b, codes, 0, 2, 3, 4, 5, 1.0, 0, None) == -1 and b"square" in h.srk_last_error()
    assert f(a, b, None, 0, 1, 1, 4, 4, 1.0, 2, None) == -1
    # overlap: identical, and out starting inside in (2 * 3 * 8 * 8 floats = 1536 bytes)
    assert f(a, a, None, 1, 2, 3, 8, 8, 1.0, 0, None) == -1 and b"overlap" in h.srk_last_error()
    assert f(a, C.c_void_p((1 << 20) + 1532), None, 1, 2, 3, 8, 8, 1.0, 0, None) == -1
    assert f(C.c_void_p((1 << 20) + 1532), a, None, 1, 2, 3, 8, 8, 1.0, 1, None) == -1
