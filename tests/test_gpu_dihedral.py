"""srk_dihedral_f32 (csrc/dihedral.hip) and what is built on it: the D4 augmentation of the device-resident training set, the x8
self-ensemble, and the two command lines.  The op is a permutation and every alpha used here is a power of two, so nothing is
rounded: all comparisons are exact (bit patterns where NaNs are involved).  The reference is augment.apply_op_host (torch.flip /
transpose), itself pinned against an explicit index map in tests/test_augment_host.py."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from guarded import Guarded
from tpu_superresolution_amd import augment as A
from tpu_superresolution_amd import sr_datasets as D

pytestmark = pytest.mark.gpu

E_SHAPE = -1


def _call(x, out_ptr, ops, op_all, shape, alpha=1.0, accumulate=0):
    from tpu_superresolution_amd._lib import lib
    B, C, H, W = shape
    return lib().srk_dihedral_f32(x if isinstance(x, int) else x.data_ptr(), out_ptr, None if ops is None else ops.data_ptr(), op_all,
                                  B, C, H, W, alpha, accumulate, torch.cuda.current_stream().cuda_stream)


def _special_input(shape, seed):
    """Random fp32 with NaN, +Inf, -Inf and -0.0 planted at random places (as many as fit)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:8]
    for i, p in enumerate(where.tolist()):
        flat[p] = (float("nan"), float("inf"), float("-inf"), -0.0)[i % 4]
    return x


SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 3, 1, 70), (1, 1, 70, 1), (2, 1, 63, 65), (1, 3, 64, 64), (1, 1, 130, 67)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_op_at_every_tile_edge(shape):
    B, C, H, W = shape
    n = B * C * H * W
    x = _special_input(shape, seed=n)
    xd = x.cuda()
    for k in range(8):
        want = A.apply_op_host(x, k)
        out = Guarded("f32", 1, n, n)
        assert _call(xd, out.ptr, None, k, shape) == 0, k
        out.assert_guards(f"op {k} on {shape}")
        got = out.data().reshape(want.shape)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"op {k} on {shape}"
    # the Python entry point: same results, output geometry chosen from the op
    for k in (0, 3, 5, 6):
        got = A.dihedral(xd, k)
        want = A.apply_op_host(x, k)
        assert got.shape == want.shape and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


CODES = [3, 6, 0, 5, 1, 7, 2, 4, 4, 1, 7, 0, 6, 2, 5, 3]          # a fixed shuffle holding each of 0..7 twice


def test_per_sample_codes():
    assert sorted(CODES) == sorted(list(range(8)) * 2)
    shape = (16, 2, 33, 33)
    n = 16 * 2 * 33 * 33
    x = _special_input(shape, seed=7)
    xd = x.cuda()
    want = torch.stack([A.apply_op_host(x[b], CODES[b]) for b in range(16)])
    for name, codes in (("plain", CODES), ("k | 8", [k | 8 for k in CODES]), ("k - 8", [k - 8 for k in CODES]),
                        ("k | 0x7ffffff8", [k | 0x7FFFFFF8 for k in CODES])):
        dev = torch.tensor(codes, dtype=torch.int32).cuda()
        out = Guarded("f32", 1, n, n)
        assert _call(xd, out.ptr, dev, 99, shape) == 0, name          # op_all is not read when codes are given
        out.assert_guards(f"per-sample codes ({name})")
        got = out.data().reshape(shape)
        for b in range(16):
            assert torch.equal(got[b].view(torch.int32), want[b].view(torch.int32)), f"{name}: sample {b}, code {codes[b]}"
    # the Python entry point: a host sequence (checked, uploaded) and a device tensor
    assert torch.equal(A.dihedral(xd, CODES).cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(A.dihedral(xd, torch.tensor(CODES, dtype=torch.int32).cuda()).cpu().view(torch.int32), want.view(torch.int32))


def test_accumulation_and_overwrite():
    B, C, H, W = 2, 3, 37, 70                                           # edge tiles in both directions, two tiles across
    n = B * C * H * W
    g = torch.Generator().manual_seed(3)
    xs = [torch.randint(-1000, 1001, (B, C, W, H) if k & 4 else (B, C, H, W), generator=g).float() for k in range(8)]
    want = torch.zeros(B, C, H, W)
    for k in range(8):
        want = want + 0.125 * A.apply_op_host(xs[k], k)                # exact in fp32: multiples of 1/8 far below 2^24
    out = Guarded("f32", 1, n, n, fill=torch.zeros(1, n))
    for k in range(8):
        assert _call(xs[k].cuda(), out.ptr, None, k, tuple(xs[k].shape), alpha=0.125, accumulate=1) == 0
        out.assert_guards(f"accumulating launch {k}")
    assert torch.equal(out.data().reshape(B, C, H, W), want)
    # accumulate == 0 ignores what the buffer held: the NaN pattern the guarded window starts with is gone
    for k in (1, 6):
        out = Guarded("f32", 1, n, n)
        assert bool(torch.isnan(out.data()).all())
        assert _call(xs[k].cuda(), out.ptr, None, k, tuple(xs[k].shape), alpha=0.125, accumulate=0) == 0
        out.assert_guards(f"scaled launch {k}")
        assert torch.equal(out.data().reshape(B, C, H, W), 0.125 * A.apply_op_host(xs[k], k))
    # Python entry point: accumulate into a given buffer
    acc = torch.zeros(B, C, H, W, device="cuda")
    for k in range(8):
        assert A.dihedral(xs[k].cuda(), k, out=acc, alpha=0.125, accumulate=True) is acc
    assert torch.equal(acc.cpu(), want)


def test_refusals_leave_the_output_untouched():
    from tpu_superresolution_amd._lib import SrkError, lib
    x = torch.rand(2, 3, 8, 12, device="cuda")
    codes = torch.zeros(2, dtype=torch.int32, device="cuda")
    n = x.numel()
    out = Guarded("f32", 1, n, n)
    assert _call(x, out.ptr, codes, 0, (2, 3, 8, 12)) == E_SHAPE and b"square" in lib().srk_last_error()
    assert _call(x, out.ptr, None, 8, (2, 3, 8, 12)) == E_SHAPE and b"0..7" in lib().srk_last_error()
    assert _call(x, out.ptr, None, 0, (0, 3, 8, 12)) == E_SHAPE
    # overlapping in / out: the same buffer, and windows that share their last / first four bytes
    assert _call(out.ptr, out.ptr, None, 1, (2, 3, 8, 12)) == E_SHAPE and b"overlap" in lib().srk_last_error()
    assert _call(out.ptr - 4 * (n - 1), out.ptr, None, 1, (2, 3, 8, 12)) == E_SHAPE
    assert _call(out.ptr + 4 * (n - 1), out.ptr, None, 1, (2, 3, 8, 12), 0.5, 1) == E_SHAPE
    torch.cuda.synchronize()
    out.assert_untouched("the output of a refused call")
    # the Python entry point refuses the same, before the library where it can
    with pytest.raises(ValueError, match="square"):
        A.dihedral(x, [0, 5])
    with pytest.raises(ValueError, match="0..7"):
        A.dihedral(x, 8)
    with pytest.raises(ValueError, match="0..7"):
        A.dihedral(x[:, :, :, :8].contiguous(), [0, 9])
    with pytest.raises(ValueError, match="2 samples, 3 codes"):
        A.dihedral(x[:, :, :, :8].contiguous(), [0, 1, 2])
    with pytest.raises(ValueError, match="accumulate"):
        A.dihedral(x, 1, accumulate=True)
    with pytest.raises(ValueError, match="out must be"):
        A.dihedral(x, 4, out=torch.empty_like(x))                      # a transposing op writes [.., W, H]
    with pytest.raises(SrkError, match="overlap"):
        A.dihedral(x, 1, out=x)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        A.dihedral(x.cpu(), 1)


def _pairs(seed, n, scale, min_lr=20, max_lr=45):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = int(rng.integers(min_lr, max_lr)), int(rng.integers(min_lr, max_lr))
        shp = (lambda f: (h * f, w * f)) if i % 3 == 0 else (lambda f: (h * f, w * f, 3))       # every third pair is gray
        out.append((Image.fromarray(rng.integers(0, 256, shp(1), dtype=np.uint8)),
                    Image.fromarray(rng.integers(0, 256, shp(scale), dtype=np.uint8))))
    return out


ORDER = [4, 0, 8, 8, 3, 1, 7, 2, 5, 6, 0, 4]                        # repeats allowed: every draw gets its own corner and code


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("augment", ["flip", "d4"])
def test_pool_path_equals_host_path(scale, augment):
    patch = 16
    pairs = _pairs(scale * 10 + len(augment), 9, scale)
    pool = D.DevicePairPool(pairs, patch, scale, device="cuda", augment=augment)
    host = D.PairTransformTrain(patch, scale, augment)
    random.seed(4321)
    ref = [host(*pairs[i]) for i in ORDER]
    host_end = random.getstate()
    random.seed(4321)
    lr, hr = pool.sample(ORDER)
    assert random.getstate() == host_end
    assert lr.shape == (len(ORDER), 3, patch, patch) and hr.shape == (len(ORDER), 3, patch * scale, patch * scale)
    assert torch.equal(lr.cpu(), torch.stack([r[0] for r in ref]))
    assert torch.equal(hr.cpu(), torch.stack([r[1] for r in ref]))
    # the batch is an augmented one: the same corners without the codes give something else
    plain = D.PairTransformTrain(patch, scale)
    random.seed(4321)
    bare = []
    for i in ORDER:
        bare.append(plain(*pairs[i])[0])
        A.draw_op(augment)
    assert not torch.equal(lr.cpu(), torch.stack(bare))


def test_pool_without_augmentation_is_the_pool_as_it_was():
    pairs = _pairs(5, 9, 2)
    random.seed(77)
    want = D.DevicePairPool(pairs, 16, 2, device="cuda").sample(ORDER)
    end = random.getstate()
    random.seed(77)
    got = D.DevicePairPool(pairs, 16, 2, device="cuda", augment="none").sample(ORDER)
    assert random.getstate() == end
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _written_out(model, x):
    """The eight passes with stock torch operators on the device, accumulated in the order self_ensemble uses."""
    acc = None
    with torch.no_grad():
        for k in range(8):
            y = A.apply_op_host(model(A.apply_op_host(x, k).contiguous()), A.inverse_op(k))
            acc = torch.zeros_like(y) if acc is None else acc
            acc += 0.125 * y
    return acc


@pytest.mark.parametrize("hw", [(24, 40), (20, 27)], ids=["24x40", "20x27-reflect-pad"])
def test_self_ensemble_on_a_small_swinir(hw):
    import tpu_superresolution_amd as T
    from test_oracle_golden import tiny_weights
    _, cfg, sd = tiny_weights("ps4")
    m = T.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1])).cuda()
    got = A.self_ensemble(m, x)
    assert got.shape == (2, 3, hw[0] * 4, hw[1] * 4) and got.dtype == torch.float32
    assert torch.equal(got, _written_out(m, x))
    with torch.no_grad():
        assert not torch.equal(got, m(x))                               # negative control: it is not the single pass


def test_self_ensemble_on_a_small_hat():
    import tpu_superresolution_amd as T
    from test_oracle_golden import hat_tiny_weights
    _, cfg, sd = hat_tiny_weights()
    m = T.HAT(**cfg.kwargs())
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    x = torch.rand(1, 3, 20, 37, generator=torch.Generator().manual_seed(2)).cuda()
    got = A.self_ensemble(m, x)
    assert got.shape == (1, 3, 80, 148)
    assert torch.equal(got, _written_out(m, x))
    with torch.no_grad():
        assert not torch.equal(got, m(x))


def _make_dataset(root, lr=72, scale=4):
    """The synthetic DeepRockSR tree of tests/test_data_and_script.py, plus a test split."""
    rng = np.random.RandomState(0)
    for split, n, size in (("train", 6, lr), ("valid", 2, lr), ("test", 2, 40)):
        hr_dir = os.path.join(root, "shuffled2D", f"shuffled2D_{split}_HR")
        lr_dir = os.path.join(root, "shuffled2D", f"shuffled2D_{split}_LR_default_X{scale}")
        os.makedirs(hr_dir)
        os.makedirs(lr_dir)
        for i in range(n):
            hr = (rng.rand(size * scale, size * scale) * 255).astype(np.uint8)
            Image.fromarray(hr, "L").save(os.path.join(hr_dir, f"{i:04d}.png"))
            Image.fromarray(hr, "L").resize((size, size), Image.BICUBIC).save(os.path.join(lr_dir, f"{i:04d}x{scale}.png"))


def test_scripts_train_with_d4_and_evaluate_with_self_ensemble(tmp_path, capsys, monkeypatch):
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd import finetune_swinir as F
    root = str(tmp_path / "data")
    _make_dataset(root)
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", root, "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--lr", "1e-4",
            "--gpu_data", "--augment", "d4"])
    out = capsys.readouterr().out
    assert "[gpu_data] 6 pairs" in out and "[X4] epoch 001/1" in out and "[done] best_val_loss=" in out
    ck = tmp_path / "bestpsnr_swinir_finetune_X4.pt"
    assert torch.load(ck, map_location="cpu", weights_only=False)["args"]["augment"] == "d4"
    res = evaluate.main(["--scale", "X4", "--data_root", root, "--ckpt", str(ck), "--batch_size", "1", "--save_dir", str(tmp_path / "p"),
                         "--save_n", "1", "--arch", "swinir", "--device", "cuda", "--self_ensemble"])
    assert "[self_ensemble] x8" in capsys.readouterr().out
    assert np.isfinite(res["psnr"]) and res["n"] == 2
