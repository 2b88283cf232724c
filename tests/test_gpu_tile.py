"""srk_tile_gather_f32 / srk_tile_merge_f32 (csrc/tile.hip) and what is built on them: tiling.tiled_forward, its composition with the
self-ensemble, and the command lines.  The reference is tests/tile_ref.py (brute force per pixel, pinned against the SwinIR script's
loop in tests/test_tile_ref.py).  Every comparison is exact.

Where NaN / Inf are planted the comparison is on bit patterns, and every element's bits are pinned.  Blend 'center' is a copy and must
match the reference bit for bit, payloads included.  For blend 'mean' IEEE 754 leaves the sign and payload of a NaN that an addition
PRODUCES to the implementation (Inf + -Inf is 0xFFC00000 on x86 SSE; GPUs return another default NaN), so a numpy reference cannot say
what those bits are: against tests/tile_ref.py a NaN must sit exactly where the reference has one and every other element must match
in its bits, and the bits AT the NaN positions are compared with the same E.add_(tile) ... E / W loop written out with torch operators
on the device (`_device_loop`), whose additions run on the same hardware in the same order."""
import math
from functools import partial

import numpy as np
import pytest
import torch

import tile_ref as R
from guarded import Guarded
from test_gpu_dihedral import _make_dataset, _special_input, _written_out
from tpu_superresolution_amd import augment as A
from tpu_superresolution_amd import tiling as T

pytestmark = pytest.mark.gpu

E_SHAPE = -1
MEAN, CENTER = 0, 1
MODES = {"mean": MEAN, "center": CENTER}

# (B, C, H, W, th, tw, vy, vx)
GRIDS = [(1, 1, 1, 1, 1, 1, 0, 0),
         (2, 3, 13, 12, 5, 5, 3, 3),          # counts up to 3 per axis; rows end on a regular origin, columns on a pulled-back one
         (1, 1, 10, 10, 4, 4, 0, 0),          # zero overlap, non-divisible
         (1, 2, 16, 24, 8, 8, 0, 0),          # exact partition, every count 1
         (1, 1, 70, 67, 64, 64, 8, 8),        # two nearly coincident tiles across 64-element block edges
         (1, 3, 9, 130, 9, 48, 0, 16),        # one axis a single tile
         (2, 1, 33, 65, 7, 7, 6, 6)]          # stride 1, counts up to 7
GRID_IDS = ["x".join(map(str, g[:4])) + "-t" + "x".join(map(str, g[4:6])) + "-v" + "x".join(map(str, g[6:])) for g in GRIDS]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t if isinstance(t, int) else t.data_ptr()


def _gather(x, tiles, t0, n, B, C, H, W, th, tw, sy, sx):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_tile_gather_f32(_ptr(x), _ptr(tiles), t0, n, B, C, H, W, th, tw, sy, sx, _stream())


def _merge(tiles, out, t0, n, B, C, Ho, Wo, th, tw, sy, sx, mode):
    from tpu_superresolution_amd._lib import lib
    return lib().srk_tile_merge_f32(_ptr(tiles), _ptr(out), t0, n, B, C, Ho, Wo, th, tw, sy, sx, mode, _stream())


def _same(got, want, bits=True):
    """Bit patterns; bits=False: NaN exactly where the reference has NaN, bit patterns elsewhere (the NaNs: module docstring)."""
    got, want = torch.as_tensor(got).contiguous(), torch.as_tensor(want).contiguous()
    if got.shape != want.shape:
        return False
    g, w = got.view(torch.int32), want.view(torch.int32)
    if bits:
        return torch.equal(g, w)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(g[~gn], w[~wn])


def _device_loop(tiles, H, W, th, tw, oys, oxs):
    """E.add_(tile); W.add_(1); E / W with stock torch operators on the device, tiles in index order."""
    tiles = tiles.cuda()
    E = torch.zeros(*tiles.shape[1:3], H, W, device="cuda")
    Wt = torch.zeros(H, W, device="cuda")
    for j in range(tiles.shape[0]):
        oy, ox = oys[j // len(oxs)], oxs[j % len(oxs)]
        E[..., oy:oy + th, ox:ox + tw].add_(tiles[j])
        Wt[oy:oy + th, ox:ox + tw].add_(1)
    return (E / Wt).cpu()


def _scaled(grid, s):
    B, C, H, W, th, tw, vy, vx = grid
    return B, C, H * s, W * s, th * s, tw * s, (th - vy) * s, (tw - vx) * s


def _geometry(grid, s):
    B, C, H, W, th, tw, sy, sx = _scaled(grid, s)
    oys, oxs = R.origins(H, th, th - sy), R.origins(W, tw, tw - sx)
    return B, C, H, W, th, tw, sy, sx, oys, oxs, len(oys) * len(oxs)


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_gather_and_merge_directly(grid, scale):
    B, C, H, W, th, tw, sy, sx, oys, oxs, N = _geometry(grid, scale)
    seed = H * 1000 + W + scale
    # gather: every tile of an image with NaN / Inf / -0.0 planted, bit for bit
    x = _special_input((B, C, H, W), seed)
    n_t = N * B * C * th * tw
    tiles = Guarded("f32", 1, n_t, n_t)
    assert _gather(x.cuda(), tiles.ptr, 0, N, B, C, H, W, th, tw, sy, sx) == 0
    tiles.assert_guards(f"gather on {grid} x{scale}")
    assert _same(tiles.data().reshape(N, B, C, th, tw), R.gather(x.numpy(), th, tw, oys, oxs))
    # merge: integer-valued tiles and tiles with specials, one reference pass over both (stacked along the channels)
    g = torch.Generator().manual_seed(seed)
    ints = torch.randint(-1000, 1001, (N, B, C, th, tw), generator=g).float()
    spec = _special_input((N, B, C, th, tw), seed + 1)
    n_o = B * C * H * W
    for blend, mode in MODES.items():
        want = R.merge(torch.cat([ints, spec], dim=2).numpy(), H, W, th, tw, oys, oxs, blend)
        for name, inp, ref in (("ints", ints, want[:, :C]), ("specials", spec, want[:, C:])):
            out = Guarded("f32", 1, n_o, n_o)
            assert _merge(inp.cuda(), out.ptr, 0, N, B, C, H, W, th, tw, sy, sx, mode) == 0
            out.assert_guards(f"merge {blend} of {name} on {grid} x{scale}")
            got = out.data().reshape(B, C, H, W)
            assert _same(got, ref, bits=(blend == "center" or name == "ints")), f"merge {blend} of {name} on {grid} x{scale}"
            if name == "ints":
                assert not bool(torch.isnan(got).any())
            elif blend == "mean":                                        # the bits of the NaNs themselves (module docstring)
                dev, nan = _device_loop(spec, H, W, th, tw, oys, oxs), torch.isnan(got)
                assert torch.equal(torch.isnan(dev), nan) and torch.equal(got.view(torch.int32)[nan], dev.view(torch.int32)[nan])


def _chunkings(N):
    uneven = [0, 1, 1 + max(1, N // 3), N - 1, N] if N >= 5 else [0, 1, N]
    cuts = {f"by {c}": list(range(0, N, c)) + [N] for c in (1, 2, 3)}
    cuts["all"] = [0, N]
    cuts["uneven"] = sorted(set(uneven))
    return cuts


@pytest.mark.parametrize("blend", ["mean", "center"])
@pytest.mark.parametrize("grid", [GRIDS[1], GRIDS[6]], ids=[GRID_IDS[1], GRID_IDS[6]])
def test_chunk_invariance(grid, blend):
    B, C, H, W, th, tw, sy, sx, oys, oxs, N = _geometry(grid, 1)
    tiles = torch.randn(N, B, C, th, tw, generator=torch.Generator().manual_seed(N))
    want = torch.as_tensor(R.merge(tiles.numpy(), H, W, th, tw, oys, oxs, blend))
    td = tiles.cuda()
    n_o, per = B * C * H * W, B * C * th * tw
    results = {}
    for name, cuts in _chunkings(N).items():
        out = Guarded("f32", 1, n_o, n_o)
        assert bool(torch.isnan(out.data()).all())                       # the output starts as NaN: nothing may rely on a zero fill
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            assert _merge(td.data_ptr() + 4 * per * t0, out.ptr, t0, t1 - t0, B, C, H, W, th, tw, sy, sx, MODES[blend]) == 0
            out.assert_guards(f"{blend} chunk [{t0}, {t1}) of {name}")
        results[name] = out.data().reshape(B, C, H, W)
        assert not bool(torch.isnan(results[name]).any()), name
        assert _same(results[name], want), name
    assert all(_same(r, results["all"]) for r in results.values())
    # chunked gather: the chunks of tiles are the slices of the whole
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(1))
    whole = torch.as_tensor(R.gather(x.numpy(), th, tw, oys, oxs))
    cuts = _chunkings(N)["uneven"]
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        buf = Guarded("f32", 1, per * (t1 - t0), per * (t1 - t0))
        assert _gather(x.cuda(), buf.ptr, t0, t1 - t0, B, C, H, W, th, tw, sy, sx) == 0
        buf.assert_guards(f"gather chunk [{t0}, {t1})")
        assert _same(buf.data().reshape(t1 - t0, B, C, th, tw), whole[t0:t1])


def test_refusals_leave_the_output_untouched():
    from tpu_superresolution_amd._lib import lib
    B, C, H, W, th, tw, sy, sx = 2, 3, 13, 12, 5, 5, 2, 2                     # 5 x 5 tiles
    N = 25
    x = torch.rand(B, C, H, W, device="cuda")
    y = torch.rand(N, B, C, th, tw, device="cuda")
    n_t, n_o = y.numel(), x.numel()
    tiles, out = Guarded("f32", 1, n_t, n_t), Guarded("f32", 1, n_o, n_o)

    def g(**kw):
        a = dict(x=x, tiles=tiles.ptr, t0=0, n=N, B=B, C=C, H=H, W=W, th=th, tw=tw, sy=sy, sx=sx)
        a.update(kw)
        return _gather(*a.values())

    def m(**kw):
        a = dict(tiles=y, out=out.ptr, t0=0, n=N, B=B, C=C, H=H, W=W, th=th, tw=tw, sy=sy, sx=sx, mode=MEAN)
        a.update(kw)
        return _merge(*a.values())

    assert g(n=1) == 0 and m(t0=24, n=1, mode=CENTER) == 0                   # the argument blocks themselves are fine
    torch.cuda.synchronize()
    tiles, out = Guarded("f32", 1, n_t, n_t), Guarded("f32", 1, n_o, n_o)
    for call in (g, m):
        for bad in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(th=0), dict(tw=0), dict(n=0), dict(n=-3),       # non-positive extents
                    dict(th=14), dict(tw=13),                                                                          # tile > image
                    dict(sy=0), dict(sx=0), dict(sy=6), dict(sx=6), dict(sx=-1),                                       # stride outside 1..t
                    dict(t0=-1), dict(t0=25, n=1), dict(t0=1), dict(t0=24, n=2), dict(n=26),                           # chunk outside the grid
                    dict(B=65536, C=65536)):                                                                           # planes beyond int
            assert call(**bad) == E_SHAPE, (call.__name__, bad)
            assert lib().srk_last_error()
    assert g(sy=6) == E_SHAPE and b"stride" in lib().srk_last_error()
    assert g(th=14) == E_SHAPE and b"larger than" in lib().srk_last_error()
    assert m(t0=24, n=2) == E_SHAPE and b"outside the grid" in lib().srk_last_error()
    # 2^32 workgroups: a grid that does not fit one launch (refused on the host, so the far-away image pointer is never followed)
    huge = dict(B=32768, C=32768, H=64, th=64, W=1, tw=1, sy=1, sx=1, n=1)
    assert g(x=tiles.ptr + (1 << 45), **huge) == E_SHAPE and b"one grid" in lib().srk_last_error()
    assert m(tiles=out.ptr + (1 << 45), **huge) == E_SHAPE and b"one grid" in lib().srk_last_error()
    for mode in (-1, 2, 7):
        assert m(mode=mode) == E_SHAPE and b"mode" in lib().srk_last_error()
    # overlapping ranges: the same buffer, and windows that share their last / first four bytes
    assert g(x=tiles.ptr) == E_SHAPE and b"overlap" in lib().srk_last_error()
    assert g(x=tiles.ptr + 4 * (n_t - 1)) == E_SHAPE and g(x=tiles.ptr - 4 * (n_o - 1)) == E_SHAPE
    assert m(tiles=out.ptr) == E_SHAPE and b"overlap" in lib().srk_last_error()
    assert m(tiles=out.ptr + 4 * (n_o - 1)) == E_SHAPE and m(tiles=out.ptr - 4 * (n_t - 1)) == E_SHAPE
    torch.cuda.synchronize()
    tiles.assert_untouched("the tiles of a refused gather")
    out.assert_untouched("the output of a refused merge")
    # the Python entry refuses the same before any launch or model call
    calls = []

    def model(t):
        calls.append(t.shape)
        return t
    for kw, msg in ((dict(tile=0), "at least 1"), (dict(tile=5, overlap=5), "overlap"), (dict(tile=5, overlap=-1), "overlap"),
                    (dict(tile=5, overlap=2, tile_batch=0), "tile_batch"), (dict(tile=5, overlap=2, blend="max"), "blend")):
        with pytest.raises(ValueError, match=msg):
            T.tiled_forward(model, x, **kw)
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        T.tiled_forward(model, x[0], 5, 2)
    assert calls == []
    with pytest.raises(ValueError, match="one integer factor"):
        T.tiled_forward(lambda t: t[..., :3], x, 5, 2)


class _Stub:
    """An exact model: s x nearest upsample, times 2, plus 1; records the shape of every call."""

    def __init__(self, s):
        self.s, self.calls = s, []

    def __call__(self, t):
        self.calls.append(tuple(t.shape))
        return t.repeat_interleave(self.s, dim=-2).repeat_interleave(self.s, dim=-1) * 2 + 1


@pytest.mark.parametrize("blend", ["mean", "center"])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_tiled_forward_with_a_stub_model(s, blend):
    B, C, H, W, th, tw, vy, vx = GRIDS[1]
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(s))
    N = len(R.origins(H, th, vy)) * len(R.origins(W, tw, vx))
    assert N == 25
    want = R.tiled(lambda t: np.repeat(np.repeat(t, s, axis=-2), s, axis=-1) * 2 + 1, x.numpy(), th, tw, vy, vx, blend)
    for tb in (1, 4, N):
        m = _Stub(s)
        got = T.tiled_forward(m, x.cuda(), (th, tw), (vy, vx), tile_batch=tb, blend=blend)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B, C, H * s, W * s)
        assert _same(got.cpu(), want), tb
        assert len(m.calls) == math.ceil(N / tb)
        assert all(c[0] <= tb * B and c[0] % B == 0 and c[1:] == (C, th, tw) for c in m.calls) and sum(c[0] for c in m.calls) == N * B
    # a tile at least the image size: one call, the stub's own output
    for tile in (13, 64, (13, 12)):
        m = _Stub(s)
        got = T.tiled_forward(m, x.cuda(), tile, 3, blend=blend)
        assert m.calls == [(B, C, H, W)] and torch.equal(got, _Stub(s)(x.cuda()))


def _written_tiled(m, x, tile, overlap, blend, scale):
    """The loop of m(x[..., tile]) merged with stock torch operators on the device, tiles in index order."""
    B, C, H, W = x.shape
    oys, oxs = R.origins(H, tile, overlap), R.origins(W, tile, overlap)
    E = torch.zeros(B, C, H * scale, W * scale, device=x.device)
    Wt = torch.zeros(H * scale, W * scale, device=x.device)
    ts = tile * scale
    own_y = torch.tensor([R.owner(p, ts, [o * scale for o in oys]) for p in range(H * scale)], device=x.device)
    own_x = torch.tensor([R.owner(p, ts, [o * scale for o in oxs]) for p in range(W * scale)], device=x.device)
    with torch.no_grad():
        for iy, oy in enumerate(oys):
            for ix, ox in enumerate(oxs):
                y = m(x[..., oy:oy + tile, ox:ox + tile].contiguous())
                ys, xs = slice(oy * scale, oy * scale + ts), slice(ox * scale, ox * scale + ts)
                if blend == "mean":
                    E[..., ys, xs].add_(y)
                    Wt[ys, xs].add_(1)
                else:
                    mine = (own_y[ys] == iy)[:, None] & (own_x[xs] == ix)[None, :]
                    E[..., ys, xs] = torch.where(mine, y, E[..., ys, xs])
    return E / Wt if blend == "mean" else E


@pytest.fixture(scope="module")
def tiny_swinir():
    import tpu_superresolution_amd as P
    from test_oracle_golden import tiny_weights
    _, cfg, sd = tiny_weights("ps4")
    m = P.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize("blend", ["mean", "center"])
def test_tiled_forward_on_a_small_swinir(tiny_swinir, blend):
    m = tiny_swinir
    x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(40)).cuda()
    got = T.tiled_forward(m, x, 16, 4, tile_batch=1, blend=blend)
    assert got.shape == (2, 3, 96, 160) and got.dtype == torch.float32
    assert torch.equal(got, _written_tiled(m, x, 16, 4, blend, 4))
    with torch.no_grad():
        assert not torch.equal(got, m(x))                               # negative control: it is not the whole-image pass
        assert torch.equal(T.tiled_forward(m, x, 64, 4, blend=blend), m(x))


def test_tiled_forward_on_a_small_hat():
    import tpu_superresolution_amd as P
    from test_oracle_golden import hat_tiny_weights
    _, cfg, sd = hat_tiny_weights()
    m = P.HAT(**cfg.kwargs())
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    x = torch.rand(1, 3, 20, 37, generator=torch.Generator().manual_seed(2)).cuda()
    got = T.tiled_forward(m, x, 16, 4, tile_batch=1)
    assert got.shape == (1, 3, 80, 148)
    assert torch.equal(got, _written_tiled(m, x, 16, 4, "mean", 4))
    with torch.no_grad():
        assert not torch.equal(got, m(x))


def test_self_ensemble_over_tiles(tiny_swinir):
    m = tiny_swinir
    x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(7)).cuda()
    got = A.self_ensemble(partial(T.tiled_forward, m, tile=16, overlap=4), x)
    assert got.shape == (2, 3, 96, 160)
    assert torch.equal(got, _written_out(lambda z: _written_tiled(m, z, 16, 4, "mean", 4), x))
    assert not torch.equal(got, A.self_ensemble(m, x))


def test_validate_takes_a_predict_function(tiny_swinir):
    from tpu_superresolution_amd import finetune_swinir as F
    g = torch.Generator().manual_seed(1)
    loader = [(torch.rand(2, 3, 24, 32, generator=g), torch.rand(2, 3, 96, 128, generator=g)) for _ in range(2)]
    seen = []

    def predict(lr, tile):
        seen.append(tuple(lr.shape))
        return T.tiled_forward(tiny_swinir, lr, tile, 4)
    plain = F.validate(tiny_swinir, loader, "cuda")
    whole = F.validate(tiny_swinir, loader, "cuda", predict=partial(predict, tile=64))
    tiled = F.validate(tiny_swinir, loader, "cuda", predict=partial(predict, tile=16))
    assert seen == [(2, 3, 24, 32)] * 4
    assert whole[:2] == plain[:2] and tiled[:2] != plain[:2] and np.isfinite(tiled[0]) and np.isfinite(tiled[1])


def test_evaluate_with_tiles(tmp_path, capsys):
    from tpu_superresolution_amd import evaluate
    from tpu_superresolution_amd.finetune_swinir import build_sr_model
    root = str(tmp_path / "data")
    _make_dataset(root)                                                 # test images of 40 x 40 LR
    torch.manual_seed(0)
    ck = tmp_path / "untrained.pt"
    torch.save({"model": build_sr_model("swinir", 4).state_dict()}, ck)
    base = ["--scale", "X4", "--data_root", root, "--ckpt", str(ck), "--batch_size", "1", "--save_dir", str(tmp_path / "p"), "--save_n", "1",
            "--arch", "swinir", "--device", "cuda"]
    plain = evaluate.main(base)
    assert "[tile]" not in capsys.readouterr().out
    res = evaluate.main(base + ["--tile", "24", "--tile_overlap", "8"])
    assert "[tile] 24 overlap 8 batch 1 blend mean" in capsys.readouterr().out
    assert np.isfinite(res["psnr"]) and np.isfinite(res["ssim"]) and res["n"] == 2
    assert (res["psnr"], res["ssim"]) != (plain["psnr"], plain["ssim"])
    big = evaluate.main(base + ["--tile", "64", "--tile_batch", "3", "--tile_blend", "center"])
    assert "[tile] 64 overlap 32 batch 3 blend center" in capsys.readouterr().out
    assert (big["psnr"], big["ssim"]) == (plain["psnr"], plain["ssim"])


def test_finetune_validates_on_tiles(tmp_path, capsys, monkeypatch):
    from tpu_superresolution_amd import finetune_swinir as F
    root = str(tmp_path / "data")
    _make_dataset(root)                                                 # validation images of 72 x 72 LR
    monkeypatch.chdir(tmp_path)
    F.main(["--data_root", root, "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--lr", "1e-4", "--gpu_data",
            "--val_tile", "48", "--val_tile_overlap", "8"])
    out = capsys.readouterr().out
    assert "[val_tile] 48 overlap 8" in out and "[X4] epoch 001/1" in out and "[done] best_val_loss=" in out
    args = torch.load(tmp_path / "bestpsnr_swinir_finetune_X4.pt", map_location="cpu", weights_only=False)["args"]
    assert args["val_tile"] == 48 and args["val_tile_overlap"] == 8
