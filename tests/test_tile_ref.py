"""The tiled-inference semantics without a GPU: tests/tile_ref.py (the brute-force reference of tests/test_gpu_tile.py) pinned against
the literal loop of the SwinIR test script, tiling.tile_origins, the host path of tiling.tiled_forward, its refusals, and the new
command-line flags.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import tile_ref as R
from tpu_superresolution_amd import tiling as T

# (H, W, th, tw, vy, vx)
GRIDS = [(1, 1, 1, 1, 0, 0), (13, 12, 5, 5, 3, 3), (10, 10, 4, 4, 0, 0), (16, 24, 8, 8, 0, 0), (9, 30, 9, 12, 0, 4), (11, 14, 7, 7, 6, 6),
         (12, 9, 5, 4, 2, 1)]


def _bits(a):
    return torch.as_tensor(np.ascontiguousarray(a)).view(torch.int32)


def _script_lists(n, t, v):
    """The index list of the SwinIR test script (main_test_swinir.py: h_idx_list / w_idx_list)."""
    return list(range(0, n - t, t - v)) + [n - t]


def _script_loop(tiles, H, W, th, tw, vy, vx):
    """E.add_(patch); W.add_(1); E / W over the script's two nested loops, in torch."""
    tiles = torch.as_tensor(tiles)
    E = torch.zeros(tiles.shape[1], tiles.shape[2], H, W)
    Wt = torch.zeros_like(E)
    j = 0
    for h_idx in _script_lists(H, th, vy):
        for w_idx in _script_lists(W, tw, vx):
            E[..., h_idx:h_idx + th, w_idx:w_idx + tw].add_(tiles[j])
            Wt[..., h_idx:h_idx + th, w_idx:w_idx + tw].add_(1)
            j += 1
    assert j == tiles.shape[0]
    return E.div_(Wt)


def _random_tiles(grid, seed, B=2, C=2):
    H, W, th, tw, vy, vx = grid
    oys, oxs = R.origins(H, th, vy), R.origins(W, tw, vx)
    tiles = np.random.default_rng(seed).standard_normal((len(oys) * len(oxs), B, C, th, tw)).astype(np.float32)
    return tiles, oys, oxs


def test_origins_are_the_list_of_the_swinir_script():
    count = 0
    for n in range(1, 21):
        for t in range(1, n + 1):
            for v in range(t):
                want = _script_lists(n, t, v)
                assert T.tile_origins(n, t, v) == want, (n, t, v)
                assert R.origins(n, t, v) == want, (n, t, v)
                assert len(want) == -(-(n - t) // (t - v)) + 1 and all(want[i] == min(i * (t - v), n - t) for i in range(len(want)))
                count += 1
    assert count == sum(t for n in range(1, 21) for t in range(1, n + 1))
    for bad in ((4, 5, 0), (4, 0, 0), (4, 2, 2), (4, 2, -1), (0, 1, 0)):
        with pytest.raises(ValueError):
            T.tile_origins(*bad)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "-".join(map(str, g)))
def test_reference_mean_is_the_script_loop(grid):
    H, W, th, tw, vy, vx = grid
    tiles, oys, oxs = _random_tiles(grid, seed=H * 100 + W)
    got = R.merge(tiles, H, W, th, tw, oys, oxs, "mean")
    assert torch.equal(_bits(got), _bits(_script_loop(tiles, H, W, th, tw, vy, vx).numpy()))
    # and 'center' copies every pixel from a tile that covers it, the one the rule names
    cen = R.merge(tiles, H, W, th, tw, oys, oxs, "center")
    for Y in range(H):
        for X in range(W):
            iy, ix = R.owner(Y, th, oys), R.owner(X, tw, oxs)
            assert oys[iy] <= Y < oys[iy] + th and oxs[ix] <= X < oxs[ix] + tw
            assert np.array_equal(cen[:, :, Y, X], tiles[iy * len(oxs) + ix, :, :, Y - oys[iy], X - oxs[ix]])


def test_center_owner_by_hand():
    # n = 12, t = 5, overlap 3: origins 0 2 4 6 7.  p = 3: covered by tiles 0 (margin min(3, 1) = 1), 1 (min(1, 3) = 1): a tie -> tile 0;
    # p = 4: tiles 0 (0), 1 (2), 2 (0) -> 1;  p = 9: tiles 2 (none: 4..8), 3 (min(3, 1) = 1), 4 (min(2, 2) = 2) -> 4
    orig = R.origins(12, 5, 3)
    assert orig == [0, 2, 4, 6, 7]
    assert [R.owner(p, 5, orig) for p in range(12)] == [0, 0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 4]


def test_negative_controls_change_the_result():
    grid = (13, 12, 5, 5, 3, 3)
    H, W, th, tw, vy, vx = grid
    tiles, oys, oxs = _random_tiles(grid, seed=5)
    want = R.merge(tiles, H, W, th, tw, oys, oxs, "mean")
    dropped = R.merge(tiles, H, W, th, tw, oys, oxs, "mean", skip={7})
    assert not np.array_equal(dropped, want)
    rev = R.merge(tiles, H, W, th, tw, oys, oxs, "mean", order=lambda c: c[::-1])
    assert not np.array_equal(rev, want) and np.allclose(rev, want, rtol=1e-5, atol=1e-6)      # the same sum in another order
    ints = np.rint(tiles * 100)                                                              # on integers the order is immaterial
    assert np.array_equal(R.merge(ints, H, W, th, tw, oys, oxs, "mean", order=lambda c: c[::-1]), R.merge(ints, H, W, th, tw, oys, oxs, "mean"))
    cen = R.merge(tiles, H, W, th, tw, oys, oxs, "center")
    high = R.merge(tiles, H, W, th, tw, oys, oxs, "center", tie_high=True)
    assert not np.array_equal(high, cen)
    assert not np.array_equal(cen, want)


def _stub(s):
    """An exact model: s x nearest upsample, times 2, plus 1; records the shape of every call."""
    calls = []

    def f(t):
        calls.append(tuple(t.shape))
        return t.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1) * 2 + 1
    f.calls = calls
    return f


def _stub_np(s):
    return lambda t: np.repeat(np.repeat(t, s, axis=-2), s, axis=-1) * 2 + 1


@pytest.mark.parametrize("blend", ["mean", "center"])
@pytest.mark.parametrize("grid", GRIDS[1:], ids=lambda g: "-".join(map(str, g)))
def test_host_path_of_tiled_forward(grid, blend):
    H, W, th, tw, vy, vx = grid
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    N = len(R.origins(H, th, vy)) * len(R.origins(W, tw, vx))
    for s in (1, 2, 3):
        want = R.tiled(_stub_np(s), x.numpy(), th, tw, vy, vx, blend)
        for tb in (1, 4, N):
            m = _stub(s)
            got = T.tiled_forward(m, x, (th, tw), (vy, vx), tile_batch=tb, blend=blend)
            assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, H * s, W * s)
            assert torch.equal(_bits(got.numpy()), _bits(want)), (s, tb)
            if N > 1:
                assert len(m.calls) == -(-N // tb) and all(c[0] <= tb * 2 and c[1:] == (3, th, tw) for c in m.calls)
                assert sum(c[0] for c in m.calls) == N * 2


def test_host_path_clamps_and_short_circuits():
    x = torch.randn(1, 2, 9, 14, generator=torch.Generator().manual_seed(0))
    m = _stub(2)
    for tile in (14, 64, (9, 14), (9, 100)):
        got = T.tiled_forward(m, x, tile, overlap=3)                    # a tile >= the image on both axes: one call on x itself
        assert m.calls[-1] == (1, 2, 9, 14) and torch.equal(got, m(x))
    n = len(m.calls)
    got = T.tiled_forward(m, x, 12, overlap=10)                         # clamped to 9 rows: one tile row, whose overlap is not used
    assert len(m.calls) == n + 2 and m.calls[-1] == (1, 2, 9, 12)
    assert torch.equal(_bits(got.numpy()), _bits(R.tiled(_stub_np(2), x.numpy(), 9, 12, 0, 10, "mean")))
    # an int and a pair are the same thing
    assert torch.equal(T.tiled_forward(m, x, 6, 2), T.tiled_forward(m, x, (6, 6), (2, 2)))
    # no gradient is recorded
    w = torch.ones(1, requires_grad=True)
    assert not T.tiled_forward(lambda t: t * w, x, 6, 2).requires_grad


def test_refusals_of_tiled_forward():
    x = torch.zeros(1, 1, 8, 8)
    m = _stub(1)
    for kw, msg in ((dict(tile=0), "at least 1"), (dict(tile=(4, 0)), "at least 1"), (dict(tile=4, overlap=4), "overlap"),
                    (dict(tile=4, overlap=-1), "overlap"), (dict(tile=(4, 6), overlap=(3, 6)), "overlap"),
                    (dict(tile=4, overlap=1, tile_batch=0), "tile_batch"), (dict(tile=4, overlap=1, blend="max"), "blend"),
                    (dict(tile=(4, 4, 4)), "pair")):
        with pytest.raises(ValueError, match=msg):
            T.tiled_forward(m, x, **kw)
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        T.tiled_forward(m, x[0], 4, 1)
    with pytest.raises(ValueError, match="one integer factor"):
        T.tiled_forward(lambda t: t.repeat_interleave(2, dim=-1), x, 4, 1)          # scales one axis only
    with pytest.raises(ValueError, match="one integer factor"):
        T.tiled_forward(lambda t: t[..., :3, :3], x, 4, 1)                          # shrinks
    with pytest.raises(ValueError, match="batch of 1"):
        T.tiled_forward(lambda t: torch.cat([t, t]), x, 4, 1)
    assert m.calls == []                                                          # the argument checks come before any call


def test_package_exports():
    import tpu_superresolution_amd as P
    assert P.tiled_forward is T.tiled_forward and P.tile_origins is T.tile_origins
    assert T.BLENDS == ("mean", "center")


def test_evaluate_flags():
    from tpu_superresolution_amd import evaluate as E
    base = ["--scale", "X4", "--ckpt", "c.pt"]
    a = E.parse_args(base)
    assert (a.tile, a.tile_overlap, a.tile_batch, a.tile_blend) == (0, 32, 1, "mean") and a.self_ensemble is False
    a = E.parse_args(base + ["--tile", "64", "--tile_overlap", "8", "--tile_batch", "4", "--tile_blend", "center", "--arch", "hat"])
    assert (a.tile, a.tile_overlap, a.tile_batch, a.tile_blend, a.arch) == (64, 8, 4, "center", "hat")
    assert E.parse_args(base + ["--tile", "48"]).tile_overlap == 32
    for bad in (["--tile", "-1"], ["--tile", "32"], ["--tile", "16", "--tile_overlap", "16"], ["--tile", "64", "--tile_batch", "0"],
                ["--tile", "64", "--tile_blend", "max"], ["--tile", "64", "--tile_overlap", "-2"]):
        with pytest.raises(SystemExit):
            E.parse_args(base + bad)


def test_finetune_flags_and_validate_signature():
    import inspect

    from tpu_superresolution_amd import finetune_swinir as F
    base = ["--data_root", "d", "--scale", "X2"]
    a = F.parse_args(base)
    assert (a.val_tile, a.val_tile_overlap) == (0, 32)
    a = F.parse_args(base + ["--val_tile", "48", "--val_tile_overlap", "8"])
    assert (a.val_tile, a.val_tile_overlap) == (48, 8)
    for bad in (["--val_tile", "-4"], ["--val_tile", "32"], ["--val_tile", "8", "--val_tile_overlap", "8"]):
        with pytest.raises(SystemExit):
            F.parse_args(base + bad)
    sig = inspect.signature(F.validate)
    assert list(sig.parameters) == ["model", "loader", "device", "with_ssim", "predict"] and sig.parameters["predict"].default is None

