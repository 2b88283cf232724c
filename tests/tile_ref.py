"""Brute-force restatement of the tiled-inference semantics (tpu_superresolution_amd/tiling.py, csrc/tile.hip) for the tests: numpy
loops only, nothing imported from the package.  Pinned in tests/test_tile_ref.py against the literal E.add_(patch); W.add_(1); E / W
loop of the SwinIR test script.

Per pixel: the covering tiles are found by scanning every origin of each axis (no closed form), visited in ascending tile index
iy * kx + ix; 'mean' adds them to 0 as sequential fp32 adds and divides once by their count in fp32, 'center' copies from the covering
tile that maximises min(p - o, o + t - 1 - p) per axis, ties to the lower index."""
import numpy as np


def origins(n, t, v):
    """The tile origins of one axis, by walking: step t - v from 0 while the tile ends before the border, then the border tile."""
    assert 1 <= t <= n and 0 <= v < t
    out, o = [], 0
    while o + t < n:
        out.append(o)
        o += t - v
    out.append(n - t)
    return out


def covering(p, t, orig):
    return [i for i, o in enumerate(orig) if o <= p < o + t]


def owner(p, t, orig):
    best, best_m = None, -1
    for i in covering(p, t, orig):
        m = min(p - orig[i], orig[i] + t - 1 - p)
        if m > best_m:
            best, best_m = i, m
    return best


def gather(x, th, tw, oys, oxs):
    """x [B,C,H,W] -> tiles [N,B,C,th,tw], N = len(oys) * len(oxs) row-major."""
    x = np.asarray(x)
    return np.stack([x[:, :, oy:oy + th, ox:ox + tw] for oy in oys for ox in oxs])


def merge(tiles, Ho, Wo, th, tw, oys, oxs, blend, skip=(), order=None, tie_high=False):
    """tiles [N,B,C,th,tw] fp32 -> out [B,C,Ho,Wo] fp32, pixel by pixel.

    The three knobs exist for the negative controls only: `skip` drops tile indices from the covering sets, `order` re-orders each
    pixel's covering list (a function list -> list), `tie_high` sends 'center' ties to the higher index."""
    tiles = np.asarray(tiles, dtype=np.float32)
    N, B, C = tiles.shape[:3]
    kx = len(oxs)
    assert N == len(oys) * kx and tiles.shape[3:] == (th, tw)
    out = np.empty((B, C, Ho, Wo), dtype=np.float32)
    cov_x = [covering(X, tw, oxs) for X in range(Wo)]
    own_x = [owner(X, tw, oxs) for X in range(Wo)]
    if tie_high:
        own_x = [max(c, key=lambda i, X=X: (min(X - oxs[i], oxs[i] + tw - 1 - X), i)) for X, c in enumerate(cov_x)]
    with np.errstate(all="ignore"):          # Inf - Inf and NaN inputs are part of the tests
        for Y in range(Ho):
            cov_y = covering(Y, th, oys)
            own_y = owner(Y, th, oys)
            if tie_high:
                own_y = max(cov_y, key=lambda i: (min(Y - oys[i], oys[i] + th - 1 - Y), i))
            for X in range(Wo):
                if blend == "center":
                    iy, ix = own_y, own_x[X]
                    out[:, :, Y, X] = tiles[iy * kx + ix, :, :, Y - oys[iy], X - oxs[ix]]
                    continue
                assert blend == "mean"
                cover = [(iy, ix) for iy in cov_y for ix in cov_x[X] if iy * kx + ix not in skip]
                if order is not None:
                    cover = order(cover)
                acc = np.zeros((B, C), dtype=np.float32)
                for iy, ix in cover:
                    acc = acc + tiles[iy * kx + ix, :, :, Y - oys[iy], X - oxs[ix]]
                out[:, :, Y, X] = acc / np.float32(len(cover))
    return out


def tiled(fn, x, th, tw, vy, vx, blend):
    """The whole pipeline on a numpy batch: fn maps one tile batch [B,C,th,tw] to [B,C',th s,tw s]; tiles one by one."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[-2:]
    oys, oxs = origins(H, th, vy), origins(W, tw, vx)
    ys = np.stack([np.asarray(fn(t), dtype=np.float32) for t in gather(x, th, tw, oys, oxs)])
    s = ys.shape[-2] // th
    assert ys.shape[-2:] == (th * s, tw * s)
    return merge(ys, H * s, W * s, th * s, tw * s, [o * s for o in oys], [o * s for o in oxs], blend)
