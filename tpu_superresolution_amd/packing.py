"""Weight packing for the host-run passes (HAT, DAT, SwinIR at window 2..7 / 16): bf16 / padded / permuted copies of the parameters in
the kernels' layouts, built with torch on the device once per parameter version (cached_pack).  A model is packed after every optimizer
step, so the count of tiny torch kernels matters: inside ``batched_pack()`` the _pack_* helpers only RECORD their request and return a
placeholder; ``resolve`` groups requests of the same kind / shape / index maps (the 42 qkv weights of HAT, ...), runs each group as ONE
stack + scatter + cast and hands out views of the stacked result.  Outside the context they run eagerly, one tensor at a time."""
from __future__ import annotations

import threading
from typing import Callable, Dict, Optional

import torch


def _rup(v, m):
    return (v + m - 1) // m * m


# ---- index maps --------------------------------------------------------------------------------------------------------------------------
_MAPS: Dict[tuple, torch.Tensor] = {}


def _cached_map(key: tuple, make):
    t = _MAPS.get(key)
    if t is None:
        t = _MAPS[key] = make()
    return t


def _head_map(nH: int, dh: int, device) -> torch.Tensor:
    """channel h * dh + d -> padded channel h * 32 + d   (one tensor per (heads, head_dim, device): the batched packer groups by identity)"""
    def make():
        c = torch.arange(nH * dh, device=device)
        return (c // dh) * 32 + c % dh
    return _cached_map(("head", nH, dh, str(device)), make)


def _qkv_rows(nH: int, dh: int, device) -> torch.Tensor:
    """row of the packed qkv weight of output feature (which, h, d)"""
    return _cached_map(("qkv", nH, dh, str(device)), lambda: torch.cat([w * nH * 32 + _head_map(nH, dh, device) for w in range(3)]))


def _ps_map(C_out: int, r: int, Cs: int, device) -> torch.Tensor:
    """PixelShuffle conv: original output channel c * r^2 + i * r + j -> packed row (i * r + j) * Cs + c"""
    def make():
        n = torch.arange(C_out, device=device)
        c, ij = n // (r * r), n % (r * r)
        return ij * Cs + c
    return _cached_map(("ps", C_out, r, Cs, str(device)), make)


# ---- the batched packer ------------------------------------------------------------------------------------------------------------------
class _Pending:
    __slots__ = ("group", "index")

    def __init__(self, group, index):
        self.group, self.index = group, index


class _Packer:
    def __init__(self):
        self.groups: Dict[tuple, list] = {}

    def add(self, kind, src, args, maps):
        key = (kind, tuple(src.shape), src.dtype, src.device, args, tuple(id(m_) if m_ is not None else None for m_ in maps))
        g = self.groups.setdefault(key, [kind, args, maps, []])
        g[3].append(src)
        return _Pending(key, len(g[3]) - 1)

    def resolve(self, P: dict) -> None:
        done = {}
        for key, (kind, args, maps, srcs) in self.groups.items():
            done[key] = _PACK_MANY[kind](torch.stack([t.float() for t in srcs]), *args, *maps)
        for name, v in P.items():
            if isinstance(v, _Pending):
                P[name] = done[v.group][v.index]


_TLS = threading.local()        # the active packer is per thread (two threads may pack two models at once)


def _active() -> Optional[_Packer]:
    return getattr(_TLS, "packer", None)


class batched_pack:
    """with batched_pack() as pk: ... P[name] = _pack_linear(...) ...; pk.resolve(P)"""

    def __enter__(self):
        self.prev = _active()
        _TLS.packer = _Packer()
        return _TLS.packer

    def __exit__(self, *exc):
        _TLS.packer = self.prev


def _many_linear(ws, NP, KP, row_map, col_map):
    n, N, K = ws.shape
    out = torch.zeros(n, NP, KP, dtype=torch.float32, device=ws.device)
    rows = row_map if row_map is not None else torch.arange(N, device=ws.device)
    cols = col_map if col_map is not None else torch.arange(K, device=ws.device)
    out[:, rows[:, None], cols[None, :]] = ws
    return out.to(torch.bfloat16)


def _many_vec(bs, NP, row_map):
    n, N = bs.shape
    out = torch.zeros(n, NP, dtype=torch.float32, device=bs.device)
    rows = row_map if row_map is not None else torch.arange(N, device=bs.device)
    out[:, rows] = bs
    return out


def _many_conv(ws, NP, CinP, row_map):
    n, Cout, Cin = ws.shape[:3]
    out = torch.zeros(n, NP, 9, CinP, dtype=torch.float32, device=ws.device)
    rows = row_map if row_map is not None else torch.arange(Cout, device=ws.device)
    out[:, rows, :, :Cin] = ws.permute(0, 1, 3, 4, 2).reshape(n, Cout, 9, Cin)
    return out.reshape(n, NP, 9 * CinP).to(torch.bfloat16)


def _many_conv_T(ws, NP, CoutP, col_map):
    n, Cout, Cin = ws.shape[:3]
    out = torch.zeros(n, NP, 9, CoutP, dtype=torch.float32, device=ws.device)
    cols = col_map if col_map is not None else torch.arange(Cout, device=ws.device)
    out[:, :Cin, :, cols] = ws.flip(3, 4).permute(0, 2, 3, 4, 1).reshape(n, Cin, 9, Cout)
    return out.reshape(n, NP, 9 * CoutP).to(torch.bfloat16)


_PACK_MANY = {"linear": _many_linear, "vec": _many_vec, "conv": _many_conv, "convT": _many_conv_T}


def _pack_linear(w: torch.Tensor, NP: int, KP: int, row_map=None, col_map=None) -> torch.Tensor:
    """fp32 [N][K] -> bf16 [NP][KP], rows / columns scattered through the given index maps (zero elsewhere)."""
    pk = _active()
    if pk is not None:
        return pk.add("linear", w, (NP, KP), (row_map, col_map))
    return _many_linear(w.float()[None], NP, KP, row_map, col_map)[0].contiguous()


def _pack_vec(b: Optional[torch.Tensor], NP: int, row_map=None, device=None) -> torch.Tensor:
    if b is None:
        return torch.zeros(NP, dtype=torch.float32, device=device)
    pk = _active()
    if pk is not None:
        return pk.add("vec", b, (NP,), (row_map,))
    return _many_vec(b.float()[None], NP, row_map)[0]


def _pack_conv(w: torch.Tensor, NP: int, CinP: int, row_map=None) -> torch.Tensor:
    """[Cout][Cin][3][3] -> bf16 [NP][9 * CinP], K tap-major: k = (3 ky + kx) * CinP + ci."""
    pk = _active()
    if pk is not None:
        return pk.add("conv", w, (NP, CinP), (row_map,))
    return _many_conv(w.float()[None], NP, CinP, row_map)[0].contiguous()


def _pack_conv_T(w: torch.Tensor, NP: int, CoutP: int, col_map=None) -> torch.Tensor:
    """[Cout][Cin][3][3] -> bf16 [NP (input channels)][9 * CoutP]: the dgrad's weight, taps flipped, K = (tap, output channel)."""
    pk = _active()
    if pk is not None:
        return pk.add("convT", w, (NP, CoutP), (col_map,))
    return _many_conv_T(w.float()[None], NP, CoutP, col_map)[0].contiguous()


# ---- what every Swin-style block packs ---------------------------------------------------------------------------------------------------
def pack_attn(P: dict, pre: str, qkv, proj, nH: int, dh: int, CP: int, device) -> None:
    """qkv / proj of a block with nH heads of dh channels, each head padded to 32 channels (a qkv without bias gets a zero one)"""
    CA, hm, qkv_rows = nH * 32, _head_map(nH, dh, device), _qkv_rows(nH, dh, device)
    P[pre + "Wqkv"] = _pack_linear(qkv.weight, 3 * CA, CP, row_map=qkv_rows)
    P[pre + "bqkv"] = _pack_vec(qkv.bias, 3 * CA, row_map=qkv_rows, device=device)
    P[pre + "Wproj"] = _pack_linear(proj.weight, CP, CA, col_map=hm)
    P[pre + "bproj"] = _pack_vec(proj.bias, CP)


def pack_mlp(P: dict, pre: str, fc1, fc2, HP: int, CP: int) -> None:
    P[pre + "W1"] = _pack_linear(fc1.weight, HP, CP)
    P[pre + "b1"] = _pack_vec(fc1.bias, HP)
    P[pre + "W2"] = _pack_linear(fc2.weight, CP, HP)
    P[pre + "b2"] = _pack_vec(fc2.bias, CP)


def pack_attn_T(P: dict, pre: str, qkv, proj, nH: int, dh: int, CP: int, device) -> None:
    """the transposed copies for the qkv / proj dgrads: [c][3 CA] and [ca][c]"""
    CA = nH * 32
    P[pre + "WqkvT"] = _pack_linear(qkv.weight.t(), CP, 3 * CA, col_map=_qkv_rows(nH, dh, device))
    P[pre + "WprojT"] = _pack_linear(proj.weight.t(), CA, CP, row_map=_head_map(nH, dh, device))


def pack_mlp_T(P: dict, pre: str, fc1, fc2, HP: int, CP: int) -> None:
    P[pre + "W1T"] = _pack_linear(fc1.weight.t(), CP, HP)
    P[pre + "W2T"] = _pack_linear(fc2.weight.t(), HP, CP)


# ---- the cache ---------------------------------------------------------------------------------------------------------------------------
class _Packs(dict):
    """{slot: (key, pack)} of one model.  It lives in model.__dict__ (no state_dict entry); a copy of the model starts without packs."""

    def __deepcopy__(self, memo):
        return _Packs()


def params_version(model) -> int:
    """changes whenever a parameter is written in place (optimizer step, load_state_dict, optim's fused step via _increment_version)"""
    return sum(p._version for p in model.parameters())


def cached_pack(model, slot: str, device, fill: Callable[[dict], None], *, buffers: bool = False, extra=None) -> dict:
    """The pack in ``slot`` of ``model``.  Hit: the slot holds a pack built for the same device, the same sum of the parameters' version
    counters (buffers=True: and of the buffers', for a pack that reads buffers) and an equal ``extra``.  Otherwise fill(P) writes a new
    pack inside one batched_pack() block (the name is looked up at every call) and the result takes the slot."""
    key = (device, params_version(model), sum(b._version for b in model.buffers()) if buffers else None, extra)
    packs = model.__dict__.setdefault("_packs", _Packs())
    hit = packs.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    P: Dict[str, torch.Tensor] = {}
    with torch.no_grad(), batched_pack() as pk:
        fill(P)
        pk.resolve(P)
    packs[slot] = (key, P)
    return P


def drop_packs(model) -> None:
    model.__dict__.pop("_packs", None)
