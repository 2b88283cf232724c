"""Pins tests/block_ref.py (the fp64 restatements that tests/test_gpu_block_fused.py compares the fused per-block kernels with) on the
CPU: the window maps, the shift mask and the dense bias against oracle/swinir_oracle.py; the forward restatements, chained without
rounding, against the oracle's whole SwinTransformerBlock; the backward restatements against torch.autograd; and -- the negative
controls -- shows that the comparator with its derived tolerances rejects nine deliberately wrong references at every case they apply to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_ref as R
from oracle import swinir_oracle as O

REL = 1e-11
C, CP, HID, HP, NH, D, DP, CA = R.C, R.CP, R.HID, R.HP, R.NH, R.D, R.DP, R.CA


def close(a, b, rel=REL):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-30)
    assert float((a - b).abs().max()) <= rel * scale, float((a - b).abs().max()) / scale


GEOMS = [(B, H, W, s) for B, H, W in R.row_shapes(256) for s in (0, 4)]


@pytest.mark.parametrize("B,H,W,shift", GEOMS + [(2, 8, 8, 4), (2, 16, 24, 4)])
def test_window_maps_are_the_oracles_roll_and_partition(B, H, W, shift):
    tok = R.win_to_token(B, H, W, shift)
    idx = torch.from_numpy(O.window_token_index(H, W, 8, shift)).reshape(-1)              # one sample
    assert torch.equal(tok, (torch.arange(B)[:, None] * H * W + idx[None]).reshape(-1))
    # ... and the oracle's separate roll + partition on data
    x = np.arange(B * H * W * 2, dtype=np.int64).reshape(B, H, W, 2)
    part = O.np_window_partition(O.np_roll2d(x, -shift, -shift), 8).reshape(-1, 2)
    assert np.array_equal(part, x.reshape(-1, 2)[tok.numpy()])
    inv = R.token_to_win(B, H, W, shift)
    assert torch.equal(inv[tok], torch.arange(B * H * W)) and torch.equal(tok[inv], torch.arange(B * H * W))
    # the device's closed forms (csrc/common.h: win_row_to_token / token_to_win_row / win_region_label)
    m = torch.arange(B * H * W)
    b_, p = m >> 6, m & 63
    nWw, nW = W // 8, (H // 8) * (W // 8)
    b, w = b_ // nW, b_ % nW
    y, x_ = (w // nWw * 8 + (p >> 3) + shift) % H, (w % nWw * 8 + (p & 7) + shift) % W
    assert torch.equal(tok, (b * H + y) * W + x_)
    if shift:
        ys, xs = w // nWw * 8 + (p >> 3), w % nWw * 8 + (p & 7)
        lab = torch.where(ys < H - 8, 0, torch.where(ys < H - 4, 1, 2)) * 3 + torch.where(xs < W - 8, 0, torch.where(xs < W - 4, 1, 2))
        assert torch.equal(lab[:nW * 64].view(nW, 64), R.region_labels(H, W))


@pytest.mark.parametrize("H,W", [(8, 8), (16, 24), (32, 40), (64, 72), (24, 24)])
def test_shift_mask_and_dense_bias_are_the_oracles(H, W):
    assert torch.equal(R.shift_mask(H, W), torch.from_numpy(O.shift_attn_mask(H, W, 8, 4)).double())
    table = torch.randn(225, NH, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    bd = R.dense_bias(table)
    assert torch.equal(bd, O.dense_rel_pos_bias(table, 8))
    assert torch.equal(R.rel_pos_index(), torch.from_numpy(O.relative_position_index(8)))
    # what the fused kernels read back from the dense bias (csrc/attn_fused.hip): offset (dy, dx) at query (max(dy,0), max(dx,0)),
    # key (max(-dy,0), max(-dx,0)) -- the 225-entry table again, which is why bias_dense must be table[rpi]
    for t in range(225):
        dy, dx = t // 15 - 7, t % 15 - 7
        qi, kj = max(dy, 0) * 8 + max(dx, 0), max(-dy, 0) * 8 + max(-dx, 0)
        assert torch.equal(bd[:, qi, kj], table[t])


def _exact_ln_stats(inp, rows=None):
    x = inp["ln_x"].double()
    mean = x[:, :C].mean(1)
    rstd = (x[:, :C].var(1, unbiased=False) + 1e-5).rsqrt()
    inp["ln_mean"], inp["ln_rstd"] = (mean, rstd) if rows is None else (mean[rows], rstd[rows])


@pytest.mark.parametrize("shift,rs", [(0, "none"), (4, "mix"), (4, "ones")])
def test_forward_restatements_chain_to_the_oracles_swin_block(shift, rs):
    """norm1 (torch) -> attn_qkv / attn_out -> proj_residual -> ln_rows (norm2) -> mlp_fwd_stage1 / stage2 -> ln_rows (next norm1, window
    order), every intermediate handed on UNROUNDED, is oracle.swin_block in fp64 -- with DropPath factors, the shift mask, the maps."""
    B, H, W = 4, 16, 24
    g = torch.Generator().manual_seed(5)
    ca = R.BCase("attn", B, H, W, shift)
    cp = R.BCase("proj", B, H, W, shift, rs)
    cm = R.BCase("mlp_fwd", B, H, W, shift, rs)
    ia, ip, im = R.make_inputs(ca), R.make_inputs(cp), R.make_inputs(cm)
    dbl = lambda d: {k: v.double() for k, v in d.items()}
    ia, ip, im = dbl(ia), dbl(ip), dbl(im)
    x = torch.zeros(B * H * W, CP, dtype=torch.float64)
    x[:, :C] = torch.randn(B * H * W, C, generator=g, dtype=torch.float64)
    n1w, n1b = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64), 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    # the oracle's state dict from the packed operands (pads dropped)
    wq = ia["wqkv"].view(3, NH, DP, CP)[:, :, :D, :C].reshape(3 * C, C)
    bq = ia["bqkv"].view(3, NH, DP)[:, :, :D].reshape(3 * C)
    wp = ip["w"].view(CP, NH, DP)[:C, :, :D].reshape(C, C)
    sd = {"norm1.weight": n1w, "norm1.bias": n1b, "attn.qkv.weight": wq, "attn.qkv.bias": bq, "attn.relative_position_bias_table": ia["table"],
          "attn.proj.weight": wp, "attn.proj.bias": ip["b"][:C], "norm2.weight": ip["gamma"][:C], "norm2.bias": ip["beta"][:C],
          "mlp.fc1.weight": im["w1"][:HID, :C], "mlp.fc1.bias": im["b1"][:HID], "mlp.fc2.weight": im["w2"][:C, :HID], "mlp.fc2.bias": im["b2"][:C]}
    f = R.rowscale(cp)
    keep = None if f is None else torch.stack([f.double(), f.double()])
    want = O.swin_block(x[:, :C].view(B, H * W, C), (H, W), sd, "", NH, 8, shift, keep, qk_scale=R.SCALE).reshape(-1, C)
    # the chain of restatements
    xn1 = torch.zeros_like(x)
    xn1[:, :C] = F.layer_norm(x[:, :C], (C,), n1w, n1b, 1e-5)
    ia["xn"] = xn1[R.win_to_token(B, H, W, shift)]
    qkv = R.attn_qkv(ca, ia, R.SCALE).ref
    ip["ao"] = R.attn_out(ca, ia, qkv).ref
    ip["res"] = x
    x1 = R.proj_residual(cp, ip)["out"].ref
    ln2 = R.ln_rows(cp, ip, x1, False)
    close(ln2["xn_out"].ref[:, :C], F.layer_norm(x1[:, :C], (C,), ip["gamma"][:C], ip["beta"][:C], 1e-5))
    im["xn"], im["res"] = ln2["xn_out"].ref, x1
    s1 = R.mlp_fwd_stage1(cm, im)
    close(s1["u"].ref[:, :HID], F.linear(im["xn"][:, :C], im["w1"][:HID, :C], im["b1"][:HID]))
    close(s1["h"].ref, F.gelu(s1["u"].ref))
    x2 = R.mlp_fwd_stage2(cm, im, s1["h"].ref)["out"].ref
    close(x2[:, :C], want, 1e-10)
    assert float(x2[:, C:].abs().max()) == 0.0
    if rs == "mix":       # a dropped sample passes through both branches untouched
        drop = R.row_factor(cp, torch.arange(cp.M))[:, 0] == 0
        assert bool(drop.any()) and torch.equal(x2[drop], x[drop])
    # the next block's norm1 in window order of ITS geometry
    nxt = R.ln_rows(cm, im, x2, True)
    tok = R.win_to_token(B, H, W, shift)
    close(nxt["xn_out"].ref[:, :C], F.layer_norm(x2[:, :C], (C,), im["gamma"][:C], im["beta"][:C], 1e-5)[tok])
    close(nxt["xn_mean"].ref[:, 0], x2[:, :C].mean(1)[tok])
    close(nxt["xn_rstd"].ref[:, 0], (x2[:, :C].var(1, unbiased=False) + 1e-5).rsqrt()[tok])
    # the attention alone against the oracle's WindowAttention with an identity output projection
    sd_a = dict(sd)
    sd_a["attn.proj.weight"], sd_a["attn.proj.bias"] = torch.eye(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    mask = torch.from_numpy(O.shift_attn_mask(H, W, 8, shift)).double() if shift else None
    ao = O.window_attention(ia["xn"][:, :C].view(-1, 64, C), sd_a, "attn.", NH, 8, mask, qk_scale=R.SCALE).reshape(-1, NH, D)
    close(ip["ao"].view(-1, NH, DP)[..., :D], ao)


def test_stored_gelu_derivative_is_autograd_of_gelu():
    c = R.BCase("mlp_fwd", 1, 8, 8, dg=1)
    inp = R.make_inputs(c)
    s1 = R.mlp_fwd_stage1(c, inp)
    u = R.mlp_fwd_stage1(R.with_(c, dg=0), inp)["u"].ref.clone().requires_grad_(True)
    (gu,) = torch.autograd.grad(F.gelu(u).sum(), u)
    close(s1["u"].ref, gu)
    x = torch.linspace(-8, 8, 160001, dtype=torch.float64).requires_grad_(True)
    (g2,) = torch.autograd.grad(R.dgelu(x).sum(), x)
    assert 0.7978 < float(g2.abs().max()) <= R.DGELU_LIP


@pytest.mark.parametrize("dg", [0, 1])
@pytest.mark.parametrize("shift,rs", [(0, "none"), (4, "mix")])
def test_mlp_backward_restatement_is_autograd(shift, rs, dg):
    c = R.BCase("mlp_bwd", 3, 16, 24, shift, rs, dg=dg)
    inp = {k: v.double() for k, v in R.make_inputs(c).items()}
    _exact_ln_stats(inp)
    x = inp["ln_x"][:, :C].clone().requires_grad_(True)
    gam = inp["ln_gamma"][:C].clone().requires_grad_(True)
    bet = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    w1, w2 = inp["w1t"].t()[:HID, :C], inp["w2t"].t()[:C, :HID]            # fc1.weight [360][180], fc2.weight [180][360]
    b1 = 0.1 * torch.randn(HID, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    u = F.linear(F.layer_norm(x, (C,), gam, bet, 1e-5), w1, b1)
    y = F.linear(F.gelu(u), w2)
    g = inp["g"][:, :C]
    dx, dgam, dbet = torch.autograd.grad(y, (x, gam, bet), g)
    inp["u"] = torch.zeros(c.M, HP, dtype=torch.float64)
    inp["u"][:, :HID] = u.detach()
    inp["udg"] = R.dgelu(inp["u"])
    du = R.mlp_bwd_stage1(c, inp)["du"].ref
    out = R.mlp_bwd_stage2(c, inp, du)
    close(out["gx"].ref[:, :C], inp["gx0"][:, :C] + dx)
    assert torch.equal(out["gx"].ref[:, C:], inp["gx0"][:, C:])
    close(out["dgamma"].ref[0], inp["dgamma0"] + dgam)
    close(out["dbeta"].ref[0], inp["dbeta0"] + dbet)
    f = R.row_factor(c, torch.arange(c.M))
    close(out["gxb"].ref, (out["gx"].ref * f)[R.win_to_token(c.B, c.H, c.W, shift)])


@pytest.mark.parametrize("shift,rs,skip", [(0, "none", False), (4, "mix", False), (4, "mix", True), (0, "ones", True)])
def test_qkv_dgrad_lnbwd_restatement_is_autograd(shift, rs, skip):
    c = R.BCase("lnbwd", 3, 16, 24, shift, rs, skip=skip)
    inp = {k: v.double() for k, v in R.make_inputs(c).items()}
    tok = R.win_to_token(c.B, c.H, c.W, shift)
    _exact_ln_stats(inp, tok)                                              # the statistics are stored in window order
    x = inp["ln_x"][:, :C].clone().requires_grad_(True)
    gam = inp["ln_gamma"][:C].clone().requires_grad_(True)
    bet = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    wqkv = inp["wt"].t()[:, :C]                                            # qkv.weight [576][180]
    y = F.linear(F.layer_norm(x, (C,), gam, bet, 1e-5)[tok], wqkv)         # norm1 -> roll + partition -> qkv projection
    dx, dgam, dbet = torch.autograd.grad(y, (x, gam, bet), inp["dqkv"])
    out = R.qkv_dgrad_lnbwd(c, inp)
    total = inp["gx0"][:, :C] + dx + (inp["skip0"][:, :C] if skip else 0)
    close(out["skip" if skip else "gx"].ref[:, :C], total)
    if skip:
        assert torch.equal(out["gx"].ref, inp["gx0"]) and float(out["gx"].tol.max()) == 0.0
    close(out["dgamma"].ref[0], inp["dgamma0"] + dgam)
    close(out["dbeta"].ref[0], inp["dbeta0"] + dbet)
    close(out["gxb"].ref[:, :C], total * R.row_factor(c, torch.arange(c.M)))


def test_case_matrix():
    cs = R.all_cases(256)
    ids = [c.id for c in cs]
    assert len(ids) == len(set(ids))
    assert R.row_shapes(256) == [(4, 64, 64), (13, 32, 40), (33, 24, 24), (1, 128, 136)]
    assert [B * H * W // 64 for B, H, W in R.row_shapes(256)] == [256, 260, 297, 272]
    assert R.attn_shapes(256) == [(4, 64, 64), (257, 8, 8), (13, 32, 40), (7, 64, 72), (11, 64, 72)]
    for n in (64, 104, 256, 304):
        assert all(B * H * W >= 64 * (n & ~7) for B, H, W in R.row_shapes(n))
        assert all(B * H * W // 64 >= n for B, H, W in R.attn_shapes(n))
        B, H, W = R.attn_shapes(n)[-1]
        assert B * H * W // 64 >= 3 * n + 5 and (B * H * W // 64) // n >= 3        # every workgroup walks at least 3 windows: the steady state
        assert [R.for_device(c, n).kind for c in cs] == [c.kind for c in cs]
    for kind in R.KINDS:
        fam = [c for c in cs if c.kind == kind and not c.small]
        assert {(c.B, c.H, c.W) for c in fam} == set(R.row_shapes(256))
        assert {(c.shift, c.rs) for c in fam} == {(s, r) for s in (0, 4) for r in R.ROWSCALES}
        assert all(c.rps % 64 == 0 and c.M % c.rps == 0 for c in fam)
        assert all(R.stream_path(c, 256, False) == "tile" for c in fam)
        # the streaming kernel serves a rowscale only where a sample is an image: the one-image shape with 8 W rows per sample is the tile kernel's
        assert all((R.stream_path(c, 256, True) == "tile") == (c.rs != "none" and c.rps != c.H * c.W) for c in fam)
        assert any(c.rs == "mix" and c.rps == 8 * c.W for c in fam)
    assert {c.dg for c in cs if c.kind == "mlp_fwd"} == {0, 1} == {c.dg for c in cs if c.kind == "mlp_bwd"}
    ln = [c for c in cs if c.kind == "lnbwd"]
    assert any(c.skip for c in ln) and any(not c.skip for c in ln) and any(c.skip and c.rs == "mix" for c in ln)
    small = [c for c in cs if c.small]
    assert {c.kind for c in small} == {"proj", "lnbwd"} and all(c.M == 64 * 5 and R.stream_path(c, 256, True) == "tile" for c in small)
    at = [c for c in cs if c.kind == "attn"]
    assert {(c.B, c.H, c.W, c.shift, c.lda) for c in at} == {(B, H, W, s, l) for B, H, W in R.attn_shapes(256) for s in (0, 4) for l in (192, 200)}
    mix = R.rowscale(R.BCase("proj", 13, 32, 40, 0, "mix"))
    assert set(mix.tolist()) == {0.0, R.KEEP} and R.rowscale(R.BCase("proj", 13, 32, 40, 0, "none")) is None


_ALL = R.all_cases(256)
_shape = {}


def _shape_inputs(c):
    if _shape.get("key") != c.shape_key:
        _shape.clear()
        inp = R.make_inputs(c)
        _shape.update(key=c.shape_key, inp=inp, core=R.CORES[c.kind](inp))
    return _shape["inp"], _shape["core"]


@pytest.mark.parametrize("c", _ALL, ids=lambda c: c.id)
def test_negative_controls_are_rejected_at_every_case(c):
    """The comparator must be able to fail: each deliberately wrong restatement, rounded to the output's format as a kernel would, is
    rejected by the derived tolerance at every case where the control applies; the reference itself, rounded, is accepted, stays finite
    and its tolerance is never negative (0 where bit equality is the contract: pads, dropped samples, the untouched outf)."""
    inp, core = _shape_inputs(c)
    ref = R.host_outputs(c, inp, core)
    for name, o in ref.items():
        assert bool(torch.isfinite(o.ref).all()) and bool(torch.isfinite(o.tol).all()) and float(o.tol.min()) >= 0.0, name
        assert float(o.tol.max()) > 0.0 or (c.skip and name == "gx"), name
        ok, ratio = R.compare(o.rounded(), o)
        assert ok, (name, ratio)
    controls = R.controls_for(c)
    assert controls
    accepted = []
    for label, v in controls.items():
        wrong = R.host_outputs(c, inp, core, v)
        if all(R.compare(wrong[name].rounded(), ref[name])[0] for name in ref):
            accepted.append(label)
    assert not accepted, accepted


def test_every_control_of_the_issue_is_exercised():
    labels = set()
    for c in _ALL:
        labels |= set(R.controls_for(c))
    assert labels == {"shift applied with the wrong sign", "H and W swapped in the row map", "rowscale of the neighbouring sample",
                      "LayerNorm over 192 instead of 180", "gelu' of the rounded u", "mask dropped", "bias table transposed",
                      "q scale applied after the rounding", "ln_skip added into outf"}


NEW = ("srk_mlp_fused_fwd_ex", "srk_mlp_fused_bwd_ex", "srk_mlp_fused_launches", "srk_qkv_window_attention_fwd", "srk_qkv_attn_fwd3_launches",
       "srk_qkv_attn_fwd8_launches", "srk_proj_residual_fwd", "srk_qkv_dgrad_lnbwd", "srk_gemm_stream_launches")


def test_new_entry_points_are_declared_bound_and_check_their_arguments_on_the_host():
    """Every call here returns on the host before any launch; the addresses are dummies that are never dereferenced."""
    import ctypes as Ct

    from tpu_superresolution_amd import _lib, build
    build.build(verbose=False)
    names, h = _lib.declared_symbols(), _lib.lib()
    for n in NEW:
        assert n in names and n in _lib._SIGNATURES and hasattr(h, n), n
    assert h.srk_mlp_fused_launches(0, 1) >= 0 and h.srk_qkv_attn_fwd3_launches() >= 0 and h.srk_qkv_attn_fwd8_launches() >= 0
    a = [Ct.c_void_p((i + 1) << 20) for i in range(16)]
    g = lambda H, W, s: Ct.byref(_lib.WinGeom(H, W, s))
    E_SHAPE, E_NULL, E_ALIGN = -1, -2, -5
    fwd = lambda **k: h.srk_mlp_fused_fwd_ex(k.get("xn", a[0]), a[1], a[2], a[3], a[4], a[5], a[6], a[7], k.get("u", a[8]), k.get("h", a[9]), 0,
                                             k.get("xnn", a[10]), a[11], a[12], a[13], a[14], 180, k.get("geom"), k.get("f"), k.get("rps", 0),
                                             k.get("M", 64 * 64 * 4), None)
    assert fwd(xn=None) == E_NULL and fwd(h=None) == E_NULL and fwd(u=None) == E_NULL
    assert fwd(xn=Ct.c_void_p((1 << 20) + 8)) == E_ALIGN
    assert fwd(geom=g(64, 60, 0)) == E_SHAPE and fwd(geom=g(64, 64, 3)) == E_SHAPE and fwd(geom=g(64, 64, 4), M=64 * 64 * 4 + 64) == E_SHAPE
    assert fwd(xnn=None, geom=g(64, 64, 0)) == E_NULL
    assert fwd(f=a[15], rps=0) == E_SHAPE and fwd(f=a[15], rps=5000) == E_SHAPE
    bwd = lambda **k: h.srk_mlp_fused_bwd_ex(k.get("g", a[0]), a[1], a[2], 1, a[3], a[4], a[5], a[6], a[7], a[8], a[9], k.get("gxb", a[10]),
                                             k.get("geom"), None, 0, a[11], a[12], k.get("C", 180), 64 * 64 * 4, None)
    assert bwd(g=None) == E_NULL and bwd(C=200) == E_SHAPE and bwd(geom=g(64, 64, 2)) == E_SHAPE and bwd(gxb=None, geom=g(64, 64, 4)) == E_NULL
    att = lambda **k: h.srk_qkv_window_attention_fwd(k.get("xn", a[0]), k.get("lda", 192), a[1], a[2], 0.18, a[3], a[4], a[5], k.get("B_", 256), 6,
                                                     k.get("geom", g(64, 64, 4)), None)
    assert att(xn=None) == E_NULL and att(lda=196) == E_SHAPE and att(lda=128) == E_SHAPE and att(B_=255) == E_SHAPE and att(geom=g(64, 64, 1)) == E_SHAPE
    prj = lambda **k: h.srk_proj_residual_fwd(k.get("ao", a[0]), a[1], a[2], a[3], k.get("out", a[4]), k.get("f"), k.get("rps", 0), k.get("xn", None), None, None, None, None,
                                              180, k.get("B_", 256), k.get("geom", g(64, 64, 4)), None)
    assert prj(ao=None) == E_NULL and prj(out=a[3]) == E_SHAPE and prj(B_=100) == E_SHAPE and prj(xn=a[5]) == E_NULL
    assert prj(f=a[15], rps=0) == E_SHAPE and prj(f=a[15], rps=5000) == E_SHAPE
    lnb = lambda **k: h.srk_qkv_dgrad_lnbwd(k.get("d", a[0]), a[1], a[2], a[3], a[4], a[5], a[6], a[7], k.get("f"), k.get("rps", 0), k.get("skip", None), a[8], a[9],
                                            k.get("C", 180), k.get("B_", 256), k.get("geom", g(64, 64, 0)), None)
    assert lnb(d=None) == E_NULL and lnb(skip=a[6]) == E_SHAPE and lnb(C=0) == E_SHAPE and lnb(geom=g(72, 64, 0)) == E_SHAPE
    assert b"multiple of H*W" in h.srk_last_error()
    assert lnb(f=a[15], rps=0) == E_SHAPE and lnb(f=a[15], rps=5000) == E_SHAPE
