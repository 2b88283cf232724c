"""tests/light_ref.py pinned on the CPU: the composed fp64 restatement against the oracle's swin_block, the packing against the project's,
every probe's claim in fp64, the derived bounds against a CPU emulation of the kernel (fp32 arithmetic, bf16 at the documented rounding
points), and the negative controls.  The multi-round case differs from the others only in how many windows a device holds at once; here
it runs at the shape of an 8-CU device (one 64 x 64 image)."""
import pytest
import torch

import light_ref as L
from oracle import swinir_oracle as O

CASES = [L.for_device(c, 8) if c.multi else c for c in L.cases()]
IDS = [c.id for c in L.cases()]
_memo = {}


def operands(c):
    key = (c.C, c.hid, c.B, c.H, c.W)
    if _memo.get("key") != key:
        _memo.clear()
        _memo.update(key=key, x=L.make_x(c), sd=L.make_weights(c))
    return _memo["x"], _memo["sd"]


def oracle64(c, x, sd):
    sd64 = {k: v.double() for k, v in sd.items()}
    return O.swin_block(x.double().view(c.B, c.H * c.W, c.C), (c.H, c.W), sd64, L.PRE, L.NH, 8, c.shift, qk_scale=c.scale).reshape(c.T, c.C)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_case_matrix():
    cs = L.cases()
    assert len(cs) == len({c.id for c in cs}) == 17
    assert {(c.C, c.dh, c.hid) for c in cs if (c.B, c.H, c.W) == (3, 24, 40)} == set(L.WIDTHS)
    assert {(c.B, c.H, c.W) for c in cs if (c.C, c.hid) == (60, 120) and not c.multi} == set(L.GEOMS)
    assert all(c.dh * L.NH == c.C for c in cs)
    multi = [c for c in cs if c.multi]
    assert len(multi) == 1 and multi[0].shift == 4 and multi[0].B == 13 and (multi[0].B - 1) * 64 <= 3 * 256 < multi[0].B * 64
    assert L.for_device(multi[0], 304).B * 64 > 3 * 304 >= (L.for_device(multi[0], 304).B - 1) * 64
    x = L.make_x(cs[0])
    assert float(x.abs().max()) <= 7.5 and torch.equal(x * 4096, torch.round(x * 4096))       # the grid `recover` relies on


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_composed_restatement_is_the_oracle_block(c):
    x, sd = operands(c)
    assert rel(L.composed(c, x, sd)["y"], oracle64(c, x, sd)) <= 1e-12


def test_packing_is_the_projects_packing():
    from tpu_superresolution_amd.packing import _head_map, _pack_linear, _pack_vec
    for C, dh, hid in L.WIDTHS:
        c = L.LCase(C, dh, hid, 1, 8, 8, 0)
        sd = L.make_weights(c)
        mine = L.pack_block(c, sd)
        hm = _head_map(L.NH, dh, torch.device("cpu"))
        assert torch.equal(hm, L.head_map(L.NH, dh))
        qmap = torch.cat([w * 192 + hm for w in range(3)])
        g = lambda k: sd[L.PRE + k]
        theirs = dict(wqkv=_pack_linear(g("attn.qkv.weight"), 576, 64, row_map=qmap), bqkv=_pack_vec(g("attn.qkv.bias"), 576, row_map=qmap),
                      wproj=_pack_linear(g("attn.proj.weight"), 64, 192, col_map=hm), bproj=_pack_vec(g("attn.proj.bias"), 64),
                      w1=_pack_linear(g("mlp.fc1.weight"), 128, 64), b1=_pack_vec(g("mlp.fc1.bias"), 128),
                      w2=_pack_linear(g("mlp.fc2.weight"), 64, 128), b2=_pack_vec(g("mlp.fc2.bias"), 64),
                      dense=O.dense_rel_pos_bias(g("attn.relative_position_bias_table"), 8).contiguous().float())
        for k, t in theirs.items():
            assert mine[k].dtype == t.dtype and mine[k].shape == t.shape, k
            assert mine[k].contiguous().view(torch.uint8).equal(t.contiguous().view(torch.uint8)), (k, C)      # byte for byte
        for k in ("n1w", "n1b", "n2w", "n2b"):
            assert mine[k].shape == (64,) and torch.isnan(mine[k][C:]).all() and torch.isfinite(mine[k][:C]).all()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_probe_exposes_the_intermediate_it_claims(c):
    """In fp64 (no rounding anywhere) y - base of each probe equals the composed restatement's intermediate."""
    x, sd = operands(c)
    X, ref = x.double(), L.composed(c, x, sd)
    run = lambda name, j0=0: oracle64(c, x, L.probe(c, sd, name, j0))
    assert torch.equal(run("P0"), X)
    assert rel(run("P1") - X, ref["xn"]) <= 1e-12
    assert rel(run("P2v") - X, ref["v"]) <= 1e-12
    assert rel(run("P2k") - X, ref["k"]) <= 1e-12
    assert rel(run("P3") - X, ref["ao"]) <= 1e-12
    assert rel(run("P4"), ref["x1"]) <= 1e-12
    for j0 in range(0, c.hid, c.C):
        n = min(c.C, c.hid - j0)
        d = run("P5", j0) - ref["x1"]
        assert rel(d[:, :n], ref["h"][:, j0:j0 + n]) <= 1e-12 and float(d[:, n:].abs().max() if n < c.C else 0.0) <= 1e-12
    assert rel(run("P6"), ref["y"]) <= 1e-12


def test_recover_returns_the_bf16_value_or_a_bound():
    g = torch.Generator().manual_seed(5)
    base = (torch.round((15 * torch.rand(20000, generator=g) - 7.5) * 4096) / 4096).float()
    mag = torch.exp2(-24 * torch.rand(20000, generator=g) + 2)                  # |t| from 4 down to 2^-22
    t = (mag * torch.where(torch.rand(20000, generator=g) < 0.5, -1.0, 1.0)).to(torch.bfloat16)
    t[:64] = 0.0
    r = L.recover((base.double() + t.double()).float(), base, True)
    big = t.double().abs() >= 2.0 ** -14                                        # the sum is exact; the test may rely on it from 2^-13
    assert torch.equal(r.val[big], t.double()[big]) and bool((r.unc[t.double().abs() >= 2.0 ** -13] == 0).all())
    assert bool(((r.val - t.double()).abs() <= r.unc).all())
    assert bool((r.unc[~big] <= 2.0 ** -20).all())
    base2 = (10 * torch.randn(20000, generator=g)).float()                       # any fp32 base
    r = L.recover((base2.double() + t.double()).float(), base2, False)
    assert bool(((r.val - t.double()).abs() <= r.unc).all())
    assert bool((r.unc[t.double().abs() >= 2.0 ** -9 * base2.double().abs().clamp_min(1.0)] == 0).all())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_emulated_kernel_passes_every_stage_and_the_controls_do_not(c):
    x, sd = operands(c)
    res = L.run_stages(c, x, sd, lambda w: L.emulate(c, x, w))
    print(f"{c.id}: " + " ".join(f"{k} {res[k]:.3f}" for k in L.STAGES))
    assert set(res) == set(L.STAGES)
    assert all(res[k] <= 1.0 for k in L.STAGES), res
    for name, (v, stage) in L.controls_for(c).items():
        bad = L.run_stages(c, x, sd, lambda w: L.emulate(c, x, w, v))
        assert bad[stage] > 1.0, (name, stage, bad)
        before = L.STAGES[:L.STAGES.index(stage)]
        assert all(bad[k] <= 1.0 for k in before), (name, "an earlier stage refused it", bad)     # the control acts in ITS stage
    for name, v in L.UNDETECTABLE.items():
        bad = L.run_stages(c, x, sd, lambda w: L.emulate(c, x, w, v))
        assert all(bad[k] <= 1.0 for k in L.STAGES if k != "h") and bad["h"] < float("inf"), (name, bad)
        if c.C >= 30:           # at C = 6 the carried LayerNorm bound is six terms wide and the h comparator does refuse some elements
            assert bad["h"] <= 1.0, (name, "listed as undetectable, yet refused", bad)


def test_controls_cover_the_list():
    names = set()
    for c in CASES:
        names |= set(L.controls_for(c))
    assert len(names) == 7, names
