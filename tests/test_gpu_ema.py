"""EMA of the weights inside the fused clip + AdamW step (csrc/adamw.h adamw_ema_elem; srk_adamw_clip_ema_step, srk_multi_adamw_clip_ema_step)
and everything built on it: optim.FusedAdamW(ema_decay=..), swap_ema(), ema_state_dict(), finetune_swinir --ema_decay, the 'params_ema'
checkpoint envelope.

Bounds.  Step unchanged / flat = multi / gate / resume / capture: bit for bit.  Value of the average after k steps against an fp64
restatement e <- D e + (1 - D) p_k (D the decimal, p_k the weights the kernel produced, cast to fp64): each step adds at most 4
roundings of size u = 2^-24 relative to M = max(|e|, |p|) (the fp32 decay constant, two products, one sum) and earlier error is
multiplied by decay < 1, so |err| <= 4 k u M per element; M is taken per element as the largest |e| or |p| met on the way.  Eval forward
on the averaged weights against the CPU oracle: 1.2e-2 * max|ref|, the bound of the models' inference tests."""
import io
import os

import pytest
import torch

from oracle import swinir_oracle as SO
from test_gpu_fused_optim import SIZES, _arch, _bag, _case, _same, _set_grads, _to_gpu, make_dataset
from test_oracle_golden import tiny_weights

pytestmark = pytest.mark.gpu

HYPER = dict(lr=2e-3, wd=0.01, max_norm=1.0, grad_div=2.0)
U = 2.0 ** -24
EMA_ODD = 5          # a tensor whose average alone sits at a 4-byte-aligned address (weights, gradient and moments are 16-byte aligned)


def _table(ops, p, g, m, v, e=None):
    tab = ops.TensorTable(len(p))
    tab.set("params", p, first=True)
    tab.set("grads", g)
    tab.set("exp_avg", m)
    tab.set("exp_avg_sq", v)
    if e is not None:
        tab.set("ema", e)
    return tab


def _run(params, grads, odd, decay):
    """len(grads) steps of the multi-tensor EMA call on separate allocations.  After every step: params / exp_avg / exp_avg_sq equal
    those of the call without EMA (multi and flat) and the average equals the one of the flat EMA call on the concatenated layout, bit
    for bit.  -> (weights after every step, final average), fp64 CPU lists."""
    from tpu_superresolution_amd import ops
    h = HYPER
    sizes = [t.numel() for t in params]
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).cuda()          # noqa: E731
    # A: multi + EMA, B: multi as it was, C: flat + EMA, D: flat as it was
    pa, pb = _to_gpu(params, odd), _to_gpu(params, odd)
    ea = _to_gpu(params, odd)
    base = torch.zeros(params[EMA_ODD].numel() + 1, device="cuda")
    ea[EMA_ODD] = base[1:].view(params[EMA_ODD].shape)
    ea[EMA_ODD].copy_(params[EMA_ODD])
    assert ea[EMA_ODD].data_ptr() % 16 == 4 and pa[EMA_ODD].data_ptr() % 16 == 0
    ma, va = [torch.zeros_like(t) for t in pa], [torch.zeros_like(t) for t in pa]
    mb, vb = [torch.zeros_like(t) for t in pb], [torch.zeros_like(t) for t in pb]
    pc, pd = cat(params), cat(params)
    ec = cat(params)
    mc, vc, md, vd = (torch.zeros_like(pc) for _ in range(4))
    sumsq = torch.zeros(1, device="cuda")
    trail = []
    for k, gs in enumerate(grads):
        g, fg = _to_gpu(gs, odd), cat(gs)
        sumsq.zero_()
        ops.multi_grad_sumsq(_table(ops, pb, g, mb, vb), sumsq)
        args = (sumsq, h["max_norm"], h["grad_div"], h["lr"], 0.9, 0.999, 1e-8, h["wd"], k + 1)
        ops.multi_adamw_clip_step(_table(ops, pa, g, ma, va, ea), *args, ema_decay=decay)
        ops.multi_adamw_clip_step(_table(ops, pb, g, mb, vb), *args)
        ops.adamw_clip_step(pc, fg, mc, vc, *args, ema=ec, ema_decay=decay)
        ops.adamw_clip_step(pd, fg, md, vd, *args)
        for name, x, y, fx, fy in (("param", pa, pb, pc, pd), ("exp_avg", ma, mb, mc, md), ("exp_avg_sq", va, vb, vc, vd)):
            assert torch.equal(fx, fy), f"step {k + 1}: flat {name} differs between the EMA call and the call without"
            for i, (a, b, c) in enumerate(zip(x, y, fx.split(sizes))):
                assert torch.equal(a, b), f"step {k + 1}: {name}[{i}] differs between the EMA call and the call without"
                assert torch.equal(a.reshape(-1), c), f"step {k + 1}: {name}[{i}] differs from the flat EMA call"
        for i, (a, c) in enumerate(zip(ea, ec.split(sizes))):
            assert torch.equal(a.reshape(-1), c), f"step {k + 1}: ema[{i}] differs between the multi-tensor and the flat call"
        trail.append([t.double().cpu() for t in pa])
    assert float(base[0]) == 0.0          # the float in front of the unaligned average was not written
    return trail, [t.double().cpu() for t in ea]


@pytest.mark.parametrize("many", [0, 200])
def test_ema_calls_leave_the_step_unchanged_and_flat_equals_multi_bit_for_bit(many):
    """Awkward sizes, one tensor at a 4-byte-aligned address, one tensor whose average alone is unaligned and, many=200, more tensors
    than one launch of the EMA table holds (chunks of 72; 80 without EMA): 3 steps, every bit of params, both moments and the
    average."""
    params, grads, odd = _case(seed=many, many=many)
    assert len(params) == len(SIZES) + 1 + many
    _run(params, grads, odd, 0.999)


@pytest.mark.parametrize("decay,many", [(0.999, 0), (0.999, 200), (0.9, 0)])
def test_ema_value_after_five_steps_vs_fp64(decay, many):
    """|err| <= 4 k u M per element, k = 5 (derivation in the module docstring; not tuned).

    Measured on MI355X (max over all elements of err, and of err / bound):
      decay 0.999, many 0:    err 5.43e-08   ratio 0.371
      decay 0.999, many 200:  err 4.76e-08   ratio 0.414
      decay 0.9,   many 0:    err 4.84e-08   ratio 0.322"""
    k = 5
    params, grads, odd = _case(seed=many, steps=k, many=many)
    trail, got = _run(params, grads, odd, decay)
    worst_err, worst_ratio = 0.0, 0.0
    for i, p0 in enumerate(params):
        e = p0.double()
        big = e.abs()
        for step in range(k):
            pk = trail[step][i]
            e = decay * e + (1.0 - decay) * pk
            big = torch.maximum(big, torch.maximum(e.abs(), pk.abs()))
        err, bound = (got[i] - e).abs().reshape(-1), (4 * k * U * big).reshape(-1)
        worst_err = max(worst_err, float(err.max()))
        worst_ratio = max(worst_ratio, float((err / bound.clamp_min(1e-300)).max()))
        at = int((err - bound).argmax())
        assert bool((err <= bound).all()), f"ema[{i}][{at}]: err {float(err[at]):.3e} > bound {float(bound[at]):.3e}"
    print(f"[decay={decay} many={many}] ema after {k} steps: max err {worst_err:.3e}, max err / bound {worst_ratio:.3f}")


def test_ema_decay_zero_copies_the_weights():
    params, grads, odd = _case(seed=3, steps=2)
    trail, got = _run(params, grads, odd, 0.0)
    assert all(torch.equal(a, b) for a, b in zip(got, trail[-1]))


# ---- FusedAdamW ---------------------------------------------------------------------------------------------------------------------
def _snap(net, opt):
    ps = [p for p in net.parameters() if p in opt.state]
    return ([p.detach().clone() for p in net.parameters()], [opt.state[p]["exp_avg"].clone() for p in ps],
            [opt.state[p]["exp_avg_sq"].clone() for p in ps], [opt.state[p]["ema"].clone() for p in ps])


KINDS4 = ("param", "exp_avg", "exp_avg_sq", "ema")


def _frac_moved(a, b):
    return sum(not torch.equal(x, y) for x, y in zip(a, b)) / len(a)


def test_gate_leaves_the_average_untouched_and_lr_zero_still_advances_it():
    from tpu_superresolution_amd.optim import FusedAdamW
    net, grads = _bag()
    opt = FusedAdamW(net, lr=2e-3, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9)
    _set_grads(net, grads[0])
    opt.step()                                         # moments are non-zero and the average differs from the weights from here on
    before = _snap(net, opt)
    assert all(not torch.equal(p, e) for p, e in zip(before[0], before[3]))
    one, zero = torch.ones(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    _set_grads(net, grads[1])
    opt.step(nonfinite=one)
    assert _same(_snap(net, opt), before)
    _set_grads(net, grads[1])
    list(net.parameters())[4].grad[7] = float("inf")
    opt.step(nonfinite=zero)
    assert _same(_snap(net, opt), before)
    _set_grads(net, grads[1])
    list(net.parameters())[6].grad[0, 3] = float("nan")
    opt.step()
    assert _same(_snap(net, opt), before)
    _set_grads(net, grads[1])
    opt.step(nonfinite=zero)
    after = _snap(net, opt)
    for kind, a, b in zip(KINDS4, after, before):
        for i, (x, y) in enumerate(zip(a, b)):
            assert not torch.equal(x, y), f"{kind}[{i}] did not move"
    # lr = 0 without decay: the weights stay, the average goes on toward them
    opt.param_groups[0]["lr"], opt.param_groups[0]["weight_decay"] = 0.0, 0.0
    _set_grads(net, grads[2])
    opt.step()
    still = _snap(net, opt)
    assert all(torch.equal(x, y) for x, y in zip(still[0], after[0]))
    for i, (e1, e0, p) in enumerate(zip(still[3], after[3], after[0])):
        assert not torch.equal(e1, e0), f"ema[{i}] did not advance"
        assert float((e1 - p).abs().max()) < float((e0 - p).abs().max()), f"ema[{i}] did not come closer to the weights"


def test_frozen_and_gradless_parameters_and_the_average():
    from tpu_superresolution_amd.optim import FusedAdamW
    net, grads = _bag()
    ps = list(net.parameters())
    names = [n for n, _ in net.named_parameters()]
    ps[2].requires_grad = False
    opt = FusedAdamW(net, lr=2e-3, weight_decay=0.0, max_grad_norm=None, ema_decay=0.9)
    _set_grads(net, grads[0])
    ps[2].grad = None
    opt.step()
    assert ps[2] not in opt.state or "ema" not in opt.state[ps[2]]
    e5 = opt.state[ps[5]]["ema"].clone()
    _set_grads(net, grads[1])
    ps[2].grad = None
    ps[5].grad = None                                  # trainable, but no gradient this step
    opt.step()
    assert torch.equal(opt.state[ps[5]]["ema"], e5), "a parameter the step skipped advanced its average"
    esd = opt.ema_state_dict()
    assert list(esd) == list(net.state_dict()) and all(not v.is_cuda for v in esd.values())
    assert torch.equal(esd[names[2]], ps[2].detach().cpu())
    for i in (0, 4, 5):
        assert torch.equal(esd[names[i]], opt.state[ps[i]]["ema"].cpu()) and not torch.equal(esd[names[i]], ps[i].detach().cpu())


def _roundtrip(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=False)


def test_state_dict_resume_with_ema_continues_bit_identically():
    from tpu_superresolution_amd.optim import FusedAdamW
    kw = dict(lr=2e-3, weight_decay=0.01, max_grad_norm=1.0, grad_div=2.0, ema_decay=0.999)
    na, grads = _bag()
    nb, _ = _bag()
    oa, ob = FusedAdamW(na, **kw), FusedAdamW(nb, **kw)
    for k in range(2):
        for net, opt in ((na, oa), (nb, ob)):
            _set_grads(net, grads[k])
            opt.step()
    sd = _roundtrip(ob.state_dict())
    assert all("ema" in st for st in sd["state"].values())
    oc = FusedAdamW(nb, **kw)
    oc.load_state_dict(sd)
    for k in range(2, 4):
        for net, opt in ((na, oa), (nb, oc)):
            _set_grads(net, grads[k])
            opt.step()
    assert _same(_snap(na, oa), _snap(nb, oc))
    # a state without an average (written by an optimizer that ran without ema_decay): the average starts from the current weights
    sd = _roundtrip(oc.state_dict())
    for st in sd["state"].values():
        del st["ema"]
    del sd["fused"]["ema"]
    od = FusedAdamW(nb, **kw)
    od.load_state_dict(sd)
    now = _snap(nb, oc)
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    _set_grads(nb, grads[0])
    od.step(nonfinite=one)                             # gated: allocates the missing state, moves nothing
    got = _snap(nb, od)
    assert _same(got[:3], now[:3]) and all(torch.equal(e, w) for e, w in zip(got[3], now[0]))


def _tiny_swinir(train=True):
    import tpu_superresolution_amd as T
    g, cfg, sd = tiny_weights("ps4")
    m = T.SwinIR(drop_path_rate=0.0, **cfg.kwargs())
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    return (m.train() if train else m.eval()), cfg, torch.from_numpy(g["x_16x16"]).cuda()


def _flat_step(m, opt, seed):
    """One optimizer step of the flat path on a gradient written straight into the engine's flat gradient buffer (the backward's
    atomics would make two runs differ in the last bits; the resume comparison is about the optimizer)."""
    eng = m._engine
    g = eng.ensure_grad()
    g.copy_(0.01 * torch.randn(g.shape, generator=torch.Generator().manual_seed(seed)).cuda())
    opt.step()


def test_flat_path_resume_with_ema_continues_bit_identically():
    from tpu_superresolution_amd.optim import FusedAdamW
    # no clipping: the sum of squares over a range of this size is added up by atomics in an order that differs from run to run, and
    # with it the last bits of the clip coefficient (the norm still gates the step); everything else in the step is deterministic
    kw = dict(lr=2e-3, weight_decay=0.01, max_grad_norm=None, ema_decay=0.999)
    (ma, _, x), (mb, _, _) = _tiny_swinir(), _tiny_swinir()
    frozen = [n for n, _ in ma.named_parameters() if "conv_first" in n]
    for m in (ma, mb):
        for n, p in m.named_parameters():
            p.requires_grad = n not in frozen
        with torch.no_grad():
            m(x)                                       # binds the engine: the parameters become views of the flat buffer
    oa, ob = FusedAdamW(ma, **kw), FusedAdamW(mb, **kw)
    for k in range(2):
        _flat_step(ma, oa, k)
        _flat_step(mb, ob, k)
    sd = _roundtrip(ob.state_dict())
    assert sd["fused"]["ema"] is not None and sd["fused"]["step"] == 2
    oc = FusedAdamW(mb, **kw)
    oc.load_state_dict(sd)
    for k in range(2, 4):
        _flat_step(ma, oa, k)
        _flat_step(mb, oc, k)
    for a, b in ((ma._engine.flat, mb._engine.flat), (oa._m, oc._m), (oa._v, oc._v), (oa._ema, oc._ema)):
        assert torch.equal(a, b)
    assert not torch.equal(oa._ema, ma._engine.flat)
    # frozen ranges are never stepped: there the average stays equal to the weights, and ema_state_dict() hands out the weight
    esd, live = oa.ema_state_dict(), ma.state_dict()
    assert list(esd) == list(live)
    for n in frozen:
        assert torch.equal(esd[n], live[n].cpu()), n
    moved = [n for n, p in ma.named_parameters() if n not in frozen and not torch.equal(esd[n], live[n].cpu())]
    assert len(moved) >= 0.8 * (len(list(ma.parameters())) - len(frozen))


def test_captured_ema_step_follows_step_count_and_learning_rate_bit_for_bit():
    """The pattern of test_captured_step_follows_step_count_and_learning_rate_bit_for_bit with the average switched on: replays equal
    eager steps exactly, the average included, also across a learning-rate change."""
    from tpu_superresolution_amd.optim import FusedAdamW
    kw = dict(lr=2e-3, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.999)
    na, grads = _bag(steps=5)
    nb, _ = _bag(steps=5)
    oa, ob = FusedAdamW(na, **kw), FusedAdamW(nb, **kw)
    static = [g.clone() for g in grads[0]]
    for p, g in zip(nb.parameters(), static):
        p.grad = g                                     # the captured launch reads these buffers
    _set_grads(na, grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()
        ob.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.step()
    assert ob._step == 1, "capturing must not count as a step"
    for k in range(1, 5):
        if k == 3:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 5e-4
        _set_grads(na, grads[k])
        oa.step()
        for s, g in zip(static, grads[k]):
            s.copy_(g)
        ob.begin_replay()
        graph.replay()
        ob.end_replay()
        assert ob._step == k + 1
        assert _same(_snap(na, oa), _snap(nb, ob)), f"replay {k} differs from the eager step"
    weights, _, _, avg = _snap(nb, ob)
    assert all(not torch.equal(e, p) for p, e in zip(weights, avg))


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _model_case(arch):
    """-> (training model, batches, oracle(state_dict, x on the CPU))"""
    if arch == "swinir":
        m, cfg, x = _tiny_swinir()
        gen = torch.Generator().manual_seed(9)
        batches = [(x if k == 0 else torch.rand(x.shape, generator=gen).cuda(),
                    torch.rand(x.shape[0], 3, x.shape[2] * cfg.upscale, x.shape[3] * cfg.upscale, generator=gen).cuda()) for k in range(4)]
        return m, batches, lambda s, xx: SO.swinir_forward(s, cfg, xx)
    make, _, batches, _, oracle = _arch(arch)
    return make(), batches, oracle


def _opt_snapshot(m, opt):
    if opt._flat:
        return [m._engine.flat.clone(), opt._m.clone(), opt._v.clone(), opt._ema.clone()]
    return [t for kind in _snap(m, opt) for t in kind] + [b.clone() for b in m.buffers()]


def _eval_forward(m, x):
    assert not m.training
    with torch.no_grad():
        return m(x).cpu()


@pytest.mark.parametrize("arch", ["swinir", "hat", "dat"])
def test_swap_ema_runs_the_model_on_the_average_and_undoes_itself(arch):
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import train_step
    m, batches, oracle = _model_case(arch)
    opt = FusedAdamW(m, lr=5e-3, weight_decay=0.0, max_grad_norm=1.0, ema_decay=0.9)
    for x, t in batches[:3]:
        _, bad = train_step(m, opt, x, t)
        assert int(bad) == 0
    x = batches[0][0]
    m.eval()                                           # once: no mode switch below refreshes a pack behind swap_ema()'s back
    y_raw = _eval_forward(m, x)                        # fills the bf16 pack cache with the raw weights
    before = _opt_snapshot(m, opt)
    esd = opt.ema_state_dict()
    assert list(esd) == list(m.state_dict())
    with torch.no_grad():
        ref = oracle(esd, x.cpu())
    with opt.swap_ema():
        y_ema = _eval_forward(m, x)
        inside = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt.step()
    assert all(torch.equal(inside[k], esd[k]) for k in esd), "inside swap_ema() the model does not hold the average"
    err, moved = float((y_ema - ref).abs().max()), float((y_ema - y_raw).abs().max())
    print(f"{arch}: averaged vs raw output differ by {moved:.3e}; max err vs oracle on ema_state_dict() {err:.3e} "
          f"(ref max {float(ref.abs().max()):.3e}, bound {1.2e-2 * float(ref.abs().max()):.3e})")
    assert moved > 0.0, "the forward inside swap_ema() ran on a stale pack of the raw weights"
    assert err <= 1.2e-2 * float(ref.abs().max())
    y_back = _eval_forward(m, x)
    assert torch.equal(y_back, y_raw), "the forward after swap_ema() is not the one before it"
    after = _opt_snapshot(m, opt)
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(after, before))
    with pytest.raises(ZeroDivisionError):
        with opt.swap_ema():
            1 / 0
    after = _opt_snapshot(m, opt)
    assert all(torch.equal(a, b) for a, b in zip(after, before)), "an exception inside swap_ema() left the weights swapped"
    assert torch.equal(_eval_forward(m, x), y_raw)


@pytest.mark.parametrize("arch", ["hat", "dat"])
def test_graphed_train_step_gates_and_advances_the_average(arch):
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import GraphedTrainStep
    make, _, batches, lr, _ = _arch(arch)
    m = make()
    opt = FusedAdamW(m, lr=lr, weight_decay=0.0, max_grad_norm=1.0, ema_decay=0.9)
    gs = GraphedTrainStep(m, opt, warmup=1)
    for x, t in batches[:2]:
        _, bad = gs(x, t)
        assert int(bad) == 0
    ps = list(m.parameters())
    before = _snap(m, opt)
    x, t = batches[1]
    xbad = x.clone()
    xbad[0, 1, 5, 7] = float("nan")
    _, bad = gs(xbad, t)
    assert int(bad) > 0
    assert _same(_snap(m, opt), before), "a non-finite batch inside a replay changed weights, moments or the average"
    lg, bad = gs(x, t)
    assert int(bad) == 0 and bool(torch.isfinite(lg))
    after = _snap(m, opt)
    # "advances": the average after the good replay is one step of e <- D e + (1 - D) p_new from the average before it, within the
    # one-step bound of the module docstring (4 u M).  Not "every average changed": where the step moves a weight by an ulp or two (a
    # norm weight at 1.0 with a small update) a tenth of that difference rounds away and the average rightly stays where it is.
    for i in range(len(ps)):
        e0, p1, e1 = before[3][i].double(), after[0][i].double(), after[3][i].double()
        want = 0.9 * e0 + (1.0 - 0.9) * p1
        bound = 4 * U * torch.maximum(torch.maximum(e0.abs(), p1.abs()), want.abs())
        assert bool(((e1 - want).abs() <= bound).all()), f"ema[{i}] is not one step on from the average before the bad batch"
    changed = sum(not torch.equal(a, b) for a, b in zip(after[3], before[3]))
    print(f"{arch}: the good replay moved {_frac_moved(after[0], before[0]):.2f} of the weights and {changed} of {len(ps)} averages")
    assert changed >= len(ps) // 2, "the good batch after the bad one did not advance the average"
    assert all(bool(torch.isfinite(e).all()) for e in after[3])
    gs.close()


# ---- script -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["hat", "swinir"])
def test_finetune_script_with_ema_decay_one_epoch_and_params_ema_reload(arch, tmp_path, capsys, monkeypatch):
    from tpu_superresolution_amd import finetune_swinir as F
    from tpu_superresolution_amd.evaluate import _load_state
    make_dataset(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    base = ["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", "--lr", "1e-4", "--arch", arch]
    F.main(base + ["--ema_decay", "0.99"])
    out = capsys.readouterr().out
    assert "[X4] epoch 001/1" in out and "[done] best_val_loss=" in out
    fresh = F.build_sr_model(arch, 4).state_dict()
    for name in (f"best_{arch}_finetune_X4.pt", f"bestpsnr_{arch}_finetune_X4.pt"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=False)
        assert set(ck) >= {"model", "params_ema", "epoch", "args"} and ck["args"]["ema_decay"] == 0.99
        for key in ("model", "params_ema"):
            assert list(ck[key]) == list(fresh), key
            assert all(torch.isfinite(v).all() for v in ck[key].values() if v.is_floating_point()), key
        differ = [k for k, v in ck["model"].items() if v.is_floating_point() and v.numel() > 1 and not torch.equal(v, ck["params_ema"][k])]
        assert len(differ) > len(fresh) // 2, f"{name}: 'model' and 'params_ema' are the same in {len(fresh) - len(differ)} of {len(fresh)} tensors"
    state, msg = _load_state(str(tmp_path / f"best_{arch}_finetune_X4.pt"), "params_ema")
    assert "params_ema" in msg
    F.build_sr_model(arch, 4).load_state_dict(state, strict=True)
    assert all(torch.equal(state[k], ck["params_ema"][k]) for k in state)          # one epoch: both files hold the same one
    torch.save({"params_ema": ck["params_ema"]}, tmp_path / "w.pth")
    os.remove(tmp_path / f"best_{arch}_finetune_X4.pt")
    F.main(base + ["--weights", str(tmp_path / "w.pth")])
    out = capsys.readouterr().out
    assert "[weights] missing=0, unexpected=0" in out and "[done] best_val_loss=" in out
    plain = torch.load(tmp_path / f"best_{arch}_finetune_X4.pt", map_location="cpu", weights_only=False)
    assert "params_ema" not in plain and "ema_decay" not in plain["args"]
    assert set(plain) == {"model", "epoch", "best_val_loss", "val_psnr", "args"}
