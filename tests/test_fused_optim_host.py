"""CPU-only checks of the multi-tensor optimizer's host side: the new C-ABI symbols exist, their argument checks answer with the
documented codes before any launch, and the fine-tuning script knows --arch / --graph."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from tpu_superresolution_amd import build
    build.build(verbose=False)
    from tpu_superresolution_amd import _lib
    return _lib


NEW = ("srk_multi_grad_sumsq", "srk_multi_adamw_clip_step", "srk_adamw_hyper")


def test_multi_tensor_symbols_are_declared_bound_and_exported(lib):
    names = lib.declared_symbols()
    handle = lib.lib()
    for n in NEW:
        assert n in names, n
        assert n in lib._SIGNATURES, n
        assert hasattr(handle, n), n


def _lists(n, fill=64):
    arr = (C.c_void_p * n)(*([fill] * n))          # never dereferenced: every call below must fail before a launch
    return arr


def test_multi_sumsq_argument_checks(lib):
    h = lib.lib()
    numel = (C.c_int64 * 2)(4, 5)
    g = _lists(2)
    assert h.srk_multi_grad_sumsq(None, numel, 2, 64, None) == -2          # SRK_E_NULL: null table
    assert b"grads" in h.srk_last_error()
    assert h.srk_multi_grad_sumsq(g, None, 2, 64, None) == -2
    assert h.srk_multi_grad_sumsq(g, numel, 2, None, None) == -2           # null sumsq
    assert h.srk_multi_grad_sumsq(g, numel, 0, 64, None) == -1             # SRK_E_SHAPE: n_tensors <= 0
    assert h.srk_multi_grad_sumsq(g, numel, -3, 64, None) == -1
    numel[1] = -1
    assert h.srk_multi_grad_sumsq(g, numel, 2, 64, None) == -1             # negative count
    assert b"numel[1]" in h.srk_last_error()
    numel[1] = 5
    g[1] = None
    assert h.srk_multi_grad_sumsq(g, numel, 2, 64, None) == -2             # null entry with a non-zero count
    assert b"grads[1]" in h.srk_last_error()


def test_multi_adamw_argument_checks(lib):
    h = lib.lib()
    numel = (C.c_int64 * 3)(4, 5, 6)
    p, g, m, v = _lists(3), _lists(3), _lists(3), _lists(3)

    def call(p=p, g=g, m=m, v=v, numel=numel, n=3, sumsq=64, max_norm=1.0, grad_div=1.0, step=1):
        return h.srk_multi_adamw_clip_step(p, g, m, v, numel, n, sumsq, max_norm, grad_div, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, None, None, None)
    for role in ("p", "g", "m", "v", "numel"):
        assert call(**{role: None}) == -2, role
    assert call(n=0) == -1 and call(n=-1) == -1
    assert call(step=0) == -1
    assert call(grad_div=0.0) == -1
    assert call(sumsq=None) == -2                      # clipping needs the sum of squares
    bad = (C.c_int64 * 3)(4, -5, 6)
    assert call(numel=bad) == -1
    hole = _lists(3)
    hole[2] = None
    assert call(m=hole) == -2
    assert b"exp_avg[2]" in h.srk_last_error()


def test_adamw_hyper_matches_the_formula(lib):
    from tpu_superresolution_amd import ops
    lr, bc1, bc2s = ops.adamw_hyper(2e-3, 0.9, 0.999, 7)
    assert lr == pytest.approx(2e-3, rel=1e-7)
    assert bc1 == pytest.approx(1 - 0.9 ** 7, rel=1e-6)
    assert bc2s == pytest.approx((1 - 0.999 ** 7) ** 0.5, rel=1e-6)
    # the betas cross the ABI as fp32 and are read back as the decimals they were written as: the factors are the fp64 values
    # rounded once, not 1 - fp32(0.999) = 0.00099998713
    import numpy as np
    _, bc1, bc2s = ops.adamw_hyper(1e-3, 0.9, 0.999, 1)
    assert np.float32(bc1) == np.float32(1 - 0.9) and np.float32(bc2s) == np.float32((1 - 0.999) ** 0.5)
    out = (C.c_float * 3)()
    assert lib.lib().srk_adamw_hyper(1e-3, 0.9, 0.999, 0, C.byref(out)) == -1
    assert lib.lib().srk_adamw_hyper(1e-3, 0.9, 0.999, 1, None) == -2


def test_tensor_table_refuses_what_the_kernels_cannot_read(lib):
    from tpu_superresolution_amd import ops
    tab = ops.TensorTable(1)
    with pytest.raises(TypeError, match="float32"):
        tab.set("grads", [torch.zeros(3, dtype=torch.float64)], first=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tab.set("grads", [torch.zeros(3)], first=True)
    with pytest.raises(ValueError, match="table of 1"):
        tab.set("grads", [], first=True)


def test_fused_adamw_accepts_any_module_on_the_host(lib):
    """Construction, zero_grad and the state_dict round trip need neither an engine nor a GPU."""
    from tpu_superresolution_amd.optim import FusedAdamW
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    net[0].bias.requires_grad = False
    opt = FusedAdamW(net, lr=1e-3, max_grad_norm=1.0)
    assert len(opt.param_groups[0]["params"]) == 3
    net(torch.rand(5, 3)).sum().backward()
    opt.zero_grad(set_to_none=False)
    assert all(p.grad is None or float(p.grad.abs().sum()) == 0.0 for p in net.parameters())
    opt.zero_grad()
    assert all(p.grad is None for p in net.parameters())
    assert opt.step() is None                          # no parameter has a gradient: nothing to do, nothing launched
    sd = opt.state_dict()
    assert sd["fused"]["step"] == 0
    opt2 = FusedAdamW(net, lr=1e-3)
    opt2.load_state_dict(sd)


def _args(tmp_path, *more):
    return ["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", *more]


@pytest.mark.parametrize("more", [("--arch", "hat"), ("--arch", "dat", "--graph"), ("--arch", "swinir")])
def test_finetune_script_parses_arch_and_graph(tmp_path, monkeypatch, more):
    """Past the parser the script stops at its first device question (made to answer 'no GPU' here)."""
    from tpu_superresolution_amd import finetune_swinir as F
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        F.main(_args(tmp_path, *more))
    assert "needs a GPU" in str(e.value)


def test_finetune_script_refuses_graph_for_swinir_and_unknown_arch(tmp_path, monkeypatch, capsys):
    from tpu_superresolution_amd import finetune_swinir as F

    def no_device_work(*a, **k):
        raise AssertionError("refusal must come before any distributed / device set-up")
    monkeypatch.setattr(F, "init_from_env", no_device_work)
    monkeypatch.setattr(torch.cuda, "is_available", no_device_work)
    with pytest.raises(SystemExit) as e:
        F.main(_args(tmp_path, "--graph"))
    assert e.value.code == 2 and "--graph" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        F.main(_args(tmp_path, "--arch", "edsr"))
    assert e.value.code == 2
