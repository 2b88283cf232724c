"""CPU-only checks of the EMA-of-weights feature: the two C-ABI symbols exist, their argument checks answer with the documented codes
before any launch, FusedAdamW(ema_decay=..) constructs and round-trips its state on the host, finetune_swinir knows --ema_decay, and
the checkpoint loaders know the 'params_ema' envelope."""
import ctypes as C
import io

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from tpu_superresolution_amd import build
    build.build(verbose=False)
    from tpu_superresolution_amd import _lib
    return _lib


NEW = ("srk_adamw_clip_ema_step", "srk_multi_adamw_clip_ema_step")
E_SHAPE, E_NULL = -1, -2


def test_ema_symbols_are_declared_bound_and_exported(lib):
    names = lib.declared_symbols()
    handle = lib.lib()
    for n in NEW:
        assert n in names, n
        assert n in lib._SIGNATURES, n
        assert hasattr(handle, n), n


def _lists(n, fill=64):
    return (C.c_void_p * n)(*([fill] * n))          # never dereferenced: every call below must fail before a launch


def test_flat_ema_step_argument_checks(lib):
    h = lib.lib()

    def call(p=64, g=64, m=64, v=64, ema=64, sumsq=64, max_norm=1.0, grad_div=1.0, step=1, decay=0.999):
        return h.srk_adamw_clip_ema_step(p, g, m, v, ema, 16, sumsq, max_norm, grad_div, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, decay, None, None)
    assert call(ema=None) == E_NULL
    assert b"ema" in h.srk_last_error()
    for role in ("p", "g", "m", "v"):
        assert call(**{role: None}) == E_NULL, role
    for bad in (1.0, -0.1, float("nan"), 1.5):
        assert call(decay=bad) == E_SHAPE, bad
        assert b"ema_decay" in h.srk_last_error()
    assert call(step=0) == E_SHAPE                      # inherited from srk_adamw_clip_step
    assert call(grad_div=0.0) == E_SHAPE
    assert call(sumsq=None) == E_NULL                   # clipping needs the sum of squares


def test_multi_ema_step_argument_checks(lib):
    h = lib.lib()
    numel = (C.c_int64 * 3)(4, 5, 6)
    p, g, m, v, e = (_lists(3) for _ in range(5))

    def call(p=p, g=g, m=m, v=v, ema=e, numel=numel, n=3, sumsq=64, max_norm=1.0, grad_div=1.0, step=1, decay=0.999):
        return h.srk_multi_adamw_clip_ema_step(p, g, m, v, ema, numel, n, sumsq, max_norm, grad_div, 1e-3, 0.9, 0.999, 1e-8, 0.0, step,
                                               decay, None, None, None)
    assert call(ema=None) == E_NULL                     # null list
    assert b"'ema'" in h.srk_last_error()
    hole = _lists(3)
    hole[2] = None
    assert call(ema=hole) == E_NULL                     # a hole in the list, at a non-zero count
    assert b"ema[2]" in h.srk_last_error()
    zero = (C.c_int64 * 3)(4, 5, 0)
    assert call(ema=hole, numel=zero, step=0) == E_SHAPE          # ... which a count of 0 excuses: the next check answers
    for bad in (1.0, -0.1, float("nan")):
        assert call(decay=bad) == E_SHAPE, bad
        assert b"ema_decay" in h.srk_last_error()
    assert call(step=0) == E_SHAPE                      # inherited from srk_multi_adamw_clip_step
    for role in ("p", "g", "m", "v", "numel"):
        assert call(**{role: None}) == E_NULL, role
    assert call(n=0) == E_SHAPE
    assert call(sumsq=None) == E_NULL


def test_fused_adamw_with_ema_on_the_host(lib):
    from tpu_superresolution_amd.optim import FusedAdamW
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    opt = FusedAdamW(net, lr=1e-3, ema_decay=0.999)
    assert opt.ema_decay == 0.999
    assert FusedAdamW(net).ema_decay is None and FusedAdamW(net, ema_decay=0).ema_decay is None and FusedAdamW(net, ema_decay=None).ema_decay is None
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(net, ema_decay=bad)
    with pytest.raises(RuntimeError, match="no step"):
        with opt.swap_ema():
            pass
    with pytest.raises(RuntimeError, match="ema_decay"):
        with FusedAdamW(net).swap_ema():
            pass
    with pytest.raises(RuntimeError, match="ema_decay"):
        FusedAdamW(net).ema_state_dict()
    # before any step nothing has an average: the weights themselves, keys and order of the model's state_dict, on the CPU
    esd = opt.ema_state_dict()
    assert list(esd) == list(net.state_dict())
    assert all(torch.equal(esd[k], v) and esd[k].data_ptr() != v.data_ptr() for k, v in net.state_dict().items())
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=False)
    assert "ema" in sd["fused"] and sd["fused"]["step"] == 0
    opt2 = FusedAdamW(net, lr=1e-3, ema_decay=0.999)
    opt2.load_state_dict(sd)
    assert "ema" not in FusedAdamW(net).state_dict()["fused"]          # EMA off: the state is what it was, key for key
    opt2.load_state_dict(FusedAdamW(net).state_dict())                 # a state without an average loads into an optimizer with one


def _args(tmp_path, *more):
    return ["--data_root", str(tmp_path), "--scale", "X4", "--epochs", "1", "--batch_size", "2", "--workers", "0", *more]


@pytest.mark.parametrize("arch", ["swinir", "hat", "dat"])
def test_finetune_script_parses_ema_decay(tmp_path, monkeypatch, arch):
    """Past the parser the script stops at its first device question (made to answer 'no GPU' here)."""
    from tpu_superresolution_amd import finetune_swinir as F
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        F.main(_args(tmp_path, "--arch", arch, "--ema_decay", "0.999"))
    assert "needs a GPU" in str(e.value)


@pytest.mark.parametrize("bad", ["1", "-0.1", "nan"])
def test_finetune_script_refuses_ema_decay_outside_the_interval(tmp_path, monkeypatch, capsys, bad):
    from tpu_superresolution_amd import finetune_swinir as F

    def no_device_work(*a, **k):
        raise AssertionError("refusal must come before any distributed / device set-up")
    monkeypatch.setattr(F, "init_from_env", no_device_work)
    monkeypatch.setattr(torch.cuda, "is_available", no_device_work)
    with pytest.raises(SystemExit) as e:
        F.main(_args(tmp_path, "--ema_decay", bad))
    assert e.value.code == 2 and "--ema_decay" in capsys.readouterr().err


def test_load_state_knows_the_params_ema_envelope(tmp_path):
    from tpu_superresolution_amd.evaluate import _load_state
    a = {"w": torch.arange(3.0), "b": torch.zeros(2)}
    b = {"w": torch.arange(3.0) + 1, "b": torch.ones(2)}

    def same(x, y):
        return list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x)
    only = str(tmp_path / "only_ema.pth")
    torch.save({"params_ema": b}, only)
    sd, msg = _load_state(only)
    assert same(sd, b) and "params_ema" in msg
    assert same(_load_state(only, "auto")[0], b) and same(_load_state(only, "params_ema")[0], b)
    both = str(tmp_path / "both.pt")
    torch.save({"model": a, "params_ema": b, "epoch": 3}, both)
    assert same(_load_state(both)[0], a)
    assert same(_load_state(both, "auto")[0], a)
    assert same(_load_state(both, "model")[0], a)
    assert same(_load_state(both, "params_ema")[0], b)
    with pytest.raises(KeyError) as e:
        _load_state(both, "params")
    assert "model" in str(e.value) and "params_ema" in str(e.value) and "epoch" in str(e.value)
    three = str(tmp_path / "three.pt")
    torch.save({"params_ema": b, "params": a}, three)
    assert same(_load_state(three)[0], a)               # order: model, params, then params_ema
    raw = str(tmp_path / "raw.pt")
    torch.save(a, raw)
    assert same(_load_state(raw)[0], a)
    with pytest.raises(KeyError, match="params_ema"):
        _load_state(raw, "params_ema")


def test_evaluate_parser_has_param_key(tmp_path, capsys):
    from tpu_superresolution_amd import evaluate as E
    with pytest.raises(SystemExit) as e:
        E.main(["--scale", "X4", "--ckpt", "x.pt", "--param_key", "weights"])
    assert e.value.code == 2 and "--param_key" in capsys.readouterr().err
