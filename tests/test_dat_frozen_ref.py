"""CPU: (1) the eval-semantics autograd oracle used by tests/test_gpu_dat_frozen.py (tests/dat_frozen_ref.py over
oracle.dat_oracle.dat_forward) against G18, the reference's own DAT in eval mode with grad enabled; (2) the host-only side of
--freeze_bn: training.freeze_batchnorm, and that the flags survive the model.train() of every epoch."""
import numpy as np
import torch

from conftest import load_golden
from dat_frozen_ref import eval_loss_and_grads, grad_errors
from oracle import dat_oracle as DO
from test_oracle_golden import DAT_TINY, _sha1


def g18_weights():
    g = load_golden("g18_dat_frozen_bn")
    cfg = DO.DATConfig(**DAT_TINY)
    sd = DO.random_state_dict(cfg, seed=int(g["weight_seed"]), scale=float(g["weight_scale"]))
    digest = _sha1(np.concatenate([v.numpy().astype(np.float32).reshape(-1) for v in sd.values()]))
    assert digest == str(g["weight_sha1"]), "DAT weight generator drifted from the one the fixture was made with"
    return g, cfg, sd


def test_g18_running_buffers_are_not_trivial():
    """frozen statistics that equal a fresh BatchNorm's (mean 0, var 1) would not tell a folded buffer from a forgotten one"""
    _, _, sd = g18_weights()
    means = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("running_mean")])
    vars_ = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("running_var")])
    assert float(means.abs().max()) > 0.1 and float((vars_ - 1.0).abs().max()) > 0.2 and float(vars_.min()) > 0.5


def test_eval_autograd_oracle_vs_reference_golden():
    """G18 (a) 24 x 40 batch 2 and (b) 32 x 32 batch 1.  fp32 against fp32: 1e-4, the bound of the other fp32 oracle pins (measured:
    output within 5e-6 absolute, loss equal to 1e-7, gradients 7e-7 per tensor).  Gradients are measured as the GPU test measures them,
    against max(|ref|, 2e-3 * the largest gradient norm): 70 tensors have an exactly zero reference gradient, a few more are rounding
    noise in both."""
    g, cfg, sd = g18_weights()
    for tag, B in (("a", 2), ("b", 1)):
        x, t = torch.from_numpy(g[f"{tag}.x"]), torch.from_numpy(g[f"{tag}.t"])
        assert x.shape[0] == B
        loss, y, grads = eval_loss_and_grads(sd, cfg, x, t)
        yr = torch.from_numpy(g[f"{tag}.y"])
        want = {n: torch.from_numpy(g[f"{tag}.grad.{n}"]) for n in grads}
        assert len(want) == 264
        errs = grad_errors(grads, want, floor=2e-3)
        worst = max(errs, key=errs.get)
        print(f"case {tag}: max|y - ref| {float((y - yr).abs().max()):.3e}, loss {loss:.8f} vs {float(g[f'{tag}.loss']):.8f}, "
              f"worst gradient {errs[worst]:.3e} at {worst}")
        assert float((y - yr).abs().max()) <= 1e-4 * float(yr.abs().max())
        assert abs(loss - float(g[f"{tag}.loss"])) <= 1e-4 * float(g[f"{tag}.loss"])
        assert errs[worst] <= 1e-4, (worst, errs[worst])
        for n in (k for k in sd if k.endswith(("running_mean", "running_var", "num_batches_tracked"))):
            assert np.array_equal(g[f"{tag}.buf.{n}"], sd[n].numpy()), n          # the reference moved no buffer


def test_g18_mixed_case_moves_only_the_unfrozen_buffers():
    g, _, sd = g18_weights()
    for n in (k for k in sd if k.endswith(("running_mean", "running_var", "num_batches_tracked"))):
        same = np.array_equal(g[f"c.buf.{n}"], sd[n].numpy())
        assert same == (".dwconv.1." in n), n


def _tiny_dat():
    import tpu_superresolution_amd as T
    return T.DAT(**DO.DATConfig(**DAT_TINY).kwargs(), drop_path_rate=0.1)


def test_freeze_batchnorm_counts_and_flags():
    from tpu_superresolution_amd.training import batchnorm_state, freeze_batchnorm
    m = _tiny_dat().train()
    bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    assert len(bns) == 3 * sum(DAT_TINY["depth"])          # dwconv[1], channel_interaction[2], spatial_interaction[1] per block
    assert all(b.training for b in bns)
    assert freeze_batchnorm(m) == len(bns)
    assert m.training and not any(b.training for b in bns)
    assert all(mod.training for mod in m.modules() if not isinstance(mod, torch.nn.modules.batchnorm._BatchNorm))
    assert batchnorm_state(m) == (True, (False,) * len(bns))
    m.train()                                                   # what every epoch does: all of them are live again
    assert batchnorm_state(m) == (True, (True,) * len(bns))
    import tpu_superresolution_amd as T
    swin = T.SwinIR(upscale=2, img_size=16, window_size=8, depths=[2], embed_dim=24, num_heads=[2], mlp_ratio=2)
    assert freeze_batchnorm(swin) == 0


def test_freeze_survives_the_epoch_loops_model_train():
    from tpu_superresolution_amd import finetune_swinir as F
    from tpu_superresolution_amd.training import batchnorm_state
    m = _tiny_dat().eval()
    F.train_one_epoch(m, [], None, "cpu", freeze_bn=True)          # no batch: only the mode switches of the epoch loop
    training, flags = batchnorm_state(m)
    assert training and len(flags) == 15 and not any(flags)
    F.train_one_epoch(m, [], None, "cpu")
    assert batchnorm_state(m) == (True, (True,) * 15)
