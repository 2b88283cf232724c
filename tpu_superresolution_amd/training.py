"""Training-step pieces of finetune_swinir.py:148-179 on the HIP path: fused L1 loss (+ finite check),
one-call train step; make_loss: MSE / Charbonnier and an optional SSIM term through the same interface."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops


class _L1Loss(torch.autograd.Function):
    """F.l1_loss(pred, target) (finetune_swinir.py:66-67): forward and d(pred) come out of one kernel pass,
    which also counts non-finite predictions (assert_finite, :133-143) without a host sync."""

    @staticmethod
    def forward(ctx, pred, target):
        loss, d_pred, bad = ops.l1_loss_fwd_bwd(pred.contiguous(), target.contiguous().float(), want_grad=True)
        ctx.save_for_backward(d_pred)
        ctx.mark_non_differentiable(bad)
        return loss.reshape(()), bad

    @staticmethod
    def backward(ctx, g_loss, _g_bad):
        (d_pred,) = ctx.saved_tensors
        return d_pred * g_loss, None


def l1_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return _L1Loss.apply(pred, target)[0]


def l1_loss_checked(pred: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (loss, nonfinite_count) both device tensors."""
    return _L1Loss.apply(pred, target)


LOSS_KINDS = ("l1", "mse", "charbonnier")


FFT_NORMS = ("backward", "ortho")
FFT_MAX_SIDE = 512          # the frequency loss takes H, W <= 512 (csrc/fft_loss.hip)


def loss_name(kind: str = "l1", ssim_weight: float = 0.0, fft_weight: float = 0.0) -> str:
    """'l1', 'charbonnier+0.2*(1-ssim)', 'l1+0.05*fft', ...: how the scripts name the objective"""
    return kind + (f"+{ssim_weight:g}*(1-ssim)" if ssim_weight else "") + (f"+{fft_weight:g}*fft" if fft_weight else "")


def make_loss(kind: str = "l1", charbonnier_eps: float = 1e-3, ssim_weight: float = 0.0, data_range: float = 1.0,
              fft_weight: float = 0.0, fft_norm: str = "backward"):
    """-> callable (pred, target) -> (loss, nonfinite_count), both device tensors, for train_step / GraphedTrainStep(loss_fn=...).

    kind 'l1' | 'mse' | 'charbonnier' (mean sqrt(d^2 + charbonnier_eps^2)); ssim_weight > 0 adds ssim_weight * (1 - SSIM(pred, target))
    with the SSIM of metrics.ssim at `data_range` (4-D batches, H, W >= 11).  One autograd Function: its forward runs the pixel kernel
    and then the SSIM kernel, which accumulates into the same loss scalar and the same d(pred) (csrc/loss.hip: fixed-order sums, no host
    read, capturable); the non-finite counter is the one optim.FusedAdamW.step(nonfinite=...) gates on.  The target gets no gradient.
    fft_weight > 0 adds fft_weight * mean(|Re D| + |Im D|), D = rfft2(pred - target) with norm `fft_norm` ('backward' | 'ortho'): the
    frequency loss of csrc/fft_loss.hip (4-D batches, H, W <= 512), run after the other two kernels into the same scalar and d(pred).
    kind 'l1' without an SSIM or frequency term returns l1_loss_checked itself."""
    if kind not in LOSS_KINDS:
        raise ValueError(f"loss kind must be one of {LOSS_KINDS} (got {kind!r})")
    eps, w, dr, fw = float(charbonnier_eps), float(ssim_weight), float(data_range), float(fft_weight)
    if not w >= 0.0 or w == float("inf"):          # also refuses NaN
        raise ValueError(f"ssim_weight must be a finite number >= 0 (got {ssim_weight!r})")
    if not fw >= 0.0 or fw == float("inf"):
        raise ValueError(f"fft_weight must be a finite number >= 0 (got {fft_weight!r})")
    if fft_norm not in FFT_NORMS:
        raise ValueError(f"fft_norm must be one of {FFT_NORMS} (got {fft_norm!r})")
    if kind == "charbonnier" and not eps > 0.0:
        raise ValueError(f"charbonnier_eps must be > 0 (got {charbonnier_eps!r})")
    if not dr > 0.0:
        raise ValueError(f"data_range must be > 0 (got {data_range!r})")
    if kind == "l1" and w == 0.0 and fw == 0.0:
        return l1_loss_checked

    class _Loss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, pred, target):
            p, t = pred.contiguous().float(), target.contiguous().float()
            loss, d_pred, bad = ops.pixel_loss_fwd_bwd(p, t, kind, eps, want_grad=True)
            if w > 0.0:
                ops.ssim_loss_fwd_bwd(p, t, dr, alpha=w, d_x=d_pred, accumulate=True, loss=loss)
            if fw > 0.0:
                ops.fft_loss_fwd_bwd(p, t, fft_norm, alpha=fw, d_x=d_pred, accumulate=True, loss=loss)
            ctx.save_for_backward(d_pred)
            ctx.mark_non_differentiable(bad)
            return loss.reshape(()), bad

        @staticmethod
        def backward(ctx, g_loss, _g_bad):
            (d_pred,) = ctx.saved_tensors
            return d_pred * g_loss, None

    def loss_fn(pred: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if target.requires_grad:
            raise ValueError("make_loss: the target gets no gradient (detach it)")
        if w > 0.0 and (pred.ndim != 4 or pred.shape[2] < 11 or pred.shape[3] < 11):
            raise ValueError(f"make_loss: the SSIM term needs [B, C, H, W] batches with H, W >= 11 (got {tuple(pred.shape)})")
        if fw > 0.0 and (pred.ndim != 4 or pred.shape[2] > FFT_MAX_SIDE or pred.shape[3] > FFT_MAX_SIDE):
            raise ValueError(f"make_loss: the frequency term needs [B, C, H, W] batches with H, W <= {FFT_MAX_SIDE} (got {tuple(pred.shape)})")
        return _Loss.apply(pred, target)

    loss_fn.__name__ = loss_fn.__qualname__ = f"loss[{loss_name(kind, w, fw)}]"
    return loss_fn


def train_step(model, optimizer, lr_img: torch.Tensor, hr_img: torch.Tensor, sync=None, loss_fn=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One step of the reference loop (finetune_swinir.py:154-176): zero_grad, forward, L1 (or `loss_fn`, see make_loss), backward,
    [gradient all-reduce], clip + AdamW.  Returns (loss, nonfinite_count) as device tensors (no host sync)."""
    optimizer.zero_grad(set_to_none=True)
    out = model(lr_img)
    loss, bad = (loss_fn or l1_loss_checked)(out, hr_img)
    loss.backward()
    if sync is not None:
        sync.finish()
    if hasattr(optimizer, "max_grad_norm"):      # FusedAdamW: the device-side counter gates the update (no host sync)
        optimizer.step(nonfinite=bad)
    else:
        optimizer.step()
    return loss.detach(), bad


def freeze_batchnorm(model) -> int:
    """Put every nn.BatchNorm* of the model into eval mode -- it then normalises with its running statistics and writes no buffer, also
    inside a training step (DAT reads the flag per module at every forward) -- and return how many there are.  ``model.train()``
    switches them all back on: call this again after it."""
    n = 0
    for mod in model.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.eval()
            n += 1
    return n


def batchnorm_state(model) -> Tuple[bool, Tuple[bool, ...]]:
    """(model.training, the ``training`` flag of every nn.BatchNorm* in module order): what decides a host-orchestrated model's launch
    sequence besides the shapes"""
    return bool(model.training), tuple(bool(mod.training) for mod in model.modules()
                                       if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm))


def assert_finite_step(loss: torch.Tensor, bad: torch.Tensor) -> None:
    """Host-side check with the reference's error behaviour (RuntimeError on non-finite output / loss)."""
    nb = int(bad)
    if nb:
        raise RuntimeError(f"out has non-finite values: count={nb}")
    if not bool(torch.isfinite(loss)):
        raise RuntimeError("loss has non-finite values")


class GraphedTrainStep:
    """The whole train step of a host-orchestrated model (HAT / DAT: hundreds of C-ABI launches plus the small torch ops between
    them, launch-bound on the host) captured ONCE into a hipGraph and replayed: forward (activations kept, DropPath factors drawn by
    the graph-safe generator, BatchNorm running statistics updated in place), L1, the hand-written backward, gradient clipping and
    the optimizer step.

        step = GraphedTrainStep(model, torch.optim.AdamW(model.parameters(), lr=2e-5, capturable=True), max_grad_norm=1.0)
        loss, bad = step(lr_batch, hr_batch)        # copies the batch into the graph's static inputs and replays

    Requirements: static batch shape, an optimizer constructed with ``capturable=True``, no gradient all-reduce hook on the model
    (world size 1: collectives stay outside graphs here), nothing in the step that reads a device value on the host.  The first call
    runs ``warmup`` eager steps (kernel attributes, caches and workspaces get set up outside the capture), then captures.  DropPath
    factors are drawn OUTSIDE the graph, before every replay, into a static buffer the captured forward reads (``model.draw_drop_path``
    / ``model._drop_override``): a fresh draw per step does not depend on how the graph-captured generator advances.  The captured
    launch sequence depends on ``model.training`` and on every BatchNorm's ``training`` flag (batch or running statistics,
    ``freeze_batchnorm``): they are recorded at capture, and a replay under another state raises ``ValueError``.

    With an ``optim.FusedAdamW`` the step is the project's own: no ``clip_grad_norm_`` (the optimizer's ``max_grad_norm`` clips on the
    device; the ``max_grad_norm`` argument here is not used) and ``opt.step(nonfinite=bad)``, so a non-finite prediction inside a replay
    leaves weights and moments untouched.  The captured step kernel reads the learning rate and the bias corrections from device memory:
    ``opt.begin_replay()`` advances the step count and rewrites them from ``param_groups[0]['lr']`` before every replay, so an LR
    scheduler stepped between calls takes effect.

        step = GraphedTrainStep(model, FusedAdamW(model, lr=2e-5, max_grad_norm=1.0))"""

    def __init__(self, model, optimizer, max_grad_norm: float = 1.0, warmup: int = 2, loss_fn=None):
        if getattr(model, "grad_sync", None) is not None:
            raise ValueError("GraphedTrainStep: detach the gradient synchronizer (graph capture is for single-process steps)")
        self.model, self.opt, self.max_grad_norm, self.warmup = model, optimizer, float(max_grad_norm), int(warmup)
        self.loss_fn = loss_fn or l1_loss_checked              # (pred, target) -> (loss, nonfinite): make_loss; captured with the step
        self.fused = hasattr(optimizer, "begin_replay")          # optim.FusedAdamW
        if self.fused and getattr(optimizer, "_flat", False):
            raise ValueError("GraphedTrainStep is for host-orchestrated models (HAT / DAT); SwinIR's step is one C call per pass already")
        self.graph = None
        self.x = self.t = self.loss = self.bad = self.drop = None
        self.bn_state = None

    def _eager(self, x, t):
        self.opt.zero_grad(set_to_none=True)
        loss, bad = self.loss_fn(self.model(x), t)
        loss.backward()
        if self.fused:
            self.opt.step(nonfinite=bad)          # clip + AdamW, gated on the device by the non-finite counter
        else:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)
            self.opt.step()
        return loss.detach(), bad

    def __call__(self, lr_img: torch.Tensor, hr_img: torch.Tensor):
        draw = getattr(self.model, "draw_drop_path", None)
        if self.graph is None:
            self.x, self.t = lr_img.clone(), hr_img.clone()
            if draw is not None and self.model.training:
                d = draw(lr_img.shape[0], lr_img.device)
                if d is not None:
                    self.drop = d.clone()
                    self.model._drop_override = self.drop        # the captured forward reads this buffer
            side = torch.cuda.Stream(device=lr_img.device)
            side.wait_stream(torch.cuda.current_stream(lr_img.device))
            with torch.cuda.stream(side):              # warm-up on a side stream, as torch.cuda.graphs asks
                for _ in range(max(self.warmup, 1)):
                    self._eager(self.x, self.t)
            torch.cuda.current_stream(lr_img.device).wait_stream(side)
            self.bn_state = batchnorm_state(self.model)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.loss, self.bad = self._eager(self.x, self.t)
        elif lr_img.shape != self.x.shape or hr_img.shape != self.t.shape:
            raise ValueError(f"GraphedTrainStep was captured for {tuple(self.x.shape)} -> {tuple(self.t.shape)}")
        now = batchnorm_state(self.model)
        if now != self.bn_state:
            (tr0, bn0), (tr1, bn1) = self.bn_state, now
            diff = [i for i, (a, b) in enumerate(zip(bn0, bn1)) if a != b]
            what = [f"model.training {tr0} -> {tr1}"] if tr0 != tr1 else []
            if diff or len(bn0) != len(bn1):
                what.append(f"{len(diff)} of {len(bn0)} BatchNorm training flags differ (first: BatchNorm #{diff[0] if diff else min(len(bn0), len(bn1))}, "
                            f"{sum(bn0)} in training mode at capture, {sum(bn1)} now)")
            raise ValueError("GraphedTrainStep: the captured launch sequence depends on the train / eval state it was captured in; "
                             + "; ".join(what) + " -- restore the state (freeze_batchnorm after model.train()) or build a new GraphedTrainStep")
        self.x.copy_(lr_img)
        self.t.copy_(hr_img)
        if self.drop is not None:
            self.drop.copy_(draw(lr_img.shape[0], lr_img.device))
        if self.fused:
            self.opt.begin_replay()
        self.graph.replay()
        if self.fused:
            self.opt.end_replay()
        return self.loss, self.bad

    def close(self) -> None:
        """Detach from the model (its forward draws its own DropPath factors again)."""
        if getattr(self.model, "_drop_override", None) is self.drop:
            self.model._drop_override = None
