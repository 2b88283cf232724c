"""Fused global-norm clip + AdamW (libsrk kernels): over the engine's flat fp32 buffers for SwinIR, over the list of separate
parameter tensors (multi-tensor kernels, csrc/optim_multi.hip) for every other model (HAT, DAT).

Semantics = ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` followed by ``torch.optim.AdamW.step()``
as used by the reference training loop (finetune_swinir.py:168-171, :303), without the host sync the
reference's clip performs: the clip coefficient is computed on the device from the gradient sum of
squares.  Subclasses ``torch.optim.Optimizer`` only so that LR schedulers (CosineAnnealingLR,
finetune_swinir.py:307-309) can drive ``param_groups[0]['lr']``.

List path under hipGraph capture (training.GraphedTrainStep): kernel arguments are frozen at capture, so the captured step kernel reads
the learning rate and the two bias-correction factors from a 3-float device tensor.  ``begin_replay()`` advances the step count and
rewrites that tensor from ``param_groups[0]['lr']`` before every replay (LR schedulers keep working, the bias correction follows the
step count); ``end_replay()`` bumps the version counters that the models' bf16 pack caches are keyed on.

EMA of the weights (``ema_decay``): the step kernels also advance ``ema = decay * ema + (1 - decay) * p_new`` while the new weight is
in a register, so the average is gated and captured with the step.  It advances for exactly the tensors / ranges a step updates: a
frozen parameter has none, and a trainable parameter without a gradient in some step is skipped by the step and so by the average in
that step.  Buffers (DAT's BatchNorm statistics) are not averaged: ``ema_state_dict()`` returns their live values.
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import ops
from ._lib import check, lib
from .network_swinir import SwinIR


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def trains_through_engine(model) -> bool:
    """A SwinIR that trains through the C++ engine (flat parameter buffer): every SwinIR but one on which
    ``enable_small_window_training()`` has been called -- call that BEFORE constructing the optimizer."""
    return isinstance(model, SwinIR) and not getattr(model, "_small_window_training", False)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None, grad_div: float = 1.0,
                 ema_decay: Optional[float] = None):
        ema_decay = ops._ema_decay(ema_decay)          # None / 0 = off; outside [0, 1): ValueError
        params = [p for p in model.parameters() if p.requires_grad]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.model = model
        self.max_grad_norm = max_grad_norm
        self.grad_div = float(grad_div)          # world size for data-parallel gradient averaging
        self.ema_decay = ema_decay
        self._swapped = False          # inside swap_ema(): the weights hold the average and the other way round
        self._ema: Optional[torch.Tensor] = None          # flat path: the average of eng.flat (frozen ranges stay equal to the weights)
        self._step = 0
        self._m: Optional[torch.Tensor] = None
        self._v: Optional[torch.Tensor] = None
        self._sumsq: Optional[torch.Tensor] = None
        self._ranges: Optional[List[Tuple[int, int]]] = None
        self._engine_id = None
        # every model but SwinIR: separate parameter tensors, moments in self.state[p] (torch's own layout, so that
        # Optimizer.state_dict / load_state_dict carry them), one pointer table per set of parameters that have a gradient
        self._flat = trains_through_engine(model)          # an enabled small-window SwinIR is host-orchestrated: list path
        self._hyper: Optional[torch.Tensor] = None          # device {lr, 1 - beta1^step, sqrt(1 - beta2^step)} for captured steps
        self._table: Optional[ops.TensorTable] = None
        self._table_key = None

    # ---- list path (HAT, DAT, any nn.Module) -------------------------------------------------------------------------------------
    def _stepped(self) -> List[torch.Tensor]:
        """Parameters this step updates: trainable and with a gradient (torch skips the others too)."""
        return [p for p in self.param_groups[0]["params"] if p.requires_grad and p.grad is not None]

    def _prepare_list(self, with_state: bool) -> Optional[ops.TensorTable]:
        ps = self._stepped()
        if not ps:
            return None
        dev = ps[0].device
        if self._sumsq is None or self._sumsq.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: run one eager step before capturing (state is allocated outside the graph)")
            self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
            self._hyper = torch.zeros(3, dtype=torch.float32, device=dev)
        key = tuple(p.data_ptr() for p in ps)
        if self._table is None or self._table_key != key:
            self._table, self._table_key = ops.TensorTable(len(ps)), key
            self._table.set("params", ps, first=True)
        tab = self._table
        tab.set("grads", [p.grad for p in ps])          # every step: the backward hands out freshly allocated tensors
        if with_state and "exp_avg" not in tab.ptrs:
            for p in ps:
                st = self.state[p]
                if "exp_avg" not in st:
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("FusedAdamW: run one eager step before capturing (state is allocated outside the graph)")
                    st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
            tab.set("exp_avg", [self.state[p]["exp_avg"] for p in ps])
            tab.set("exp_avg_sq", [self.state[p]["exp_avg_sq"] for p in ps])
            if self.ema_decay is not None:
                for p in ps:          # starts from the weights as they are before the parameter's first update (also after loading a
                    st = self.state[p]          # state that has no average)
                    if "ema" not in st:
                        if torch.cuda.is_current_stream_capturing():
                            raise RuntimeError("FusedAdamW: run one eager step before capturing (state is allocated outside the graph)")
                        st["ema"] = p.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
                tab.set("ema", [self.state[p]["ema"] for p in ps])
        tab.keep = ps
        return tab

    def _write_hyper(self) -> None:
        grp = self.param_groups[0]
        b1, b2 = grp["betas"]
        self._hyper.copy_(torch.tensor(ops.adamw_hyper(grp["lr"], b1, b2, self._step), dtype=torch.float32))

    def begin_replay(self) -> None:
        """Before every replay of a captured step: advance the step count and hand lr / bias corrections to the captured kernels."""
        if self._flat or self._hyper is None:
            raise RuntimeError("FusedAdamW.begin_replay(): no captured list-path step")
        self._step += 1
        self._write_hyper()

    def end_replay(self) -> None:
        """After a replay: the weights (and the model's buffers) changed behind the host's back; bump the version counters that the
        bf16 pack caches of HAT / DAT are keyed on."""
        torch._C._increment_version(list(self.param_groups[0]["params"]) + list(self.model.buffers()))

    def _step_list(self, nonfinite: Optional[torch.Tensor]):
        tab = self._prepare_list(with_state=True)
        if tab is None:
            return None
        grp = self.param_groups[0]
        dev = tab.keep[0].device
        if nonfinite is not None and (nonfinite.dtype != torch.int32 or nonfinite.device != dev):
            raise ValueError("nonfinite must be an int32 tensor on the model's device")
        clip = self.max_grad_norm if self.max_grad_norm and self.max_grad_norm > 0 else 0.0
        b1, b2 = grp["betas"]
        capturing = torch.cuda.is_current_stream_capturing()
        with torch.cuda.device(dev):
            self._sumsq.zero_()
            ops.multi_grad_sumsq(tab, self._sumsq)
            if not capturing:
                self._step += 1          # a captured step advances in begin_replay()
            ops.multi_adamw_clip_step(tab, self._sumsq, clip, self.grad_div, grp["lr"], b1, b2, grp["eps"], grp["weight_decay"],
                                      max(self._step, 1), hyper=self._hyper if capturing else None, nonfinite=nonfinite,
                                      ema_decay=self.ema_decay)
        # the kernels wrote through raw pointers: tell the pack caches (hat_arch.HAT._pack, dat_arch.DAT._pack, hat_train /
        # dat_train pack_*) that the parameters changed.  Under capture this makes the NEXT forward outside the graph re-pack.
        torch._C._increment_version(tab.keep)
        return None

    # ---- flat path (SwinIR) ----------------------------------------------------------------------------------------------------------
    def _prepare(self):
        eng = self.model._engine
        if eng is None:
            raise RuntimeError("FusedAdamW.step() before the model ran on the GPU")
        if self._engine_id != id(eng):
            if self._m is not None and self._m.numel() == eng.flat.numel():
                self._m, self._v = self._m.to(eng.device), self._v.to(eng.device)
            else:
                self._m, self._v = torch.zeros_like(eng.flat), torch.zeros_like(eng.flat)
            if self.ema_decay is not None:
                if self._ema is not None and self._ema.numel() == eng.flat.numel():
                    self._ema = self._ema.to(eng.device)
                else:
                    self._ema = eng.flat.clone()          # before the first update
            self._sumsq = torch.zeros(1, dtype=torch.float32, device=eng.device)
            trainable = {n for n, p in self.model.named_parameters() if p.requires_grad}
            ranges: List[Tuple[int, int]] = []
            for info in eng.plan.params:          # merge adjacent trainable tensors (64-float aligned slots)
                if info.name not in trainable:
                    continue
                b, e = info.offset, info.offset + (info.numel + 63) // 64 * 64
                if ranges and ranges[-1][1] == b:
                    ranges[-1] = (ranges[-1][0], e)
                else:
                    ranges.append((b, e))
            self._ranges = ranges
            self._engine_id = id(eng)
        return eng

    @torch.no_grad()
    def grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the (averaged) gradients as a device tensor (no host sync)."""
        if not self._flat:
            tab = self._prepare_list(with_state=False)
            if tab is None:
                raise RuntimeError("FusedAdamW.grad_norm(): no parameter has a gradient")
            with torch.cuda.device(tab.keep[0].device):
                self._sumsq.zero_()
                ops.multi_grad_sumsq(tab, self._sumsq)
                return self._sumsq.sqrt() / self.grad_div
        eng = self._prepare()
        g = eng.ensure_grad()
        with torch.cuda.device(eng.device):
            self._sumsq.zero_()
            for b, e in self._ranges:
                check(lib().srk_grad_sumsq(g.data_ptr() + 4 * b, e - b, self._sumsq.data_ptr(), _stream(eng.device)))
            return self._sumsq.sqrt() / self.grad_div

    @torch.no_grad()
    def step(self, closure=None, nonfinite: Optional[torch.Tensor] = None):
        """clip + AdamW.  `nonfinite`: optional int32 device counter (training.l1_loss_checked); when it is non-zero -- or
        when the gradient norm is NaN/Inf -- the kernels leave weights and moments untouched (no host sync needed), so a
        bad batch cannot destroy the model before the caller's finite check raises (finetune_swinir.py:159-165)."""
        if closure is not None:
            raise RuntimeError("FusedAdamW does not support closures")
        if self._swapped:
            raise RuntimeError("FusedAdamW.step() inside swap_ema(): the weights hold the average")
        if not self._flat:
            return self._step_list(nonfinite)
        if not trains_through_engine(self.model):
            raise RuntimeError("FusedAdamW: enable_small_window_training() was called on the model after this optimizer was constructed "
                               "(it was classified as an engine model); enable first, then construct the optimizer")
        eng = self._prepare()
        g = eng.ensure_grad()
        grp = self.param_groups[0]
        clip = self.max_grad_norm if self.max_grad_norm and self.max_grad_norm > 0 else 0.0
        bad = None
        if nonfinite is not None:
            if nonfinite.dtype != torch.int32 or nonfinite.device != eng.flat.device:
                raise ValueError("nonfinite must be an int32 tensor on the model's device")
            bad = nonfinite.data_ptr()
        with torch.cuda.device(eng.device):
            st = _stream(eng.device)
            self._sumsq.zero_()          # always computed: a NaN/Inf norm gates the step even without clipping
            for b, e in self._ranges:
                check(lib().srk_grad_sumsq(g.data_ptr() + 4 * b, e - b, self._sumsq.data_ptr(), st))
            self._step += 1
            b1, b2 = grp["betas"]
            for b, e in self._ranges:
                if self.ema_decay is not None:
                    ops.adamw_clip_step(eng.flat, g, self._m, self._v, self._sumsq, clip, self.grad_div, grp["lr"], b1, b2, grp["eps"],
                                        grp["weight_decay"], self._step, nonfinite=nonfinite, ema=self._ema, ema_decay=self.ema_decay,
                                        offset=b, numel=e - b)
                    continue
                check(lib().srk_adamw_clip_step(eng.flat.data_ptr() + 4 * b, g.data_ptr() + 4 * b, self._m.data_ptr() + 4 * b,
                                                self._v.data_ptr() + 4 * b, e - b, self._sumsq.data_ptr(), float(clip),
                                                self.grad_div, float(grp["lr"]), float(b1), float(b2), float(grp["eps"]),
                                                float(grp["weight_decay"]), self._step, bad, st))
        eng.packed_valid = False
        return None

    def zero_grad(self, set_to_none: bool = True):
        if not self._flat and not set_to_none:
            return super().zero_grad(set_to_none=False)
        eng = getattr(self.model, "_engine", None)
        if set_to_none or eng is None or eng.flat_grad is None:
            for p in self.model.parameters():
                p.grad = None
        else:
            eng.flat_grad.zero_()

    def state_dict(self):
        sd = super().state_dict()          # list path: the per-parameter moments are in sd["state"], as torch.optim.AdamW keeps them
        sd["fused"] = {"step": self._step, "exp_avg": self._m, "exp_avg_sq": self._v}
        if self.ema_decay is not None:
            sd["fused"]["ema"] = self._ema          # flat path; the list path keeps it in sd["state"][i]["ema"]
        return sd

    def load_state_dict(self, state_dict):
        fused = state_dict.get("fused")
        rest = {k: v for k, v in state_dict.items() if k != "fused"}
        super().load_state_dict(rest)
        if fused is not None:
            self._step = int(fused["step"])
            self._m, self._v = fused["exp_avg"], fused["exp_avg_sq"]
            self._ema = fused.get("ema") if self.ema_decay is not None else None          # absent: starts from the current weights
            self._engine_id = None
        self._table = None          # list path: the moments were replaced, rebuild the pointer table

    # ---- EMA of the weights ----------------------------------------------------------------------------------------------------------
    def _ema_pairs(self) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """(weights, average) pairs that exist: one per stepped parameter on the list path, the two flat buffers on the flat path."""
        if self._flat:
            eng = getattr(self.model, "_engine", None)
            if eng is None or self._ema is None or self._engine_id != id(eng):
                return []
            return [(eng.flat, self._ema)]
        return [(p, self.state[p]["ema"]) for p in self.param_groups[0]["params"] if "ema" in self.state.get(p, {})]

    @torch.no_grad()
    def ema_state_dict(self):
        """The model's state_dict (same keys, same order, on the CPU) with the average in place of every parameter that has one.
        Parameters that never stepped (frozen) come as the weights they are; buffers (DAT's BatchNorm statistics, index tables) are
        not averaged and come as their live values."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW.ema_state_dict(): ema_decay is not set")
        if self._swapped:
            raise RuntimeError("FusedAdamW.ema_state_dict() inside swap_ema(): the average is in the model (model.state_dict())")
        named = dict(self.model.named_parameters())
        avg = {}
        if self._flat:
            pairs = self._ema_pairs()
            if pairs:
                avg = self.model._engine.views(pairs[0][1])
        else:
            avg = {n: self.state[p]["ema"] for n, p in named.items() if "ema" in self.state.get(p, {})}
        out = OrderedDict()
        for k, v in self.model.state_dict().items():
            src = avg[k].reshape(v.shape) if k in avg and k in named else v
            out[k] = src.detach().cpu().clone()
        return out

    def _exchange(self, pairs) -> None:
        with torch.no_grad():
            ws, es = [w for w, _ in pairs], [e for _, e in pairs]
            tmp = [w.detach().clone() for w in ws]
            for w, e, t in zip(ws, es, tmp):          # by content: a captured graph and SwinIR's parameter views hold the pointers
                w.copy_(e.view_as(w))
                e.copy_(t.view_as(e))
        if self._flat:
            self.model._engine.packed_valid = False
        else:
            torch._C._increment_version([w for w, _ in pairs])

    @contextlib.contextmanager
    def swap_ema(self):
        """``with opt.swap_ema():`` the model runs on the averaged weights (validation, export); weights and average change places by
        content and change back on exit, also after an exception.  The bf16 pack caches are invalidated on entry and on exit."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW.swap_ema(): ema_decay is not set")
        if self._swapped:
            raise RuntimeError("FusedAdamW.swap_ema() does not nest")
        pairs = self._ema_pairs()
        if self._step < 1 or not pairs:
            raise RuntimeError("FusedAdamW.swap_ema(): no step has run yet, there is no average to swap in")
        self._exchange(pairs)
        self._swapped = True
        try:
            yield self
        finally:
            self._exchange(pairs)
            self._swapped = False
