"""Fused multi-tensor optimizers: SGD (one HIP launch per step for all parameters) and AdamW with
global-norm gradient clipping (one norm launch over the model + one update launch per group).

Drop-in for ``torch.optim.SGD(params, lr, momentum, weight_decay)`` as the
reference uses it (`master/part1/part1.py:98-99`): same update rule and same
``state_dict`` format (``momentum_buffer`` per parameter), so checkpoints are
interchangeable. On CPU tensors it defers to torch's implementation.

``FusedAdamW`` is the same for ``torch.optim.AdamW``: torch's update rule and torch's state
(``step``, ``exp_avg``, ``exp_avg_sq`` per parameter), with ``clip_grad_norm_`` folded into the pass.
"""
from __future__ import annotations

import torch

from . import native


_NO_SHADOW = {}


def _shadow_of(p: torch.Tensor) -> torch.Tensor:
    """the live bf16 shadow of ``p`` (registered by ``ops.lm.ShadowLinear``), or an empty tensor"""
    sh = getattr(p, "_cs_bf16_shadow", None)
    if sh is not None and getattr(p, "_cs_bf16_shadow_version", -1) == p._version and sh.numel() == p.numel():
        return sh
    dev = p.device
    if dev not in _NO_SHADOW:
        _NO_SHADOW[dev] = torch.empty(0, device=dev, dtype=torch.bfloat16)
    return _NO_SHADOW[dev]


class FusedSGD(torch.optim.SGD):
    def __init__(self, params, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 grad_scale: float = 1.0):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov)
        if nesterov:
            raise ValueError("FusedSGD: nesterov not supported (the reference does not use it)")
        self.grad_scale = grad_scale
        self._tables = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            if not ps[0].is_cuda:
                return super().step()
            # `first` (buf = d, the buffer is not read) is decided per parameter, as torch.optim.SGD does:
            # a parameter whose first gradient arrives after the others' must not reset their momentum.
            # One launch per group whenever all its parameters agree (every step but such a one); in
            # the step where they differ the new parameters get a launch and a cached table of their own.
            fresh = [p for p in ps if self.state[p].get("momentum_buffer") is None]
            for p in fresh:
                self.state[p]["momentum_buffer"] = torch.zeros_like(p)
            if group["momentum"] == 0 or len(fresh) in (0, len(ps)):
                self._launch(group, 0, ps, bool(fresh))
            else:
                new = {id(p) for p in fresh}
                self._launch(group, 0, [p for p in ps if id(p) not in new], False)
                self._launch(group, 1, fresh, True)
        return loss

    def _launch(self, group, slot, ps, first):
        """one fused update of ``ps`` (parameters of ``group`` that have a gradient and a buffer); the
        device table is cached per (group, slot) and rebuilt when a pointer changes"""
        mom = group["momentum"]
        bufs = [self.state[p]["momentum_buffer"] for p in ps]
        gs = [p.grad for p in ps]
        # a parameter with a live bf16 shadow (ops.lm.ShadowLinear) gets it rewritten by the same pass
        shs = [_shadow_of(p) for p in ps]
        key = tuple((p.data_ptr(), g.data_ptr(), b.data_ptr(), s.data_ptr() if s.numel() else 0)
                    for p, g, b, s in zip(ps, gs, bufs, shs))
        tab = self._tables.get((id(group), slot))
        if tab is None or tab[0] != key:
            t = native.C().sgd_multi_table(ps, gs, bufs, shs)
            nchunks = int(t[-1].item())
            tab = (key, t, nchunks)
            self._tables[(id(group), slot)] = tab
        native.C().sgd_multi(tab[1], len(ps), tab[2], group["lr"], mom, group["weight_decay"],
                             group["dampening"], self.grad_scale, first and mom != 0)


class FusedAdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` (decoupled weight decay) with ``clip_grad_norm_(max_grad_norm)`` and the
    gradient scale folded into two passes over the model: one deterministic sum-of-squares launch over
    every parameter of every group (the norm is global) and one update launch per parameter group,
    which also rewrites the bf16 shadows of ``ops.lm.ShadowLinear`` weights. ``lr``, ``betas``,
    ``eps`` and ``weight_decay`` are read from the group at every step (schedulers work). The state is
    torch's, so ``state_dict()`` loads into ``torch.optim.AdamW`` and back."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 grad_scale: float = 1.0, *, amsgrad=False, maximize=False, capturable=False):
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable)):
            if on:
                raise ValueError(f"FusedAdamW: {name} not supported")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"FusedAdamW: max_grad_norm must be positive or None, got {max_grad_norm}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # (not `grad_scale`: torch's Adam.step reads an attribute of that name as the AMP GradScaler's tensor)
        self.grad_mult = grad_scale
        self._table = None      # (pointer key, device table, chunk prefix): rebuilt when a pointer changes
        self._partials = None   # the norm pass's per-block sums (float64) and the norm it leaves (float32)
        self._norm = None
        self._norm_valid = False

    def last_grad_norm(self):
        """The gradient norm of the last step as a device scalar (before clipping, after ``grad_scale``);
        ``None`` when clipping is off. Reading it is the caller's sync, the step itself has none."""
        return self._norm if self._norm_valid else None

    def _step_cpu(self):
        ps = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if self.grad_mult != 1.0:
            torch._foreach_mul_([p.grad for p in ps], self.grad_mult)
        if self.max_grad_norm is not None:
            self._norm = torch.nn.utils.clip_grad_norm_(ps, self.max_grad_norm)
            self._norm_valid = True
        return super().step()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        first = next((p for group in self.param_groups for p in group["params"] if p.grad is not None), None)
        if first is None:
            return loss
        if not first.is_cuda:
            self._step_cpu()
            return loss
        # runs of the table: one per group (and per step count inside a group, which differs only when
        # a parameter sat out some steps); each is one update launch with its own bias corrections
        runs = []
        ps, ms, vs = [], [], []
        for gi, group in enumerate(self.param_groups):
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(name):
                    raise ValueError(f"FusedAdamW: {name} not supported")
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                by_step.setdefault(int(st["step"]), []).append(p)
            for t in sorted(by_step):
                runs.append((gi, t, len(ps), len(by_step[t])))
                for p in by_step[t]:
                    ps.append(p)
                    ms.append(self.state[p]["exp_avg"])
                    vs.append(self.state[p]["exp_avg_sq"])
        gs = [p.grad for p in ps]
        shs = [_shadow_of(p) for p in ps]
        key = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), s.data_ptr() if s.numel() else 0)
                    for p, g, m, v, s in zip(ps, gs, ms, vs, shs))
        if self._table is None or self._table[0] != key:
            starts = [0]
            for p in ps:
                starts.append(starts[-1] + (p.numel() + 4095) // 4096)
            self._table = (key, native.C().adamw_multi_table(ps, gs, ms, vs, shs), starts)
        _, table, starts = self._table
        C = native.C()
        clip = self.max_grad_norm is not None
        if clip:
            if self._partials is None or self._partials.device != first.device:
                self._partials = torch.empty(2048, dtype=torch.float64, device=first.device)
                self._norm = torch.zeros((), dtype=torch.float32, device=first.device)
            C.grad_sumsq(table, len(ps), starts[-1], self.grad_mult, self._partials)
        self._norm_valid = clip
        for gi, t, t0, nt in runs:
            group = self.param_groups[gi]
            b1, b2 = group["betas"]
            C.adamw_multi(table, nt, starts[t0 + nt] - starts[t0], float(group["lr"]), float(b1), float(b2),
                          group["eps"], group["weight_decay"], 1.0 - b1 ** t, 1.0 - b2 ** t, self.grad_mult,
                          self.max_grad_norm if clip else 0.0, self._partials if clip else None,
                          self._norm if clip else None, t0, starts[t0])
        return loss
