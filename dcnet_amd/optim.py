"""The reference driver's three optimisers (train_DCNet.py:527-534) with the step as one fused HIP pass per 32 tensors:
``RMSprop`` (dcn_rmsprop_step), ``Adam`` (dcn_adam_prepare + dcn_adam_step) and ``SGD`` with momentum (dcn_sgd_step).

Same update, hyper-parameters and ``state_dict`` layout as ``torch.optim.RMSprop`` with ``momentum=0`` and ``centered=False``,
``torch.optim.Adam`` without ``amsgrad`` and ``torch.optim.SGD`` with ``dampening=0`` and without Nesterov momentum, so
checkpoints move between the two.  torch's foreach implementations make several element-wise passes over parameters, gradients
and state (RMSprop: five, in ~20 launches, 2.4 ms per step for the 74 M trained parameters of DCNet); these read and write each
value once.

All three follow one protocol, which is what ``dcnet_amd.graph.GraphedTrainStep`` captures them through: ``device_lr`` (the step
reads each group's learning rate from a device scalar), ``sync_lr()`` (uploads the groups' rates into those scalars),
``bump_steps()`` (a replay of a captured step ran the device update: advance the host's ``step`` counters) and ``step()``.
"""
from __future__ import annotations

import ctypes

import torch

from .lib import lib


def _ptrs(addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: the device learning rates, the ``step`` bookkeeping and the walk over the groups.
    A subclass names its state in ``_new_state`` and launches one group's update in ``_launch``."""

    LR_RING = 4

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        # device_lr: the step reads each group's learning rate from a device scalar (refreshed by sync_lr()) instead of a kernel
        # argument — what a step captured into a hipGraph needs to follow a schedule (dcnet_amd.graph.GraphedTrainStep)
        self.device_lr = False
        self._lr_dev = {}
        self._stepped = []           # the "step" counters touched by the last step() (bump_steps: replays of a captured step)
        self._stepped_params = []    # ... and whose they are (load_state_dict replaces the counters)

    def sync_lr(self, device=None) -> None:
        """Upload every group's current ``lr`` into its device scalar when it changed (async, from page-locked memory).

        The host may run several replays ahead of the GPU, so one staging word would be overwritten before its copy has
        run: each group stages through a ring of ``LR_RING`` pinned words, a slot is rewritten only after the event recorded
        behind its last copy has completed.  The "changed" test compares Python floats (the value last uploaded), not the
        float32 staging word against a double."""
        for gi, group in enumerate(self.param_groups):
            ent = self._lr_dev.get(gi)
            if ent is None:
                dev = device if device is not None else next(p.device for p in group["params"] if p.is_cuda)
                ent = {"pinned": torch.empty(self.LR_RING, dtype=torch.float32).pin_memory(), "dev": torch.empty(1, dtype=torch.float32, device=dev),
                       "events": [None] * self.LR_RING, "next": 0, "last": None}
                self._lr_dev[gi] = ent
            lr = float(group["lr"])
            if ent["last"] is not None and ent["last"] == lr:
                continue
            i = ent["next"]
            if ent["events"][i] is not None:
                ent["events"][i].synchronize()          # the copy that last read this slot has run
            ent["pinned"][i] = lr
            ent["dev"].copy_(ent["pinned"][i:i + 1], non_blocking=True)
            ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(ent["dev"].device))
            ent["events"][i] = ev
            ent["next"] = (i + 1) % self.LR_RING
            ent["last"] = lr

    def bump_steps(self) -> None:
        """Advance the per-parameter ``step`` counters once more (a replay of a captured step ran the device update)."""
        if self._stepped:
            torch._foreach_add_(self._stepped, 1)

    def _name(self) -> str:
        return f"dcnet_amd.optim.{type(self).__name__}"

    def _new_state(self, p) -> dict:
        raise NotImplementedError

    def _launch(self, L, gi, group, live, lr_dev, stream) -> None:
        """One group's update.  ``live``: (parameter, contiguous gradient, state) of every parameter that has a gradient."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = lib()
        self._stepped, self._stepped_params = [], []
        if self.device_lr:
            if not torch.cuda.is_current_stream_capturing():
                self.sync_lr()           # an eager step always sees the groups' current learning rates (a captured one: sync_lr() before the replay)
            elif not self._lr_dev:
                raise RuntimeError(f"{self._name()}: device_lr is set but sync_lr() was never called before the capture")
        for gi, group in enumerate(self.param_groups):
            live = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError(f"{self._name()}: contiguous fp32 CUDA parameters only (no CPU path)")
                st = self.state[p]
                if len(st) == 0:
                    st.update(self._new_state(p))
                # (a contiguous copy of the gradient may be freed right after the launch: same-stream reuse is ordered)
                live.append((p, p.grad if p.grad.is_contiguous() else p.grad.contiguous(), st))
            if not live:
                continue
            lr_dev = self._lr_dev[gi]["dev"].data_ptr() if self.device_lr else 0
            self._launch(L, gi, group, live, lr_dev, torch.cuda.current_stream().cuda_stream)
            for p, _, st in live:
                if "step" in st:
                    st["step"] += 1
                    self._stepped.append(st["step"]); self._stepped_params.append(p)
        return loss

    def load_state_dict(self, state_dict) -> None:
        """torch's, then: ``step`` counters as the host scalars torch's own default keeps (whatever device the writer had them on), and
        the bookkeeping of ``bump_steps`` pointed at the counters that replaced the old ones."""
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if "step" in st:
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
        self._stepped_params = [p for p in self._stepped_params if "step" in self.state.get(p, {})]
        self._stepped = [self.state[p]["step"] for p in self._stepped_params]


class RMSprop(_FusedOptimizer):
    def __init__(self, params, lr: float = 1e-2, alpha: float = 0.99, eps: float = 1e-8, weight_decay: float = 0.0,
                 momentum: float = 0.0, centered: bool = False):
        if momentum != 0.0 or centered:
            raise NotImplementedError("dcnet_amd.optim.RMSprop implements momentum=0, centered=False (the reference's setting)")
        if lr < 0 or eps < 0 or alpha < 0 or weight_decay < 0:
            raise ValueError("invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=0.0, centered=False))

    def _new_state(self, p):
        return {"step": torch.zeros((), dtype=torch.float32), "square_avg": torch.zeros_like(p, memory_format=torch.preserve_format)}

    def _launch(self, L, gi, group, live, lr_dev, stream):
        n = len(live)
        L.rmsprop_step(_ptrs([p.data_ptr() for p, _, _ in live]), _ptrs([g.data_ptr() for _, g, _ in live]),
                       _ptrs([st["square_avg"].data_ptr() for _, _, st in live]), (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in live]), n,
                       float(group["lr"]), lr_dev, float(group["alpha"]), float(group["eps"]), float(group["weight_decay"]), stream)


class Adam(_FusedOptimizer):
    """``torch.optim.Adam`` (``amsgrad=False``, ``maximize=False``; train_DCNet.py:528-529) as dcn_adam_prepare + dcn_adam_step.

    The bias corrections depend on the step count, and a replayed hipGraph must advance it without the host.  So beside the host
    ``step`` scalar of the state (torch's layout: what ``state_dict()`` carries) every parameter has a device step word, which the
    step's own first launch advances and turns into the step's two scalars (``lr / (1 - beta1^t)``, ``1 / sqrt(1 - beta2^t)``) — in
    an eager step and in a captured one alike.  The words are made from the host counters when a group first steps and again by
    ``load_state_dict``; a parameter without a gradient is left out of the launches and keeps its count, as in torch."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, maximize: bool = False):
        if amsgrad or maximize:
            raise NotImplementedError("dcnet_amd.optim.Adam implements amsgrad=False, maximize=False (the reference's setting)")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid hyper-parameter")
        # (the keys and values of torch.optim.Adam's groups: a state_dict loaded into torch's class brings its groups along)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False))
        self._tables = {}            # group index -> device step words and scalar slots of the group's parameters

    def _new_state(self, p):
        return {"step": torch.zeros((), dtype=torch.float32), "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
                "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}

    def _host_steps(self, group):
        return torch.tensor([int(self.state[p]["step"]) if "step" in self.state.get(p, {}) else 0 for p in group["params"]], dtype=torch.int32)

    def _table(self, gi, group, device):
        tab = self._tables.get(gi)
        if tab is None or len(tab["index"]) != len(group["params"]):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._name()}: the first step of a group cannot be a captured one (its device step words are made "
                                   "from the host counters); run an eager step first")
            n = len(group["params"])
            tab = {"steps": self._host_steps(group).to(device), "scal": torch.zeros(n, 2, dtype=torch.float32, device=device),
                   "index": {id(p): i for i, p in enumerate(group["params"])}}
            self._tables[gi] = tab
        return tab

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
            raise NotImplementedError(f"{self._name()}: amsgrad / maximize / decoupled_weight_decay are not implemented")

    def _launch(self, L, gi, group, live, lr_dev, stream):
        self._check_group(group)
        tab = self._table(gi, group, live[0][0].device)
        n = len(live)
        rows = [tab["index"][id(p)] for p, _, _ in live]
        s0, c0 = tab["steps"].data_ptr(), tab["scal"].data_ptr()
        scal = _ptrs([c0 + 8 * r for r in rows])
        b1, b2 = (float(b) for b in group["betas"])
        L.adam_prepare(_ptrs([s0 + 4 * r for r in rows]), scal, n, float(group["lr"]), lr_dev, b1, b2, stream)
        L.adam_step(_ptrs([p.data_ptr() for p, _, _ in live]), _ptrs([g.data_ptr() for _, g, _ in live]),
                    _ptrs([st["exp_avg"].data_ptr() for _, _, st in live]), _ptrs([st["exp_avg_sq"].data_ptr() for _, _, st in live]), scal,
                    (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in live]), n, b1, b2, float(group["eps"]), float(group["weight_decay"]), stream)

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        if self._tables and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._name()}: load_state_dict during a stream capture cannot refresh the device step words")
        for gi, tab in list(self._tables.items()):
            group = self.param_groups[gi]
            if len(tab["index"]) != len(group["params"]):
                del self._tables[gi]                     # (the group changed: its next eager step makes the table)
            else:
                tab["steps"].copy_(self._host_steps(group))      # in place: a captured step keeps reading these words


class SGD(_FusedOptimizer):
    """``torch.optim.SGD`` with momentum (``dampening=0``, ``nesterov=False``; train_DCNet.py:530-531) as dcn_sgd_step.  torch's SGD
    keeps no ``step`` in its state, and neither does this one: ``bump_steps()`` has nothing to advance."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, maximize: bool = False):
        if dampening != 0 or nesterov or maximize:
            raise NotImplementedError("dcnet_amd.optim.SGD implements dampening=0, nesterov=False, maximize=False (the reference's setting)")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False,
                                      foreach=None, differentiable=False, fused=None))

    def _new_state(self, p):
        return {"momentum_buffer": torch.zeros_like(p, memory_format=torch.preserve_format)}

    def _launch(self, L, gi, group, live, lr_dev, stream):
        if group.get("dampening") or group.get("nesterov") or group.get("maximize"):
            raise NotImplementedError(f"{self._name()}: dampening / nesterov / maximize are not implemented")
        for p, _, st in live:
            if st.get("momentum_buffer") is None:        # (a state written by torch before the parameter's first step)
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        n = len(live)
        L.sgd_step(_ptrs([p.data_ptr() for p, _, _ in live]), _ptrs([g.data_ptr() for _, g, _ in live]),
                   _ptrs([st["momentum_buffer"].data_ptr() for _, _, st in live]), (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in live]), n,
                   float(group["lr"]), lr_dev, float(group["momentum"]), float(group["weight_decay"]), stream)
