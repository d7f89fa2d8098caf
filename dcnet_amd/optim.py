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

Gradient clipping and the non-finite skip (constructor options ``max_grad_norm`` and ``skip_nonfinite`` of all three; attributes of
the optimiser, not group keys: groups and ``state_dict`` keep torch's layout).  With either set, ``step()`` first reads the gradients
of every group's live parameters once more (dcn_grad_sumsq: per-block sums of squares in double, one slot per block, no atomics),
one workgroup turns them into a four-word control block on the device (dcn_grad_clip_coef: the global L2 norm, torch's
``min(1, max_norm / (norm + 1e-6))``, an ``apply`` word, a ``skips`` counter), and the groups' updates run in their clipped form:
they take ``grad * coef`` as the gradient — what ``torch.nn.utils.clip_grad_norm_`` followed by the plain step computes — and write
nothing at all when ``skip_nonfinite`` is set and the norm is inf or NaN.  Nothing synchronises, so the whole of it is captured
into the replayed step.  What differs from torch's function: **``.grad`` is not modified** (the coefficient is applied as the
update reads the gradient; a caller that looks at ``.grad`` afterwards, as ``bench.py --dump-outputs`` does, sees raw gradients).
``opt.grad_norm`` is the last step's norm as a 0-dim device tensor (reading it is the caller's synchronisation),
``opt.skipped_steps()`` synchronises and returns the skip counter.  The skip protects parameters and optimiser state only: the
forward of the skipped step has already updated BatchNorm's running statistics.

Under ``skip_nonfinite`` the host cannot know whether a step was applied, so its ``step`` counters count calls until
``state_dict()`` — a host-synchronising moment anyway — makes them read "updates applied": Adam copies its device step words,
RMSprop (whose ``step`` is bookkeeping only) subtracts the skips it has not yet accounted for, SGD has no counter.

``clip_grad_norm_`` is the stand-alone form with torch's in-place semantics, for a caller that keeps a torch optimiser.

``AdamW`` (and ``Adam(decoupled_weight_decay=True)``, torch's spelling of the same thing) is torch 2.10's single-tensor AdamW:
``param.mul_(1 - lr * weight_decay)``, then Adam's update on the unmodified gradient (dcn_adamw_prepare + dcn_adamw_step; the factor
is formed on the device, in double, from the step's learning rate).  Groups and ``state_dict`` are ``torch.optim.AdamW``'s.

Gradient accumulation (constructor option ``accum_steps = K`` of all four classes; an attribute like ``max_grad_norm``, not a group
key).  Every K consecutive ``step()`` calls form one window.  Calls 1 ... K-1 write only an fp32 accumulation buffer per live parameter
(4 B per trained parameter): parameters, optimiser state, Adam's device step words, an attached EMA and its count keep their bits.  Call
K forms the window's gradient ``G = (((g_1 + g_2) + g_3) ... + g_K) * fl32(1/K)`` — fp32 additions in call order, one multiplication,
what K backward passes on ``loss / K`` accumulate to up to the rounding order — **writes it into the parameter's contiguous ``.grad``**
(the one place where the fused step writes ``.grad``: a post-backward reducer, or a caller who looks at ``.grad``, sees the window
mean) and applies the unchanged update to it.  Which call is which is decided on the device (dcn_accum_prepare advances a window
position in a four-word accumulation block, dcn_grad_accumulate takes its phase from it, dcn_accum_clip_coef gates the ``_clipped``
updates and the EMA through the clipping control block), so every call launches the same kernels on the same addresses and the whole
of it replays as one hipGraph.  Clipping and the non-finite skip act on ``G``: one norm per window, ``opt.grad_norm`` keeps the last
closed window's norm in between, a window whose ``G`` has a non-finite norm is skipped as a whole (one skip, EMA untouched) and the next
one starts clean — call 1 overwrites the buffers.  The learning rate is read at call K; host ``step`` counters, schedules and
``skipped_steps()`` are in units of updates.  The live set (the parameters that have a gradient) is fixed per window.  Buffers and
position are not part of ``state_dict()``; ``load_state_dict()`` and ``reset_accumulation()`` put the window back to its start.  What
accumulation does NOT emulate is a larger batch inside the model: BatchNorm's batch statistics and running-stat updates happen per
micro-batch, the sampling heads draw once per micro-batch, the contrastive losses take their negatives from one micro-batch.

``WeightEMA`` keeps an exponential moving average of a model's weights and running statistics in shadow tensors, updated by two
launches (dcn_ema_prepare + dcn_ema_update) that the fused optimisers append to their step (``opt.attach_ema(ema)``), so the update
is part of the replayed training step and a ``skip_nonfinite`` step skips it too.  ``ema.swap()`` / ``with ema.applied():`` exchange
the average with the model's tensors **in place** (dcn_tensor_swap): parameter addresses, optimiser state and a captured graph
stay valid, evaluation needs no third copy.
"""
from __future__ import annotations

import contextlib
import ctypes
import math

import torch

from .lib import lib


def _ptrs(addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


def _tables(live, keys, *more):
    """The leading arguments of an update entry point for a group's ``live`` parameters: the pointer tables of the parameters, the
    gradients, the state tensors named by ``keys`` and ``more`` (tables that follow the state's), the element counts, the count."""
    n = len(live)
    return (_ptrs([p.data_ptr() for p, _, _ in live]), _ptrs([g.data_ptr() for _, g, _ in live]),
            *(_ptrs([st[k].data_ptr() for _, _, st in live]) for k in keys), *more, (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in live]), n)


def _call(L, name, args, ctl, stream) -> None:
    """Entry point ``name`` of the library, or with a control block its ``_clipped`` form (``ctl`` in front of ``stream``); looked up
    on ``L`` at the call."""
    if ctl:
        getattr(L, name + "_clipped")(*args, ctl, stream)
    else:
        getattr(L, name)(*args, stream)


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: the device learning rates, the ``step`` bookkeeping and the walk over the groups.
    A subclass names its state in ``_new_state`` and launches one group's update in ``_launch``."""

    LR_RING = 4

    def __init__(self, params, defaults, max_grad_norm=None, skip_nonfinite: bool = False, accum_steps: int = 1):
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
            raise ValueError(f"accum_steps must be an integer >= 1, not {accum_steps!r}")
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
                raise ValueError(f"max_grad_norm must be a finite number > 0 (or None), not {max_grad_norm!r}")
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip_ws = None         # {"ctrl": the control block, "partials", "key": the live element counts the partials were sized for}
        self._skips_accounted = 0    # skips already taken off the host step counters (state_dict)
        # device_lr: the step reads each group's learning rate from a device scalar (refreshed by sync_lr()) instead of a kernel
        # argument — what a step captured into a hipGraph needs to follow a schedule (dcnet_amd.graph.GraphedTrainStep)
        self.device_lr = False
        self._lr_dev = {}
        self._stepped = []           # the "step" counters touched by the last step() (bump_steps: replays of a captured step)
        self._stepped_params = []    # ... and whose they are (load_state_dict replaces the counters)
        self._ema = None             # attach_ema: a WeightEMA whose update closes every step
        self.accum_steps = accum_steps
        self._accum = None           # {"block": the accumulation block, "ctrl": a control block of its own (no clipping), "bufs": {parameter: buffer}}
        self._accum_pos = 0          # host mirror of the window position: step() calls made in the open window
        self._accum_live = None      # the live set of the open window (ids of its parameters)
        self._pending = None         # accumulate() ran since the last step(): the live lists it worked on

    def attach_ema(self, ema) -> None:
        """Make the end of every ``step()`` call ``ema.update(ctl)`` (a ``WeightEMA``; ``None`` detaches) with the address of the step's
        clipping control block (0 without clipping): the average follows the parameters inside the step — eager or captured — and a
        step that ``skip_nonfinite`` turned into a no-op leaves the average and its update count alone.  Attach BEFORE building a
        ``GraphedTrainStep``: the capture records the launches ``step()`` makes at that moment, so an EMA attached afterwards would
        never run in the replays (and one detached afterwards would keep running).  A step without any gradient updates nothing,
        the average included.  With no EMA attached ``step()`` launches exactly what it launched before there was one."""
        if ema is not None and not isinstance(ema, WeightEMA):
            raise TypeError(f"{self._name()}.attach_ema: a dcnet_amd.optim.WeightEMA or None, not {type(ema).__name__}")
        self._ema = ema

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
        """Advance the per-parameter ``step`` counters once more (a replay of a captured step ran the device update).  With
        ``accum_steps`` > 1 the replay was one call of the window: the host's window position advances, the counters only when the
        replay closed a window — they count updates."""
        if self._advance_window() and self._stepped:
            torch._foreach_add_(self._stepped, 1)

    # ---- gradient accumulation ----------------------------------------------------------------------------------------------
    @property
    def window_position(self) -> int:
        """``step()`` calls (or replays) made in the open accumulation window: 0 ... ``accum_steps`` - 1.  A host mirror of the
        device's position; deterministic, because a skipped window still closes."""
        return self._accum_pos

    @property
    def at_boundary(self) -> bool:
        """True when the next ``step()`` (the current call, between ``accumulate()`` and ``step()``) closes a window: the call that
        updates.  Always True with ``accum_steps`` = 1."""
        return self._accum_pos == self.accum_steps - 1

    def _advance_window(self) -> bool:
        """One call of the window is done; returns whether it closed the window."""
        closes = self.at_boundary
        self._accum_pos = 0 if closes else self._accum_pos + 1
        if closes:
            self._accum_live = None
        return closes

    def reset_accumulation(self) -> None:
        """Put the accumulation window back to its start, on the device and on the host: the next ``accum_steps`` calls form a fresh
        window (its first call overwrites the buffers, so what an abandoned window gathered is never read).  Not during a capture."""
        if self._accum is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._name()}.reset_accumulation: not during a stream capture")
            self._accum["block"][:2].zero_()             # position and phase (in place: a captured step keeps reading these words)
        self._accum_pos, self._accum_live, self._pending = 0, None, None

    def _collect(self):
        """[(group index, group, live)] with ``live`` = (parameter, contiguous gradient, state) of every parameter of the group that
        has a gradient; groups without one are left out."""
        lives = []
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
            if live:
                lives.append((gi, group, live))
        return lives

    @torch.no_grad()
    def accumulate(self) -> None:
        """This call's share of the window, over the live gradients of all groups (dcn_accum_prepare + dcn_grad_accumulate): calls
        1 ... K-1 add ``.grad`` into the accumulation buffers, call K turns ``.grad`` into the window mean ``G``.  ``step()`` calls it
        itself unless it was called since the last ``step()`` — which is what a data-parallel loop does to put its all-reduce between
        the two: ``opt.accumulate()``, the reducer when ``opt.at_boundary``, ``opt.step()``.  (A non-contiguous ``.grad`` is accumulated
        through a contiguous copy, which is then the tensor that holds ``G`` and that the update reads.)  Nothing with
        ``accum_steps`` = 1."""
        if self.accum_steps == 1:
            return
        if self._pending is not None:
            raise RuntimeError(f"{self._name()}.accumulate: already called since the last step()")
        lives = self._collect()
        live_ids = tuple(id(p) for _, _, live in lives for p, _, _ in live)
        if self._accum_pos == 0:
            if not lives:
                self._pending = []
                return                   # nothing has a gradient: no window is opened
        elif live_ids != self._accum_live:
            raise RuntimeError(f"{self._name()}: the set of parameters that have a gradient changed inside an accumulation window (call "
                               f"{self._accum_pos + 1} of {self.accum_steps}): the live set is fixed per window; reset_accumulation() abandons the window")
        pairs = [(p, g) for _, _, live in lives for p, g, _ in live]
        dev = pairs[0][0].device
        if any(p.device != dev for p, _ in pairs):
            raise RuntimeError(f"{self._name()}: accum_steps > 1 needs all parameters on one device (one window position)")
        capturing = torch.cuda.is_current_stream_capturing()
        if self._accum is None or self._accum["block"].device != dev:
            if capturing:
                raise RuntimeError(f"{self._name()}: the first accumulating step cannot be a captured one (its accumulation block and buffers "
                                   "are allocated then); run an eager step first")
            self._accum = {"block": torch.zeros(4, dtype=torch.int32, device=dev), "ctrl": torch.zeros(4, dtype=torch.int32, device=dev), "bufs": {}}
        bufs = self._accum["bufs"]
        for p, _ in pairs:
            if p not in bufs:
                if capturing:
                    raise RuntimeError(f"{self._name()}: a parameter joined the accumulation inside a capture (its buffer is allocated at its "
                                       "first eager accumulating step); run an eager window first")
                bufs[p] = torch.empty_like(p, memory_format=torch.contiguous_format)
        L = lib()
        stream = torch.cuda.current_stream().cuda_stream
        n = len(pairs)
        L.accum_prepare(self._accum["block"].data_ptr(), self.accum_steps, stream)
        L.grad_accumulate(_ptrs([bufs[p].data_ptr() for p, _ in pairs]), _ptrs([g.data_ptr() for _, g in pairs]),
                          (ctypes.c_int64 * n)(*[g.numel() for _, g in pairs]), n, self._accum["block"].data_ptr(), stream)
        self._accum_live = live_ids
        self._pending = lives

    def _name(self) -> str:
        return f"dcnet_amd.optim.{type(self).__name__}"

    def _new_state(self, p) -> dict:
        raise NotImplementedError

    def _launch(self, L, gi, group, live, lr_dev, ctl, stream) -> None:
        """One group's update.  ``live``: (parameter, contiguous gradient, state) of every parameter that has a gradient; ``ctl``: the
        address of the clipping control block, 0 for the plain step."""
        raise NotImplementedError

    # ---- clipping / skip ---------------------------------------------------------------------------------------------------
    @property
    def clipping(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    @property
    def grad_norm(self):
        """The global gradient norm of the last step, a 0-dim fp32 device tensor (a view of the control block: the next step
        overwrites it; reading it synchronises).  None before the first step and without the options."""
        return None if self._clip_ws is None else self._clip_ws["ctrl"].view(torch.float32)[0]

    def skipped_steps(self) -> int:
        """How many steps ``skip_nonfinite`` has turned into no-ops so far (synchronises)."""
        return 0 if self._clip_ws is None else int(self._clip_ws["ctrl"][3].item())

    def _norm_launches(self, L, grads, stream) -> int:
        """The sum-of-squares launches over ``grads`` and the coefficient launch (with ``accum_steps`` > 1 its gated form: the norm is
        the window's, formed on the boundary call); returns the control block's address."""
        numel = [g.numel() for g in grads]
        key = (grads[0].device, tuple(numel))
        if any(g.device != key[0] for g in grads):
            raise RuntimeError(f"{self._name()}: max_grad_norm / skip_nonfinite need all gradients on one device (one norm, one control block)")
        ws = self._clip_ws
        if ws is None or ws["key"] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._name()}: the first clipped step (or the first one with another set of gradients) cannot be a captured "
                                   "one (its workspace is allocated then); run an eager step first")
            n = len(numel)
            slots = L.grad_sumsq_slots((ctypes.c_int64 * n)(*numel), n)
            if slots <= 0:
                raise RuntimeError(f"{self._name()}: dcn_grad_sumsq_slots failed")
            ctrl = ws["ctrl"] if ws is not None and ws["ctrl"].device == key[0] else torch.zeros(4, dtype=torch.int32, device=key[0])
            ws = self._clip_ws = {"ctrl": ctrl, "partials": torch.empty(slots, dtype=torch.float64, device=key[0]), "key": key}
        n = len(numel)
        part = ws["partials"]
        L.grad_sumsq(_ptrs([g.data_ptr() for g in grads]), (ctypes.c_int64 * n)(*numel), n, part.data_ptr(), part.numel(), stream)
        max_norm = self.max_grad_norm if self.max_grad_norm is not None else math.inf
        if self.accum_steps > 1:
            L.accum_clip_coef(part.data_ptr(), part.numel(), max_norm, int(self.skip_nonfinite), self._accum["block"].data_ptr(), ws["ctrl"].data_ptr(), stream)
        else:
            L.grad_clip_coef(part.data_ptr(), part.numel(), max_norm, int(self.skip_nonfinite), ws["ctrl"].data_ptr(), stream)
        return ws["ctrl"].data_ptr()

    def _reconcile_steps(self) -> None:
        """Make the host ``step`` counters read "updates applied" (``skip_nonfinite``; synchronises).  Here: counters that counted
        every call lose the skips not yet accounted for; Adam copies its device step words instead."""
        skips = self.skipped_steps()
        new = skips - self._skips_accounted
        self._skips_accounted = skips
        if new > 0:
            for st in self.state.values():
                if "step" in st:
                    st["step"].sub_(new).clamp_(min=0)

    def state_dict(self):
        if self.skip_nonfinite and self._clip_ws is not None:
            self._reconcile_steps()
        return super().state_dict()

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
        accumulating = self.accum_steps > 1
        if accumulating:
            # this call's share of the window first (unless the caller ran it already, to put a reducer between the two): on the
            # boundary call .grad then holds the window mean, which is what the norm and the update read
            if self._pending is None:
                self.accumulate()
            lives, self._pending = self._pending, None
        else:
            lives = self._collect()
        if not lives:
            return loss
        stream = torch.cuda.current_stream().cuda_stream
        updates = self.at_boundary                 # (host bookkeeping only: every call launches the same kernels)
        ctl = 0
        if self.clipping:
            # ONE norm over the gradients of every group (what torch's function gives for model.parameters()), then the coefficient
            grads = [g for _, _, live in lives for _, g, _ in live if g.numel() > 0]
            if grads:
                ctl = self._norm_launches(L, grads, stream)
        if accumulating and not ctl:
            # no norm was asked for (or every gradient is empty): the control block still gates the updates, with a coefficient of
            # exactly 1 — g * 1.0f keeps g's bits, so the clipped update on the boundary is the plain one
            ctl = self._accum["ctrl"].data_ptr()
            L.accum_clip_coef(0, 0, math.inf, 0, self._accum["block"].data_ptr(), ctl, stream)
        for gi, group, live in lives:
            lr_dev = self._lr_dev[gi]["dev"].data_ptr() if self.device_lr else 0
            self._launch(L, gi, group, live, lr_dev, ctl, stream)
            for p, _, st in live:
                if "step" in st:
                    if updates:
                        st["step"] += 1
                    self._stepped.append(st["step"]); self._stepped_params.append(p)
        if self._ema is not None:
            self._ema.update(ctl)
        self._advance_window()
        return loss

    def load_state_dict(self, state_dict) -> None:
        """torch's, then: ``step`` counters as the host scalars torch's own default keeps (whatever device the writer had them on), and
        the bookkeeping of ``bump_steps`` pointed at the counters that replaced the old ones.  An open accumulation window is
        abandoned (``reset_accumulation``): buffers and position are not part of a state."""
        if self._accum is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._name()}: load_state_dict during a stream capture cannot reset the accumulation window")
        super().load_state_dict(state_dict)
        self.reset_accumulation()
        for st in self.state.values():
            if "step" in st:
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
        self._stepped_params = [p for p in self._stepped_params if "step" in self.state.get(p, {})]
        self._stepped = [self.state[p]["step"] for p in self._stepped_params]
        self._skips_accounted = self.skipped_steps()     # the loaded counters are right as they are: earlier skips are not theirs


class RMSprop(_FusedOptimizer):
    def __init__(self, params, lr: float = 1e-2, alpha: float = 0.99, eps: float = 1e-8, weight_decay: float = 0.0,
                 momentum: float = 0.0, centered: bool = False, max_grad_norm=None, skip_nonfinite: bool = False, accum_steps: int = 1):
        if momentum != 0.0 or centered:
            raise NotImplementedError("dcnet_amd.optim.RMSprop implements momentum=0, centered=False (the reference's setting)")
        if lr < 0 or eps < 0 or alpha < 0 or weight_decay < 0:
            raise ValueError("invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=0.0, centered=False),
                         max_grad_norm, skip_nonfinite, accum_steps)

    def _new_state(self, p):
        return {"step": torch.zeros((), dtype=torch.float32), "square_avg": torch.zeros_like(p, memory_format=torch.preserve_format)}

    def _launch(self, L, gi, group, live, lr_dev, ctl, stream):
        _call(L, "rmsprop_step", (*_tables(live, ("square_avg",)), float(group["lr"]), lr_dev, float(group["alpha"]), float(group["eps"]),
                                  float(group["weight_decay"])), ctl, stream)


class Adam(_FusedOptimizer):
    """``torch.optim.Adam`` (``amsgrad=False``, ``maximize=False``; train_DCNet.py:528-529) as dcn_adam_prepare + dcn_adam_step.

    The bias corrections depend on the step count, and a replayed hipGraph must advance it without the host.  So beside the host
    ``step`` scalar of the state (torch's layout: what ``state_dict()`` carries) every parameter has a device step word, which the
    step's own first launch advances and turns into the step's two scalars (``lr / (1 - beta1^t)``, ``1 / sqrt(1 - beta2^t)``) — in
    an eager step and in a captured one alike.  The words are made from the host counters when a group first steps and again by
    ``load_state_dict``; a parameter without a gradient is left out of the launches and keeps its count, as in torch.

    ``decoupled_weight_decay=True`` (constructor argument and group key, torch's) makes a group's step AdamW's: dcn_adamw_prepare +
    dcn_adamw_step, three scalars per parameter instead of two (the third: ``1 - lr * weight_decay``).  A group without it runs the
    entry points, kernels and two-scalar slots it always ran."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, maximize: bool = False, max_grad_norm=None, skip_nonfinite: bool = False,
                 decoupled_weight_decay: bool = False, accum_steps: int = 1):
        if amsgrad or maximize:
            raise NotImplementedError(f"dcnet_amd.optim.{type(self).__name__} implements amsgrad=False, maximize=False (the reference's setting)")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid hyper-parameter")
        # (the keys and values of torch.optim.Adam's groups: a state_dict loaded into torch's class brings its groups along)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled_weight_decay)),
                         max_grad_norm, skip_nonfinite, accum_steps)
        self._tables = {}            # group index -> device step words and scalar slots of the group's parameters

    def _new_state(self, p):
        return {"step": torch.zeros((), dtype=torch.float32), "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
                "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}

    def _host_steps(self, group):
        return torch.tensor([int(self.state[p]["step"]) if "step" in self.state.get(p, {}) else 0 for p in group["params"]], dtype=torch.int32)

    def _table(self, gi, group, device):
        tab = self._tables.get(gi)
        width = 3 if group.get("decoupled_weight_decay") else 2
        if tab is not None and len(tab["index"]) == len(group["params"]) and tab["scal"].shape[1] != width:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._name()}: decoupled_weight_decay of a group changed: run an eager step before capturing one")
            tab["scal"] = torch.zeros(len(group["params"]), width, dtype=torch.float32, device=device)       # (the step words stay)
        if tab is None or len(tab["index"]) != len(group["params"]):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._name()}: the first step of a group cannot be a captured one (its device step words are made "
                                   "from the host counters); run an eager step first")
            n = len(group["params"])
            tab = {"steps": self._host_steps(group).to(device), "scal": torch.zeros(n, width, dtype=torch.float32, device=device),
                   "index": {id(p): i for i, p in enumerate(group["params"])}}
            self._tables[gi] = tab
        return tab

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError(f"{self._name()}: amsgrad / maximize are not implemented")

    def _reconcile_steps(self) -> None:
        """The device step words are the truth under ``skip_nonfinite`` (a skipped step does not advance them): copy them into the host
        counters, in place — ``bump_steps`` keeps pointing at the same tensors."""
        self._skips_accounted = self.skipped_steps()
        for gi, tab in self._tables.items():
            words = tab["steps"].tolist()
            for p in self.param_groups[gi]["params"]:
                st = self.state.get(p, {})
                if "step" in st and id(p) in tab["index"]:
                    st["step"].fill_(float(words[tab["index"][id(p)]]))

    def _launch(self, L, gi, group, live, lr_dev, ctl, stream):
        self._check_group(group)
        tab = self._table(gi, group, live[0][0].device)
        rows = [tab["index"][id(p)] for p, _, _ in live]
        s0, c0 = tab["steps"].data_ptr(), tab["scal"].data_ptr()
        scal = _ptrs([c0 + 4 * tab["scal"].shape[1] * r for r in rows])
        b1, b2 = (float(b) for b in group["betas"])
        # weight_decay: AdamW's goes into the prepare launch (the third scalar), Adam's into the update
        decoupled, wd = bool(group.get("decoupled_weight_decay")), (float(group["weight_decay"]),)
        kind = "adamw" if decoupled else "adam"
        _call(L, kind + "_prepare", (_ptrs([s0 + 4 * r for r in rows]), scal, len(live), float(group["lr"]), lr_dev, b1, b2, *(wd if decoupled else ())),
              ctl, stream)
        _call(L, kind + "_step", (*_tables(live, ("exp_avg", "exp_avg_sq"), scal), b1, b2, float(group["eps"]), *(() if decoupled else wd)), ctl, stream)

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


class AdamW(Adam):
    """``torch.optim.AdamW``: ``Adam`` with ``decoupled_weight_decay=True`` and torch's defaults (``lr=1e-3``, ``weight_decay=1e-2``).
    Groups and ``state_dict`` are ``torch.optim.AdamW``'s, so states load both ways."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, maximize: bool = False, max_grad_norm=None, skip_nonfinite: bool = False, accum_steps: int = 1):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, decoupled_weight_decay=True, accum_steps=accum_steps)


class SGD(_FusedOptimizer):
    """``torch.optim.SGD`` with momentum (``dampening=0``, ``nesterov=False``; train_DCNet.py:530-531) as dcn_sgd_step.  torch's SGD
    keeps no ``step`` in its state, and neither does this one: ``bump_steps()`` has nothing to advance."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, maximize: bool = False, max_grad_norm=None, skip_nonfinite: bool = False, accum_steps: int = 1):
        if dampening != 0 or nesterov or maximize:
            raise NotImplementedError("dcnet_amd.optim.SGD implements dampening=0, nesterov=False, maximize=False (the reference's setting)")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False,
                                      foreach=None, differentiable=False, fused=None), max_grad_norm, skip_nonfinite, accum_steps)

    def _new_state(self, p):
        return {"momentum_buffer": torch.zeros_like(p, memory_format=torch.preserve_format)}

    def _launch(self, L, gi, group, live, lr_dev, ctl, stream):
        if group.get("dampening") or group.get("nesterov") or group.get("maximize"):
            raise NotImplementedError(f"{self._name()}: dampening / nesterov / maximize are not implemented")
        for p, _, st in live:
            if st.get("momentum_buffer") is None:        # (a state written by torch before the parameter's first step)
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        _call(L, "sgd_step", (*_tables(live, ("momentum_buffer",)), float(group["lr"]), lr_dev, float(group["momentum"]), float(group["weight_decay"])),
              ctl, stream)


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False):
    """``torch.nn.utils.clip_grad_norm_`` on the device, for a caller that keeps a torch optimiser: the gradients of ``parameters`` (a
    tensor or an iterable; those without a gradient are left out) are scaled **in place** by ``min(1, max_norm / (norm + 1e-6))`` of
    their global L2 norm, and the norm is returned as a 0-dim fp32 device tensor.  The norm is the one the fused steps compute
    (sums of squares in double: exact to the final fp32 rounding, finite wherever the true norm is, the same bits in every run),
    in ~3 launches per 32 tensors instead of torch's per-tensor norms, stack and foreach multiply.  Nothing synchronises unless
    ``error_if_nonfinite`` is set: that form reads the norm on the host (the only synchronising one) and raises ``RuntimeError`` on
    inf / NaN before any gradient is touched.  Only ``norm_type=2``; contiguous fp32 CUDA gradients only."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("dcnet_amd.optim.clip_grad_norm_ implements norm_type=2 only")
    max_norm = float(max_norm)
    if not max_norm > 0:
        raise ValueError(f"max_norm must be > 0, not {max_norm!r}")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
            raise RuntimeError("dcnet_amd.optim.clip_grad_norm_: contiguous fp32 CUDA parameters only (no CPU path)")
    grads = [g for g in grads if g.numel() > 0]
    if not grads:
        return torch.tensor(0.0)
    if any(g.device != grads[0].device for g in grads):
        raise RuntimeError("dcnet_amd.optim.clip_grad_norm_: gradients on more than one device")
    L = lib()
    dev, n = grads[0].device, len(grads)
    numel = (ctypes.c_int64 * n)(*[g.numel() for g in grads])
    ptrs = _ptrs([g.data_ptr() for g in grads])
    slots = L.grad_sumsq_slots(numel, n)
    if slots <= 0:
        raise RuntimeError("dcnet_amd.optim.clip_grad_norm_: dcn_grad_sumsq_slots failed")
    with torch.cuda.device(dev):
        part = torch.empty(slots, dtype=torch.float64, device=dev)
        ctrl = torch.zeros(4, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        L.grad_sumsq(ptrs, numel, n, part.data_ptr(), slots, stream)
        L.grad_clip_coef(part.data_ptr(), slots, max_norm, 0, ctrl.data_ptr(), stream)
        norm = ctrl.view(torch.float32)[0]
        if error_if_nonfinite and not math.isfinite(float(norm)):
            raise RuntimeError(f"The total norm of order 2.0 for gradients from `parameters` is non-finite ({float(norm)}), so it cannot be clipped")
        L.grad_scale(ptrs, numel, n, ctrl.data_ptr(), stream)
    return norm


def weight_at(t: int, decay: float, tau: float) -> float:
    """The weight ``w_t = 1 - d_t`` of the ``t``-th applied update (t = 1, 2, ...) of a ``WeightEMA``: ``shadow <- lerp(shadow, theta, w_t)``
    with ``d_t = decay * (1 - exp(-t / tau))`` for ``tau > 0`` (the warm-up ramp of the YOLO recipes: early averages follow the weights
    closely) and ``d_t = decay`` for ``tau == 0``.  Host arithmetic in double — what dcn_ema_prepare rounds to fp32 on the device."""
    return 1.0 - (decay * (1.0 - math.exp(-t / tau)) if tau > 0 else decay)


class WeightEMA:
    """An exponential moving average of a model's weights, kept on the device and updated inside the fused training step.

    ``WeightEMA(model, decay=0.9999, tau=2000.0)`` (``model`` may be DDP-wrapped) shadows every floating-point entry of
    ``model.state_dict()`` — parameters and BatchNorm running statistics; integer buffers such as ``num_batches_tracked`` are not
    shadowed.  The shadows start as copies (``shadow_0 = theta_0``); they, the device step word, the weight word and the pointer
    tables exist from construction on, so an update allocates nothing and can be captured.  Contiguous fp32 CUDA tensors only.  The
    tables hold the addresses of the model's tensors: like a captured graph, the EMA is valid while they stay where they are
    (``load_state_dict`` and the optimisers write in place; ``model.to(...)`` moves them).

    ``update(ctl=0)``   ``shadow <- lerp(shadow, theta, w_t)``, ``w_t = weight_at(t, decay, tau)`` with ``t`` the count of applied
                        updates, advanced on the device (dcn_ema_prepare + dcn_ema_update on the current stream).  ``ctl``: the address
                        of a clipping control block whose ``apply`` word gates both.  ``opt.attach_ema(ema)`` makes the fused
                        optimisers call it at the end of ``step()``; with a torch optimiser call it yourself after ``step()``.
    ``swap()``          exchanges shadows and model tensors in place (dcn_tensor_swap).  ``swapped`` tells which way round they are;
                        ``update`` raises while swapped.
    ``applied()``       ``with ema.applied(): evaluate(model, ...)`` — swap, yield, swap back; the round trip is bitwise.
    ``copy_to(model)``  the one-way case: the averages overwrite ``model``'s tensors (this model or another of the same layout).
    ``updates()``       the device step word (synchronises).
    ``state_dict()`` / ``load_state_dict()``   ``{"decay", "tau", "updates", "shadow": {state_dict key: tensor}}``; loading copies into the
                        existing shadows and step word in place (a captured update keeps reading them), strict on keys and shapes.
                        ``decay`` and ``tau`` are recorded, the constructor's stay in force."""

    weight_at = staticmethod(weight_at)

    def __init__(self, model, decay: float = 0.9999, tau: float = 2000.0):
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightEMA: decay must be a number in [0, 1), not {decay!r}")
        if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not (tau >= 0.0 and math.isfinite(tau)):
            raise ValueError(f"WeightEMA: tau must be a finite number >= 0, not {tau!r}")
        self.decay, self.tau = float(decay), float(tau)
        core = model.module if hasattr(model, "module") else model
        self._keys, self._src, self._shadow = [], [], []
        for k, v in core.state_dict().items():
            if not v.is_floating_point():
                continue
            if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
                raise RuntimeError(f"dcnet_amd.optim.WeightEMA: contiguous fp32 CUDA tensors only (no CPU path): {k}")
            self._keys.append(k); self._src.append(v.detach())
        if not self._src:
            raise RuntimeError("dcnet_amd.optim.WeightEMA: the model has no floating-point tensor to average")
        self.device = self._src[0].device
        if any(v.device != self.device for v in self._src):
            raise RuntimeError("dcnet_amd.optim.WeightEMA: the model's tensors live on more than one device")
        for v in self._src:
            s = torch.empty_like(v, memory_format=torch.contiguous_format)
            s.copy_(v)
            self._shadow.append(s)
        self._step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._w = torch.zeros(1, dtype=torch.float32, device=self.device)
        n = self._count = len(self._src)
        self._p_shadow = _ptrs([s.data_ptr() for s in self._shadow])
        self._p_src = _ptrs([v.data_ptr() for v in self._src])
        self._numel = (ctypes.c_int64 * n)(*[v.numel() for v in self._src])
        self._swapped = False

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    @property
    def swapped(self) -> bool:
        """True while the model holds the averages and the shadows hold the raw weights."""
        return self._swapped

    @property
    def shadow(self) -> dict:
        """state_dict key -> shadow tensor (the tensors themselves)."""
        return dict(zip(self._keys, self._shadow))

    def update(self, ctl: int = 0) -> None:
        if self._swapped:
            raise RuntimeError("dcnet_amd.optim.WeightEMA.update: the model holds the averages (swap() / applied()): swap back first")
        L = lib()
        stream = self._stream()
        L.ema_prepare(self._step.data_ptr(), self._w.data_ptr(), self.decay, self.tau, ctl, stream)
        L.ema_update(self._p_shadow, self._p_src, self._numel, self._count, self._w.data_ptr(), ctl, stream)

    def swap(self) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dcnet_amd.optim.WeightEMA.swap: not during a stream capture")
        lib().tensor_swap(self._p_shadow, self._p_src, self._numel, self._count, self._stream())
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def applied(self):
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def updates(self) -> int:
        return int(self._step.item())

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"dcnet_amd.optim.WeightEMA.{what}: the shadows hold the raw weights (swap() / applied()): swap back first")

    def state_dict(self) -> dict:
        self._not_swapped("state_dict")
        return {"decay": self.decay, "tau": self.tau, "updates": self.updates(), "shadow": self.shadow}

    def load_state_dict(self, state: dict) -> None:
        self._not_swapped("load_state_dict")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dcnet_amd.optim.WeightEMA.load_state_dict: not during a stream capture")
        src = {(k[7:] if k.startswith("module.") else k): v for k, v in state["shadow"].items()}
        missing, unexpected = [k for k in self._keys if k not in src], [k for k in src if k not in set(self._keys)]
        if missing or unexpected:
            raise KeyError(f"WeightEMA.load_state_dict: missing keys {missing[:5]}{'...' if len(missing) > 5 else ''}, "
                           f"unexpected keys {unexpected[:5]}{'...' if len(unexpected) > 5 else ''}")
        for k, s in zip(self._keys, self._shadow):
            if tuple(src[k].shape) != tuple(s.shape):
                raise ValueError(f"WeightEMA.load_state_dict: {k} has shape {tuple(src[k].shape)}, the shadow {tuple(s.shape)}")
        updates = int(state["updates"])
        if updates < 0:
            raise ValueError(f"WeightEMA.load_state_dict: updates = {updates}")
        with torch.no_grad():
            for k, s in zip(self._keys, self._shadow):
                s.copy_(src[k])
            self._step.fill_(updates)

    @torch.no_grad()
    def copy_to(self, model) -> None:
        self._not_swapped("copy_to")
        core = model.module if hasattr(model, "module") else model
        dst = {k: v for k, v in core.state_dict().items() if v.is_floating_point()}
        if list(dst) != self._keys:
            raise KeyError("WeightEMA.copy_to: the model's floating-point state_dict keys are not the shadowed ones")
        for k, s in zip(self._keys, self._shadow):
            if tuple(dst[k].shape) != tuple(s.shape):
                raise ValueError(f"WeightEMA.copy_to: {k} has shape {tuple(dst[k].shape)}, the shadow {tuple(s.shape)}")
            dst[k].copy_(s)
